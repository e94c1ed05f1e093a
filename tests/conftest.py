import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def z():
    """The product package (zlib.es_amd/ loaded as zlibes_amd); builds the HIP library if missing."""
    # torch before the library, whichever test asks first: PyTorch ships its own HIP runtime, and libzes_hip.so
    # (NEEDED libamdhip64.so.7) shares it only if it is already loaded.  The other way round the process gets two HIP
    # runtimes, and the one that opens the GPU second fails (zes_init: ZES_E_DEVICE in every GPU test after a CPU test).
    import torch  # noqa: F401

    import __graft_entry__ as ge

    mod = ge.load()
    if not os.path.exists(os.path.join(ROOT, "zlib.es_amd", "libzes_hip.so")):
        mod.build()
    return mod


@pytest.fixture(scope="session")
def oracle():
    import _oracle

    _oracle.lib()
    return _oracle


@pytest.fixture(scope="session")
def gpu(z):
    """Initialised device; fails (not skips) when the HIP path cannot run on a GPU box."""
    import torch

    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    z.init(0)
    return torch.device("cuda:0")

