"""zip() of the N-API façade under Node, without a GPU (tests/host_node_zipwrite_args_test.js): the archive of no files, which
needs no device, and the façade's TypeErrors."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_node_zip_arguments(z):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_zipwrite_args_test.js")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "zip write argument checks passed" in out.stdout
