"""The { verify: true } option of the N-API façade's inflate forms under Node (tests/host_node_verify_test.js)."""
import os
import shutil
import subprocess
import zlib as pz

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_node_verify(gpu, z, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    raw = z.gen("itext", 88, 150000).tobytes()
    good = pz.compress(raw)
    bad = bytearray(good)
    bad[-2] ^= 0x04
    (tmp_path / "raw.bin").write_bytes(raw)
    (tmp_path / "good.z").write_bytes(good)
    (tmp_path / "bad.z").write_bytes(bytes(bad))
    env = dict(os.environ, ZES_VERIFY_DIR=str(tmp_path))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_verify_test.js")], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "verify node checks passed" in out.stdout
