"""bgzip() and bgzipIndex() of the N-API façade under Node (tests/host_node_bgzip_test.js)."""
import os
import shutil
import subprocess

import pytest

import _bgzf
import _bgzip_expect as E
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_node_bgzip(gpu, z, oracle, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    # a text chunk, an incompressible one (stored), a short text tail
    a = z.gen("itext", 48, E.CHUNK).tobytes() + z.gen("xorshift", 49, E.CHUNK).tobytes() + z.gen("itext", 50, 777).tobytes()
    want = E.expect(a)
    assert E.plan(a)[2] == [False, True, False]
    (tmp_path / "in.bin").write_bytes(a)
    (tmp_path / "want.gz").write_bytes(want)
    (tmp_path / "offsets.txt").write_text(" ".join(str(pos) for pos, _, _ in _bgzf.walk(want)))
    env = dict(os.environ, ZES_BGZIP_DIR=str(tmp_path))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_bgzip_test.js")], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "bgzip node checks passed" in out.stdout
