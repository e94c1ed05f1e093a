"""gunzip() of the N-API façade on a BGZF file, under Node (tests/host_node_bgzf_test.js)."""
import gzip as pygzip
import os
import shutil
import subprocess

import pytest

import _bgzf
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_node_gunzip_of_bgzf(gpu, z, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    a = z.gen("itext", 47, 3 * 65280 + 777).tobytes()
    chunks = [a[i:i + 65280] for i in range(0, len(a), 65280)]
    blob = _bgzf.bgzf(chunks)
    assert pygzip.decompress(blob) == a
    (tmp_path / "bgzf.gz").write_bytes(blob)
    (tmp_path / "plain.gz").write_bytes(pygzip.compress(a, mtime=0))
    (tmp_path / "want.bin").write_bytes(a)
    (tmp_path / "members.txt").write_text(str(len(chunks) + 1))
    env = dict(os.environ, ZES_BGZF_DIR=str(tmp_path))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_bgzf_test.js")], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "bgzf node checks passed" in out.stdout
