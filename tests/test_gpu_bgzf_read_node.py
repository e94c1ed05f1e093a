"""bgzfIndex() and bgzfRead() of the N-API façade under Node (tests/host_node_bgzf_read_test.js)."""
import gzip as pygzip
import os
import shutil
import subprocess

import pytest

import _bgzf
import _bgzf_index_cases as cases
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_node_bgzf_read(gpu, z, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    a = z.gen("itext", 71, 3 * 40000 + 777).tobytes()
    blob = _bgzf.bgzf([a[i:i + 40000] for i in range(0, len(a), 40000)], level=[6, 0, 9, 1])
    assert pygzip.decompress(blob) == a
    coff, uoff = cases.expected(blob)
    (tmp_path / "file.gz").write_bytes(blob)
    (tmp_path / "compressed.txt").write_text(" ".join(str(int(v)) for v in coff))
    (tmp_path / "uncompressed.txt").write_text(" ".join(str(int(v)) for v in uoff))
    ranges = [(100, 50), (39990, 40020), (len(a) - 5, 100)]  # inside a member, across three, clipped at the end
    (tmp_path / "ranges.txt").write_text("\n".join("%d %d" % r for r in ranges))
    for k, (pos, n) in enumerate(ranges):
        (tmp_path / ("slice%d.bin" % k)).write_bytes(a[pos:pos + n])
    env = dict(os.environ, ZES_BGZF_READ_DIR=str(tmp_path))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_bgzf_read_test.js")], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "bgzf read node checks passed" in out.stdout
