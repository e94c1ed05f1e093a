"""gzipBatch() and gunzipBatch() of the N-API façade under Node (tests/host_node_gzip_batch_test.js): round trips, the bytes of
gzip(), a mixed batch with per-file Errors, the argument errors, and — handed over in a directory — the writer's case list with
the files that tests/_gzip_batch.py's builder gives and the reader's files of both routes with the Python call's verdicts."""
import json
import os
import shutil
import subprocess

import pytest

import _gzip_batch as G
import _gzip_batch_poison as GP
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_node_gzip_batch(gpu, z, oracle, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    items = []
    for k, (name, data) in enumerate(G.writer_cases(z)):
        (tmp_path / ("%d.in" % k)).write_bytes(data)
        (tmp_path / ("%d.gz" % k)).write_bytes(G.expect(data)[0])
        items.append(dict(name=name, input="%d.in" % k, file="%d.gz" % k))
    files = []
    blobs = [f for f, _ in GP.reader_files(z)]
    py = z.gunzip_batch(blobs)
    for k, (f, got) in enumerate(zip(blobs, py)):
        (tmp_path / ("r%d.gz" % k)).write_bytes(f)
        row = dict(name="file %d" % k, file="r%d.gz" % k)
        if isinstance(got, Exception):
            row["message"] = z.strerror(got.code)
        else:
            (tmp_path / ("r%d.out" % k)).write_bytes(got.tobytes())
            row["plain"] = "r%d.out" % k
        files.append(row)
    want = [w for _, w in GP.reader_files(z)]
    assert [("err", g.code) if isinstance(g, Exception) else ("out", len(g), GP.P.sha(g)) for g in py] == want
    assert sum(1 for r in files if "message" in r) == 8
    (tmp_path / "expected.json").write_text(json.dumps(dict(items=items, files=files)))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_gzip_batch_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_GZB_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "gzip batch node checks passed" in out.stdout
