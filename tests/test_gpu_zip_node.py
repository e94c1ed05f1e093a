"""zipIndex() and zipRead() of the N-API façade under Node (tests/host_node_zip_test.js): the standard and the failure archive
of tests/_zip.py, with an Error in the place of every entry that does not check out."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _zip
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_node_zip_read(gpu, z, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    blob, plain, _ = _zip.standard(lambda d: z.deflate_raw(np.frombuffer(d, dtype=np.uint8)).tobytes())
    fblob, plan = _zip.failures()
    archives = []
    for tag, b, rows in (("standard", blob, [(0, p) for p in plain]), ("failure", fblob, [(want, data) for _, want, data in plan])):
        (tmp_path / (tag + ".zip")).write_bytes(b)
        entries = []
        for k, (want, data) in enumerate(rows):
            if want == 0:
                (tmp_path / ("%s.%d.bin" % (tag, k))).write_bytes(data)
                entries.append(dict(plain="%s.%d.bin" % (tag, k)))
            else:
                entries.append(dict(messages=[z.strerror(s) for s in (want if isinstance(want, tuple) else (want,))]))
        archives.append(dict(file=tag + ".zip", entries=entries))
    (tmp_path / "expected.json").write_text(json.dumps(dict(archives=archives)))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_zip_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_ZIP_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "zip read node checks passed" in out.stdout
