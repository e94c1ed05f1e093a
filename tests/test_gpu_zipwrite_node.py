"""zip() of the N-API façade under Node (tests/host_node_zipwrite_test.js): a few entries of the case list of tests/_zipwrite.py,
names as strings and as bytes, against the archive the builder and the CPU oracle give, and back through zipIndex() / zipRead()."""
import json
import os
import shutil
import subprocess

import pytest

import _zipwrite as W
from conftest import ROOT

pytestmark = pytest.mark.gpu

PICK = [b"text/48.txt", b"text/32.txt", b"text/1000.txt", b"random/4096.bin", "grüß/日本.txt".encode("utf-8"), b"refused/1", b"zero/64", b"text/300000.txt",
        (b"long/" + b"n" * 300)[:300], b"", b"same/one", b"same/two"]


def test_node_zip_write(gpu, z, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    by_name = dict(W.cases(z))
    entries = [(n, by_name[n]) for n in PICK]
    files = []
    for k, (n, d) in enumerate(entries):
        (tmp_path / ("%d.bin" % k)).write_bytes(d)
        f = dict(data="%d.bin" % k, method=W.entry(n, d)["method"])
        f.update(dict(nameHex=n.hex()) if k % 3 == 2 or not n else dict(name=n.decode("utf-8")))  # as bytes, or as a string
        files.append(f)
    assert {f["method"] for f in files} == {0, 8} and any("name" in f and W.name_flags(n) for f, (n, _) in zip(files, entries))
    (tmp_path / "want.zip").write_bytes(W.expect(entries))
    (tmp_path / "expected.json").write_text(json.dumps(dict(files=files)))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_zipwrite_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_ZIP_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "zip write node checks passed" in out.stdout
