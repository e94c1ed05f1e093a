"""zipIndex() of the N-API façade under Node, without a GPU (tests/host_node_zip_index_test.js): the archives of the CPU index
tests against what CPython's zipfile lists, the reject list's messages, and the façade's TypeErrors."""
import json
import os
import shutil
import subprocess

import pytest

import _zip
from conftest import ROOT


def test_node_zip_index(z, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    archives, rejects = [], []
    for k, (what, b) in enumerate(_zip.cpython_archives().items()):
        (tmp_path / ("%d.zip" % k)).write_bytes(b)
        st, ent, names = _zip.index_rule(b)
        info = _zip.infolist(b)
        assert st == 0 and len(info) == len(ent)
        archives.append(dict(what=what, file="%d.zip" % k, entries=[
            dict(name=zi["name"] if zi["flags"] & 0x800 else n.decode("latin1"), nameHex=n.hex(), method=zi["method"], flags=zi["flags"], csize=zi["csize"],
                 usize=zi["usize"], crc=zi["crc"], hdr_off=zi["hdr_off"]) for zi, n in zip(info, names)]))
    for k, (what, (b, status, _)) in enumerate(_zip.reject_cases().items()):
        if status:
            (tmp_path / ("r%d.zip" % k)).write_bytes(b)
            rejects.append(dict(what=what, file="r%d.zip" % k, message=z.strerror(status)))
    assert {r["message"] for r in rejects} == {z.strerror(_zip.ZES_E_ZIP), z.strerror(_zip.ZES_E_UNSUPPORTED)}
    name = bytes([0x66, 0xE9, 0x80, 0xFF, 0x2F, 0x78])  # no flag bit 11: neither UTF-8 nor ASCII
    (tmp_path / "latin1.zip").write_bytes(_zip.build([_zip.entry(name, b"some bytes")]))
    (tmp_path / "expected.json").write_text(json.dumps(dict(archives=archives, rejects=rejects, latin1=dict(file="latin1.zip", name=name.decode("latin1")))))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_zip_index_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_ZIP_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "zip index node checks passed" in out.stdout
