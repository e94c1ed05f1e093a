"""pngEncode() and pngEncodeBatch() of the N-API façade under Node (tests/host_node_pngwrite_test.js): images of
tests/_pngwrite.py, the files byte for byte those of the Python call (which tests/test_gpu_pngwrite.py holds against the model),
a round trip through pngDecode, a refused record between them, and the argument errors."""
import json
import os
import shutil
import subprocess

import pytest

import _png
import _pngwrite as W
import _pngwrite_poison  # noqa: F401
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_node_png_encode(gpu, z, oracle, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    g = W.geometry()
    ims = [W.nine()[0], g[28], W.rgba16(6), W.Img("refused record", 4, 3, 2, 8, 7, bytes(36)), W.each_wins(5)]
    py = W.run_host(z, ims)
    rows = []
    for k, (im, got) in enumerate(zip(ims, py)):
        (tmp_path / ("%d.bin" % k)).write_bytes(im.raw)
        row = dict(name="%d: %s" % (k, im.name), rows="%d.bin" % k,
                   image=dict(width=im.width, height=im.height, colourType=im.colour, depth=im.depth, filter=im.filter))
        if im.plte:
            (tmp_path / ("%d.plte" % k)).write_bytes(im.plte)
            row["palette"] = "%d.plte" % k
        if im.trns:
            (tmp_path / ("%d.trns" % k)).write_bytes(im.trns)
            row["transparency"] = "%d.trns" % k
        if isinstance(got, bytes):
            assert got == W.expect(im, oracle)[0], im.name
            (tmp_path / ("%d.png" % k)).write_bytes(got)
            row["png"] = "%d.png" % k
        else:
            assert got == _png.ZES_E_ARG
            row["message"] = z.strerror(got)
        rows.append(row)
    assert sum(1 for r in rows if "png" in r) == 4 and any("palette" in r for r in rows)
    (tmp_path / "expected.json").write_text(json.dumps(dict(images=rows)))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_pngwrite_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_PNGW_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "pngwrite node checks passed" in out.stdout
