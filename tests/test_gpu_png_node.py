"""pngInfo(), pngDecode() and pngDecodeBatch() of the N-API façade under Node (tests/host_node_png_test.js): the geometry
table and the damage table of tests/_png.py in one batch, with an Error in the place of every file that does not check out."""
import json
import os
import shutil
import subprocess

import pytest

import _png
from conftest import ROOT

pytestmark = pytest.mark.gpu

JS_NAMES = dict(width="width", height="height", depth="depth", colour="colourType", interlace="interlace", channels="channels", bpp="bpp",
                rowbytes="rowBytes", out_size="size", idat_count="idatCount", idat_bytes="idatBytes", plte_pos="paletteOffset", plte_len="paletteLength",
                trns_pos="transparencyOffset", trns_len="transparencyLength")


def test_node_png_decode(gpu, z, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    good = _png.geometry()
    cases = []
    for k, c in enumerate(c for c in _png.damage() if not c.short):
        cases += [good[2 * k], c, good[2 * k + 1]]
    cases += good[30:]
    files = []
    for k, c in enumerate(cases):
        (tmp_path / ("%d.png" % k)).write_bytes(c.blob)
        st, info = _png.info_rule(c.blob)
        row = dict(name="%d: %s" % (k, c.name), file="%d.png" % k)
        if st == 0:
            row["info"] = {JS_NAMES[f]: v for f, v in info.items() if f in JS_NAMES}
        else:
            row["infoMessage"] = z.strerror(st)
        if c.status == 0:
            (tmp_path / ("%d.bin" % k)).write_bytes(c.want)
            row["plain"] = "%d.bin" % k
        else:
            row["messages"] = [z.strerror(s) for s in (c.status if isinstance(c.status, tuple) else (c.status,))]
        files.append(row)
    (tmp_path / "expected.json").write_text(json.dumps(dict(files=files)))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_png_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_PNG_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "png node checks passed" in out.stdout
