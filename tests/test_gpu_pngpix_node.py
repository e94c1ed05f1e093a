"""pngPixels() and pngPixelsBatch() of the N-API façade under Node (tests/host_node_pngpix_test.js): a part of the case table
of tests/_pngpix.py that spans the pairs and the kinds, and the reader's damage table between good neighbours, in one batch —
the pixels computed here by the numpy rule and written to temporary files, an Error in the place of every damaged file."""
import json
import os
import shutil
import subprocess

import pytest

import _png
import _pngpix as X
from conftest import ROOT

pytestmark = pytest.mark.gpu

JS_NAMES = dict(width="width", height="height", depth="depth", colour="colourType", interlace="interlace", channels="channels", bpp="bpp",
                rowbytes="rowBytes", out_size="size", idat_count="idatCount", idat_bytes="idatBytes", plte_pos="paletteOffset", plte_len="paletteLength",
                trns_pos="transparencyOffset", trns_len="transparencyLength")


def test_node_png_pixels(gpu, z, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    rows = X.damaged() + [(c.name, c.blob, 0, c.want) for c in X.subset()]
    files = []
    for k, (name, blob, status, want) in enumerate(rows):
        (tmp_path / ("%d.png" % k)).write_bytes(blob)
        row = dict(name="%d: %s" % (k, name), file="%d.png" % k, k=k)
        if status == 0:
            (tmp_path / ("%d.rgba" % k)).write_bytes(want.tobytes())
            row["pixels"] = "%d.rgba" % k
            row["info"] = {JS_NAMES[f]: v for f, v in _png.info_rule(blob)[1].items() if f in JS_NAMES}
        else:
            row["messages"] = [z.strerror(s) for s in (status if isinstance(status, tuple) else (status,))]
        files.append(row)
    (tmp_path / "expected.json").write_text(json.dumps(dict(files=files)))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_pngpix_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_PNGPIX_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "pngpix node checks passed" in out.stdout
