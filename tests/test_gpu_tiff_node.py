"""tiffInfo() and tiffRead() of the N-API façade under Node (tests/host_node_tiff_test.js) on files that tests/_tiff.py writes
into a temporary directory: whole images of several kinds, rectangles, the second directory of a file, a damaged tile, files
the rule refuses and a file that is no TIFF at all — with the records and pixels of the helper's restatement and independent
reader, and the library's messages, as the expected values."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _tiff as T
import _tiff_poison  # noqa: F401
from conftest import ROOT

pytestmark = pytest.mark.gpu

JS_NAMES = dict(width="width", height="height", seg_w="segmentWidth", seg_h="segmentHeight", across="across", down="down", bits="bits", spp="samples",
                compression="compression", predictor="predictor", photometric="photometric", sample_format="sampleFormat", extra_samples="extraSamples",
                big_endian="bigEndian", tiled="tiled", out_size="size")


def js_info(rec, dirs):
    d = {JS_NAMES[k]: (bool(v) if k in ("big_endian", "tiled") else v) for k, v in rec.items()}
    d["dirs"] = dirs
    return d


def test_node_tiff(gpu, z, oracle, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    items = []

    def image(name, f, dir=None, rect=None):
        k = len(items)
        (tmp_path / ("%d.tif" % k)).write_bytes(f)
        rec, _, _, dirs = T.rule(f, dir or 0)
        px = T.decode(f, dir or 0, rect)
        (tmp_path / ("%d.pix" % k)).write_bytes(px.tobytes())
        options = {}
        if dir is not None:
            options["dir"] = dir
        if rect is not None:
            options["rect"] = dict(zip("xywh", rect))
        row = dict(name=name, file="%d.tif" % k, options=options or None, info=js_info(rec, dirs), pixels="%d.pix" % k,
                   shape=[px.shape[1], px.shape[0], rec["spp"], rec["bits"]])
        if dir is not None:
            row["dir"] = dir
        items.append(row)

    def refusal(name, f, status, dir=None, info=False):
        k = len(items)
        (tmp_path / ("%d.tif" % k)).write_bytes(f)
        row = dict(name=name, file="%d.tif" % k, options=None if dir is None else dict(dir=dir), message=z.strerror(status))
        if dir is not None:
            row["dir"] = dir
        if info:
            rec, _, _, dirs = T.rule(f, dir or 0)
            row["info"] = js_info(rec, dirs)
        items.append(row)

    kinds = [dict(spp=3, bits=8, layout=("tiles", 16, 16), order="II", compression=8, predictor=2),
             dict(spp=1, bits=16, layout=("strips", 5), order="MM", compression=32946, predictor=2),
             dict(spp=4, bits=32, layout=("tiles", 32, 16), order="MM", compression=1, predictor=1)]
    for kw in kinds:
        f, _ = T.make(w=37, h=23, **kw)
        image("whole image %s" % (kw,), f)
        image("a rectangle %s" % (kw,), f, rect=(27, 9, 8, 11))
    two, _ = T.two_directories()
    image("the second directory", two, dir=1)
    image("the second directory, a rectangle", two, dir=1, rect=(2, 9, 17, 21))
    for name, f, px, bad, want in T.segment_damage(oracle):
        if name in ("a wrong Adler-32", "one row too long", "an uncompressed segment too short"):
            refusal("a damaged tile: " + name, f, want, info=True)
    refusal("not a TIFF file", b"\x89PNG\r\n\x1a\n" + bytes(100), T.E_TIFF)
    refusal("LZW", [f for n, f, d, s, _ in T.index_damage() if n == "LZW"][0], T.E_UNSUPPORTED)
    refusal("dir 2 of two", two, T.E_ARG, dir=2)
    assert sum(1 for r in items if "message" in r) == 6 and len(items) == 14
    (tmp_path / "expected.json").write_text(json.dumps(dict(items=items, arg=z.strerror(T.E_ARG))))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_tiff_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_TIFF_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "tiff node checks passed" in out.stdout
