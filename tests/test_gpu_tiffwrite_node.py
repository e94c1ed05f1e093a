"""tiffWrite() of the N-API façade under Node (tests/host_node_tiffwrite_test.js) on images of tests/_tiffwrite.py's tables: the
bytes must equal the Python form's — which tests/test_gpu_tiffwrite.py holds against the restated layout, and which is held
against it here once more — and tiffInfo / tiffRead of them must give the record and the pixels back."""
import json
import os
import shutil
import subprocess

import pytest

import _tiff as T
import _tiffwrite as W
import _tiffwrite_poison  # noqa: F401
from conftest import ROOT
from test_gpu_tiff_node import js_info

pytestmark = pytest.mark.gpu


def test_node_tiffwrite(gpu, z, oracle, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    cases = [W.six_tiles(), W.mixed(), W.kinds()[0], W.kinds()[1], W.refused()[0], W.shapes()[4],
             next(iter(W.grid(layouts=(("strips", 5),), depths=(32,), samples=(4,), orders=("MM",), codings=((1, 1),))))]
    items = []
    for k, case in enumerate(cases):
        f = z.tiff_write(case.px, case.record())
        assert f == W.expect(case, oracle)[0], case.name
        (tmp_path / ("%d.pix" % k)).write_bytes(case.raw().tobytes())
        (tmp_path / ("%d.tif" % k)).write_bytes(f)
        items.append(dict(name=case.name, pixels="%d.pix" % k, file="%d.tif" % k, info=js_info(case.record(), 1)))
    (tmp_path / "expected.json").write_text(json.dumps(dict(items=items, arg=z.strerror(T.E_ARG), unsupported=z.strerror(T.E_UNSUPPORTED))))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_tiffwrite_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_TIFFW_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "tiffwrite node checks passed: %d images" % len(cases) in out.stdout
