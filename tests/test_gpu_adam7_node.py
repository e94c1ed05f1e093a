"""The `{ interlaced }` option of the N-API façade's PNG readers under Node (tests/host_node_adam7_test.js): interlaced files
of tests/_adam7.py between plain ones of tests/_png.py, scanlines and pixels, with and without the option."""
import json
import os
import shutil
import subprocess

import pytest

import _adam7
import _png
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_node_adam7(gpu, z, tmp_path):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    inter = _adam7.pairs()[::2] + _adam7.small_grid()[::23]
    plain = _png.geometry()[::9]
    cases = []
    for k, c in enumerate(inter):
        cases.append((c, True))
        if k % 4 == 0:
            cases.append((plain[(k // 4) % len(plain)], False))
    # the pixels by the path that has tests of its own: the same scanlines in a non-interlaced file
    pixels = z.png_pixels_batch([(_adam7.plain_of(c) if il else c).blob for c, il in cases])
    files = []
    for k, ((c, il), px) in enumerate(zip(cases, pixels)):
        assert not isinstance(px, Exception), c.name
        (tmp_path / ("%d.png" % k)).write_bytes(c.blob)
        (tmp_path / ("%d.rows" % k)).write_bytes(c.want)
        (tmp_path / ("%d.rgba" % k)).write_bytes(px[1].tobytes())
        files.append(dict(name="%d: %s" % (k, c.name), file="%d.png" % k, interlaced=il, rows="%d.rows" % k, pixels="%d.rgba" % k))
    (tmp_path / "expected.json").write_text(json.dumps(dict(files=files, unsupported=z.strerror(_png.ZES_E_UNSUPPORTED))))
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_adam7_test.js")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ZES_ADAM7_DIR=str(tmp_path)))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "adam7 node checks passed" in out.stdout
