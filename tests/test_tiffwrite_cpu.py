"""The TIFF writer's host side, without a GPU: the expectation itself — every file tests/_tiffwrite.py expects passes the
restated file rule with the record it was made from, the independent reader and PIL give its pixels back — the bound, every
status that the arguments alone decide, the routes the GPU tests' cases take, the bindings, the header and the catalogue."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import _poison_cases as P
import _tiff as T
import _tiffwrite as W
import _tiffwrite_poison
from conftest import ROOT

ARG, UNS = T.E_ARG, T.E_UNSUPPORTED


def all_cases():
    return list(W.grid()) + W.gpu_cases()


def test_the_expected_files_pass_the_rule_with_their_record_and_decode_to_the_pixels(oracle):
    names = set()
    for case in all_cases():
        f, routes = W.expect(case, oracle)
        rec, off, ln, dirs = T.rule(f)
        assert rec == case.record() and dirs == 1, case.name
        assert len(routes) == len(off) == rec["across"] * rec["down"], case.name
        assert all(o % 2 == 0 and o >= 8 for o in off) and off == sorted(off), case.name
        got = T.decode(f)
        assert got.dtype == case.px.dtype and got.shape == case.px.shape and (got.view(np.uint8) == case.px.view(np.uint8)).all(), case.name
        assert len(f) <= W.bound(rec), case.name
        if set(routes) <= {"stored", "refused", "none"}:
            assert len(f) == W.bound(rec), case.name  # the bound is exact when every segment goes stored
        names.add(case.name)
    assert len(names) == len(all_cases())  # (expect() keeps its files by name)


def test_pil_reads_the_expected_files_to_the_same_pixels(oracle):
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for case in W.grid():
        rec = case.record()
        if not ((rec["bits"] == 8 and rec["spp"] in (1, 3, 4)) or (rec["bits"] == 16 and rec["spp"] == 1)):
            continue
        im = Image.open(io.BytesIO(W.expect(case, oracle)[0]))
        got = np.asarray(im)
        got = got.reshape(got.shape[0], got.shape[1], -1)
        assert got.shape == case.px.shape and (got.astype(np.uint32) == case.px).all(), (case.name, im.mode)
        n += 1
    assert n == 4 * len(T.LAYOUTS) * 2 * len(W.CODINGS)


def test_bound_equals_the_restated_bound_on_every_case(z):
    for case in all_cases():
        rec = case.record()
        assert W.bound_call(z, rec) == (0, W.bound(rec), rec["across"] * rec["down"]), case.name
        assert z.tiff_bound(rec) == (W.bound(rec), rec["across"] * rec["down"]), case.name
    # 1 x 1 grey, Compression 8: 2 + 5 + 1 + 4 stored bytes = 12, no arrays, ten entries
    one = W.refused()[0].record()
    assert W.bound_call(z, one) == (0, 8 + 12 + 2 + 12 * 10 + 4, 1)
    lib = z.lib()
    img = W.record_array(z, one)
    cap = C.c_uint64()
    assert lib.zes_tiffwrite_bound(img.ctypes.data, C.byref(cap), None) == 0 and cap.value == 146  # (segments may be null)
    assert lib.zes_tiffwrite_bound(None, C.byref(cap), None) == ARG and lib.zes_tiffwrite_bound(img.ctypes.data, None, None) == ARG


def test_every_status_line_is_reached_by_one_record(z):
    bad = W.bad_records()
    assert [s for _, _, _, s in bad].count(UNS) == 5 and len(bad) == 33
    for name, rec, n, status in bad:
        for form in ("dev", "host"):
            assert W.raw_call(z, rec, n, form) == (status, 0), (name, form)
        if n is None:
            assert W.bound_call(z, rec) == (status, 0, 0), name
    good = bad[4][1]
    assert W.bound_call(z, good)[0] == 0
    # the whole call's argument errors
    for form, nulls in (("dev", ("img", "out_len", "in")), ("host", ("img", "out_len", "in", "alloc"))):
        for null in nulls:
            assert W.raw_call(z, good, form=form, null=(null,))[0] == ARG, (form, null)
        for flags in (1, 2, 8, 16, 32, 64, 4 | 1, 0x80000000):
            assert W.raw_call(z, good, form=form, flags=flags)[0] == ARG, (form, flags)
    # ZES_E_ARG comes first: an unsupported record with a wrong n
    uns = bad[28][1]
    assert bad[28][3] == UNS and W.raw_call(z, uns, uns["out_size"] + 1)[0] == ARG


def test_device_error_without_a_gpu(z):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_tiffwrite.py runs these calls")
    good = W.six_tiles().record()
    for form in ("dev", "host"):
        assert W.raw_call(z, good, form=form)[0] == T.E_DEVICE
    with pytest.raises(z.ZlibEsError) as e:
        z.tiff_write(W.six_tiles().px, good)
    assert e.value.code == T.E_DEVICE


def test_the_gpu_tests_cases_take_all_three_routes(oracle):
    """What tests/test_gpu_tiffwrite.py relies on, asserted from the oracle: not assumed."""
    routes = lambda case: W.expect(case, oracle)[1]
    seen = set()
    for case in W.grid():
        r = set(routes(case))
        assert r == {"none"} if case.compression == 1 else r <= {"stream", "stored"}, case.name
        seen |= r
    assert seen == {"none", "stream", "stored"}
    assert [routes(c) for c in W.refused()] == [["refused"], ["refused"]]
    assert [len(c.segments()[0]) for c in W.refused()] == [1, 131073]
    mixed = routes(W.mixed())
    assert len(mixed) == 12 and "stream" in mixed and "stored" in mixed and set(mixed) == {"stream", "stored"}
    assert [mixed[k] for k in range(12)] == ["stored" if k % 2 == 0 else "stream" for k in range(12)]
    assert set(routes(W.rgba_tiles(32))) == {"stored"}  # noise: the launch-list images go stored throughout
    rec = W.six_tiles().record()
    assert W.groups(rec) == [6] and W.groups(rec, W.PIECES) == [4, 2]
    assert W.groups(W.many_strips().record()) == [1024, 1]


def test_the_python_record_builder(z):
    for case in all_cases():
        rec = case.record()
        lay = dict(tile=case.layout[1:]) if rec["tiled"] else dict(rows=case.layout[1])
        got = z.tiff_image(rec["width"], rec["height"], rec["bits"], rec["spp"], compression=rec["compression"], predictor=rec["predictor"],
                           sample_format=rec["sample_format"], big_endian=rec["big_endian"], **lay)
        assert got == rec, case.name
    assert z.tiff_image(5, 7)["seg_h"] == 7 and z.tiff_image(5, 7, rows=100)["seg_h"] == 7 and z.tiff_image(5, 7, photometric=0)["photometric"] == 0
    with pytest.raises(z.ZlibEsError) as e:
        z.tiff_bound(z.tiff_image(5, 7, tile=(24, 16)))
    assert e.value.code == ARG
    with pytest.raises(z.ZlibEsError) as e:
        z.tiff_bound(z.tiff_image(5, 7, compression=1, predictor=2))
    assert e.value.code == UNS


def test_entry_points_are_exported_and_in_the_poison_catalogue(z, oracle):
    """What tests/test_pngwrite_cpu.py checks for the PNG writer's three."""
    whole = open(os.path.join(ROOT, "include", "zes.h")).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    names = sorted(n for n in set(re.findall(r"^\s*int\s+(zes_[a-z0-9_]+)\s*\(", text, flags=re.M)) if n.startswith("zes_tiffwrite"))
    assert names == ["zes_tiffwrite", "zes_tiffwrite_bound", "zes_tiffwrite_dev"] == sorted(list(_tiffwrite_poison.COVERS) + list(_tiffwrite_poison.EXEMPT))
    for n in names:
        assert hasattr(z.lib(), n), n
        assert (n in P.COVERS) != (n in P.EXEMPT), n
    entries = list(P.catalogue(z, oracle).values())
    for fn, patterns in _tiffwrite_poison.COVERS.items():
        for pat in patterns:
            assert any(fn in e.calls for e in P.covering(entries, pat)), (fn, pat)
    mine = [e for e in entries if any(fn in _tiffwrite_poison.COVERS for fn in e.calls)]
    again = {e.name: e for e in _tiffwrite_poison.entries(z, oracle)}
    assert len(mine) == 8 and sorted(again) == sorted(e.name for e in mine)
    for e in mine:
        assert e.source == "oracle" and all(c.startswith("zes_tiffwrite") for c in e.calls), e.name
        assert e.want() == again[e.name].want() and e.want()[0] == "out" and e.want()[1] > 500, e.name
    assert "no TIFF writer" not in whole and "zes_tiffwrite_dev" in whole
