"""The PNG writer's host side, without a GPU: the bound, every status that the arguments alone decide, the record's size and
the catalogue; and the expectation itself — the conditions that tests/_pngwrite.py's images were built for hold in the model,
and the files it expects are PNG files for the restated file rule, for CPython's zlib and for PIL."""
import io
import os
import re
import zlib

import numpy as np
import pytest

import _png
import _pngwrite as W
import _poison_cases as P
import _pngwrite_poison
from conftest import ROOT

ARG, UNS = _png.ZES_E_ARG, _png.ZES_E_UNSUPPORTED


def test_record_size_and_bound(z):
    assert z.PNGW_IMAGE.itemsize == 16 and z.PNGW_IMAGE.names == ("width", "height", "depth", "colour", "filter", "pad", "plte_len", "trns_len")
    ims = W.geometry() + [W.random_rgba(), W.lowent_rgba()] + W.refused()
    assert z.png_bound(W.records(z, ims)) == [W.bound(im) for im in ims]
    assert z.png_bound(np.zeros(0, dtype=z.PNGW_IMAGE)) == []
    # 1 x 1 grey: F = 2, stored 2 + 5 + 2 + 4 = 13 bytes in one IDAT
    assert z.png_bound(W.records(z, [(1, 1, 8, 0, 0, 0, 0, 0)])[:1]) == [8 + 25 + 12 + 13 + 12]
    # F = 65536: two stored blocks, 65552 stream bytes, two IDAT chunks
    assert z.png_bound(W.records(z, [(255, 256, 8, 0, 0, 0, 0, 0)])[:1]) == [8 + 25 + (2 + 10 + 65536 + 4) + 24 + 12]
    bad = W.bad_records()
    assert z.png_bound(W.records(z, [r for r, _, _ in bad])) == [0 if k != 6 else W.bound(W.Img("x", 4, 3, 0, 8, 0, bytes(12))) for k in range(len(bad))]
    lib = z.lib()
    rec = W.records(z, [(1, 1, 8, 0, 0, 0, 0, 0)])
    cap = np.zeros(1, dtype=np.uint64)
    assert lib.zes_pngwrite_bound(rec.ctypes.data, 1, None) == ARG and lib.zes_pngwrite_bound(None, 1, cap.ctypes.data) == ARG
    assert lib.zes_pngwrite_bound(None, 0, None) == 0


def test_statuses_from_the_arguments_alone(z):
    """Steps 1 and 2 and count == 0: answered by both forms without a device (the pointers are never followed)."""
    bad = W.bad_records()
    assert len(bad) == 18 and [s for _, _, s in bad].count(UNS) == 1
    for form in ("dev", "host"):
        aux = bytes(sum(r[6] + r[7] for r, _, _ in bad))
        rc, out_len, status = W.raw_call(z, [r for r, _, _ in bad], [n for _, n, _ in bad], form, aux=aux)
        assert rc == 0 and status == [s for _, _, s in bad] and out_len == [0] * len(bad), form
        for k, (r, n, s) in enumerate(bad):  # and one by one
            assert W.raw_call(z, [r], [n], form, aux=bytes(r[6] + r[7])) == (0, [0], [s]), (form, k)
        assert W.raw_call(z, [], [], form)[0] == 0
        assert W.raw_call(z, [], [], form, null=("img", "in_len", "in_off", "out_off", "out_cap", "out_len", "status", "aux", "d_in", "d_out", "in"))[0] == 0


def test_argument_errors_of_the_whole_call(z):
    good = (4, 3, 8, 0, 0, 0, 0, 0)
    pal = (4, 3, 8, 3, 0, 0, 6, 1)
    for name in ("img", "in_len", "in_off", "out_off", "out_cap", "out_len", "status", "d_in"):
        assert W.raw_call(z, [good], [12], "dev", null=(name,))[0] == ARG, name
    for name in ("img", "in_len", "out_len", "status", "in", "in0", "alloc"):
        assert W.raw_call(z, [good], [12], "host", null=(name,))[0] == ARG, name
    for form in ("dev", "host"):
        assert W.raw_call(z, [pal], [12], form, aux=bytes(7), null=("aux",))[0] == ARG
        for flags in (1, 2, 8, 16, 32, 64, 4 | 1, 0x80000000):
            assert W.raw_call(z, [good], [12], form, flags=flags)[0] == ARG, flags
        # a null d_in / in[i] is fine for an image of no bytes ... which no record describes: in_len 0 is a step-1 status
        assert W.raw_call(z, [good], [0], form, null=("d_in", "in0")) == (0, [0], [ARG])


def test_device_error_without_a_gpu(z):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_pngwrite.py runs these calls")
    good = (4, 3, 8, 0, 0, 0, 0, 0)
    for form in ("dev", "host"):
        assert W.raw_call(z, [good], [12], form)[0] == _png.ZES_E_DEVICE
        assert W.raw_call(z, [(0, 3, 8, 0, 0, 0, 0, 0), good], [0, 12], form)[0] == _png.ZES_E_DEVICE  # one image passes: a call for the device
    with pytest.raises(z.ZlibEsError) as e:
        z.png_encode(np.zeros((3, 4), dtype=np.uint8))
    assert e.value.code == _png.ZES_E_DEVICE


def test_the_model_meets_the_conditions_its_images_were_built_for(oracle):
    c5, c6 = W.choose(W.each_wins(5)), W.choose(W.each_wins(6))
    assert set(c6) == {0, 1, 2, 3, 4} and c6[64] in (2, 4) and c6[128] in (2, 4)
    assert c5[64] in (0, 1) and c5[128] in (0, 1) and c5[0] in (0, 1) and [a for r, a in enumerate(c5) if r % 64] == [a for r, a in enumerate(c6) if r % 64]
    assert set(W.choose(W.zeros(6))) == {0} == set(W.choose(W.zeros(5)))  # every type costs 0: the lowest number
    assert set(W.choose(W.grey4(5))) == {0} == set(W.choose(W.grey4(6))) and len(set(W.choose(W.rgba16(6)))) >= 2
    rnd, low = W.random_rgba(), W.lowent_rgba()
    assert W.expect(rnd, oracle)[1] == "stored" and W.idats(W.expect(rnd, oracle)[0]) == [65536, W.stored_len(rnd.F) - 65536]
    assert rnd.F == 73920 and len(W.expect(rnd, oracle)[0]) == W.bound(rnd)
    assert W.expect(low, oracle)[1] == "stream" and len(W.idats(W.expect(low, oracle)[0])) >= 3 and len(W.expect(low, oracle)[0]) < W.bound(low)
    assert [W.expect(im, oracle)[1] for im in W.refused()] == ["refused", "refused"] and [im.F for im in W.refused()] == [131073] * 2
    assert W.groups(W.nine()) == [9] and W.groups(W.nine(), W.PIECES) == [4, 4, 1]
    f = W.geometry_facts()
    assert f["pairs"] == set(_png.PAIRS) and f["filters"] == set(range(7)) and f["bpp"] == {1, 2, 3, 4, 6, 8}
    routes = {W.expect(im, oracle)[1] for im in W.geometry()}
    assert routes == {"stream", "stored"}


def test_the_expected_files_are_png_files(oracle):
    """The expectation, pinned: the restated file rule accepts every expected file, CPython's zlib inflates its IDATs to rows
    that the independent unfilter turns back into the image, and PIL loads it."""
    Image = pytest.importorskip("PIL.Image")
    ims = W.geometry()[::2] + [W.each_wins(5), W.rgba16(6), W.random_rgba()] + W.refused()[:1]
    for im in ims:
        blob = W.expect(im, oracle)[0]
        st, info = _png.info_rule(blob)
        assert st == 0 and (info["width"], info["height"], info["colour"], info["depth"]) == (im.width, im.height, im.colour, im.depth), im.name
        assert info["plte_len"] == len(im.plte) and info["trns_len"] == len(im.trns), im.name
        sizes = W.idats(blob)
        assert sizes and all(n == 65536 for n in sizes[:-1]) and 0 < sizes[-1] <= 65536, im.name
        assert [t for _, t, _, _ in _png.chunks_of(blob) if t not in (b"IDAT",)] == [b"IHDR"] + [b"PLTE"] * bool(im.plte) + [b"tRNS"] * bool(im.trns) + [b"IEND"]
        f = zlib.decompress(b"".join(blob[d:d + n] for _, t, d, n in _png.chunks_of(blob) if t == b"IDAT"))
        assert _png.unfilter(f, im.height, im.rowbytes, im.bpp) == im.raw, im.name
        with Image.open(io.BytesIO(blob)) as p:
            p.load()
            assert p.size == (im.width, im.height), im.name


def test_entry_points_are_exported_and_in_the_poison_catalogue(z, oracle):
    """What tests/test_zipwrite_cpu.py checks for the ZIP writer's three."""
    whole = open(os.path.join(ROOT, "include", "zes.h")).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    names = sorted(n for n in set(re.findall(r"^\s*int\s+(zes_[a-z0-9_]+)\s*\(", text, flags=re.M)) if n.startswith("zes_pngwrite"))
    assert names == ["zes_pngwrite", "zes_pngwrite_bound", "zes_pngwrite_dev"] == sorted(list(_pngwrite_poison.COVERS) + list(_pngwrite_poison.EXEMPT))
    for n in names:
        assert hasattr(z.lib(), n), n
        assert (n in P.COVERS) != (n in P.EXEMPT), n
    assert not any(n.startswith("zes_png_") for n in names)
    entries = list(P.catalogue(z, oracle).values())
    for fn, patterns in _pngwrite_poison.COVERS.items():
        for pat in patterns:
            assert any(fn in e.calls for e in P.covering(entries, pat)), (fn, pat)
    mine = [e for e in entries if any(fn in _pngwrite_poison.COVERS for fn in e.calls)]
    again = {e.name: e for e in _pngwrite_poison.entries(z, oracle)}
    assert len(mine) == 4 and sorted(again) == sorted(e.name for e in mine)
    for e in mine:
        assert e.source == "oracle" and all(c.startswith("zes_pngwrite") for c in e.calls), e.name
        assert e.want() == again[e.name].want() and e.want()[0] == "out" and e.want()[1] > 2000, e.name
    assert "no writer" not in whole
