"""The PNG pixel forms' host side, without a GPU: the case table's coverage, the numpy rule of tests/_pngpix.py against Pillow
where the two agree, what zes_pngpix_dev / zes_pngpix_alloc / zes_pngpix_expand_dev answer before they touch a device, and
the poison-catalogue facts for the three entry points."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import _png
import _pngpix as X
import _pngpix_poison
import _pngwrite as W
import _poison_cases as P
from conftest import ROOT

ARG, UNS, DEVICE = _png.ZES_E_ARG, _png.ZES_E_UNSUPPORTED, _png.ZES_E_DEVICE


def test_case_table_covers_what_it_is_for():
    f = X.facts()
    assert f["pairs"] == set(_png.PAIRS) and len(f["pairs"]) == 15
    assert f["widths"] >= set(X.WIDTHS) and f["heights"] == set(X.HEIGHTS)
    assert f["pair_heights"] == {(c, d, h) for c, d in _png.PAIRS for h in X.HEIGHTS}
    assert f["kinds"] == {"plain", "trns", "trns high byte only", "trns small key", "trns scaled key", "short palette", "short palette short trns",
                          "unfitting trns"}
    assert f["keyed"] == {(c, d) for c, d in _png.PAIRS if c in (0, 2)}  # every key of the "trns" kind does match a pixel
    assert 300 <= f["count"] <= 340
    by = {}
    for c in X.cases():
        by.setdefault(c.kind, []).append(c)
    for c in by["trns high byte only"]:  # the key's high bytes are a pixel's, and nothing matches
        assert c.depth == 16 and (c.want[..., 3] == 255).all()
        key = np.frombuffer(c.trns, dtype=">u2") >> 8
        assert ((X.samples(c.raw, c.width, c.height, c.colour, 16) >> 8) == key).all(axis=2).any()
    for c in by["trns small key"]:
        assert (c.want[..., 3] == 0).any() and (c.want[..., 3] == 255).any()
    for c in by["trns scaled key"]:
        assert (c.want[..., 3] == 255).all() and (c.want[..., 0] == X.SCALE[c.depth]).any()
    for c in by["short palette"] + by["short palette short trns"]:
        beyond = X.samples(c.raw, c.width, c.height, 3, c.depth)[..., 0] >= len(c.plte) // 3
        assert beyond.any() and (c.want[beyond] == (0, 0, 0, 255)).all()
    for c in by["unfitting trns"]:
        assert not c.fits and (c.want == X.rule(c.raw, c.width, c.height, c.colour, c.depth, c.plte)).all()
    assert all(c.fits for c in X.cases() if c.kind != "unfitting trns")
    assert {(c.colour, c.depth) for c in X.subset()} == set(_png.PAIRS) and {c.kind for c in X.subset()} == f["kinds"]


def test_rule_by_hand():
    """The rule on bytes small enough to read: one row a pair."""
    r = lambda raw, w, colour, depth, plte=b"", trns=b"": X.rule(bytes(raw), w, 1, colour, depth, plte, trns).reshape(-1, 4).tolist()
    assert r([0b10100000], 3, 0, 1) == [[255, 255, 255, 255], [0, 0, 0, 255], [255, 255, 255, 255]]
    assert r([0b00011011], 4, 0, 2, trns=b"\0\2") == [[0, 0, 0, 255], [85, 85, 85, 255], [170, 170, 170, 0], [255, 255, 255, 255]]
    assert r([0x1F], 2, 0, 4, trns=b"\0\x11") == [[17, 17, 17, 255], [255, 255, 255, 255]]  # 0x11 is no 4-bit sample
    assert r([0x12, 0x34, 0x12, 0x35], 2, 0, 16, trns=b"\x12\x35") == [[0x12, 0x12, 0x12, 255], [0x12, 0x12, 0x12, 0]]
    assert r([1, 2, 3, 1, 2, 4], 2, 2, 8, trns=b"\0\1\0\2\0\4") == [[1, 2, 3, 255], [1, 2, 4, 0]]
    assert r([1, 2, 3, 1, 2, 4], 2, 2, 8, trns=b"\0\1\0\2") == [[1, 2, 3, 255], [1, 2, 4, 255]]  # four bytes: not a tRNS for RGB
    assert r([0x21], 2, 3, 4, plte=bytes(range(9)), trns=b"\x07\x08") == [[6, 7, 8, 255], [3, 4, 5, 8]]
    assert r([0x30], 2, 3, 4, plte=bytes(range(9))) == [[0, 0, 0, 255], [0, 1, 2, 255]]  # index 3 of a palette of 3
    assert r([9, 200], 1, 4, 8) == [[9, 9, 9, 200]]
    assert r([1, 2, 3, 4, 5, 6, 7, 8], 1, 6, 16) == [[1, 3, 5, 7]]


def test_rule_equals_pillow_where_they_agree():
    Image = pytest.importorskip("PIL.Image")
    seen = set()
    for c in X.cases():
        combo = (c.colour, c.depth, bool(c.trns))
        if c.kind not in ("plain", "trns") or combo not in X.PIL_AGREES:
            continue
        got = np.asarray(Image.open(io.BytesIO(c.blob)).convert("RGBA"))
        assert got.shape == c.want.shape and (got == c.want).all(), c.name
        seen.add(combo)
    assert seen == X.PIL_AGREES and len(seen) >= 19


def raw_alloc(z, blobs, count=None, alloc=True, out_len=True, status=True, lens=True, flags=0):
    calls = []

    def cb(_user, i, n):
        calls.append((i, n))
        return None

    arrs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
    cnt = len(arrs) if count is None else count
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data if a.size else None for a in arrs])
    ln = np.array([a.size for a in arrs] + [0], dtype=np.uint64)
    ol = np.zeros(max(cnt, 1), dtype=np.uint64)
    st = np.full(max(cnt, 1), 99, dtype=np.int32)
    rc = z.lib().zes_pngpix_alloc(ptrs, ln.ctypes.data if lens else None, cnt, z.ALLOC_FN(cb) if alloc else C.cast(None, z.ALLOC_FN), None,
                                  ol.ctypes.data if out_len else None, st.ctypes.data if status else None, None, flags)
    return rc, [int(x) for x in st[:cnt]], calls


def raw_dev(z, n, null=(), flags=0, d_in=0x1000):
    """zes_pngpix_dev with pointers that are never followed (only for calls that end before the device)."""
    arr = {k: np.zeros(n + 1, dtype=np.uint64) for k in ("in_off", "in_len", "out_off", "out_cap", "out_len")}
    arr["in_len"][:n] = 100
    st = np.full(n + 1, 99, dtype=np.int32)
    p = lambda k: None if k in null else arr[k].ctypes.data
    return z.lib().zes_pngpix_dev(None if "d_in" in null else d_in, p("in_off"), p("in_len"), n, 0x2000, p("out_off"), p("out_cap"), p("out_len"),
                                  None if "status" in null else st.ctypes.data, None, flags)


def test_file_forms_before_the_device(z):
    import torch

    good = X.cases()[0].blob
    bad = [c.blob for c in _png.damage()[:7]]  # what the rule (and the interlace test) rejects on the host
    for flags in (1, 8, 16, 32, 4 | 64):
        assert raw_alloc(z, [good], flags=flags)[0] == ARG
        assert raw_dev(z, 1, flags=flags) == ARG
    assert raw_alloc(z, [good], alloc=False)[0] == ARG
    assert raw_alloc(z, [good], out_len=False)[0] == ARG
    assert raw_alloc(z, [good], status=False)[0] == ARG
    assert raw_alloc(z, [good], lens=False)[0] == ARG
    for name in ("in_off", "in_len", "out_off", "out_cap", "out_len", "status", "d_in"):
        assert raw_dev(z, 1, null=(name,)) == ARG, name
    assert raw_alloc(z, [good], count=0) == (0, [], [])  # nothing to do: ZES_OK, no device
    assert raw_alloc(z, [], flags=4) == (0, [], [])
    assert raw_dev(z, 0) == 0 and raw_dev(z, 0, null=("in_off", "in_len", "out_off", "out_cap", "out_len", "status", "d_in")) == 0
    assert z.png_pixels_batch([]) == []
    # a batch in which no file passes the rule is answered on the host
    rc, st, calls = raw_alloc(z, bad)
    assert (rc, calls) == (0, []) and st == [-24, -24, -24, -24, -24, -23, -23]
    assert [r.code for r in z.png_pixels_batch(bad)] == st
    with pytest.raises(z.ZlibEsError) as e:
        z.png_pixels(bad[0])
    assert e.value.code == _png.ZES_E_PNG
    if not torch.cuda.is_available():  # anything else needs the device
        assert raw_alloc(z, [good])[0] == DEVICE
        assert raw_alloc(z, bad + [good])[0] == DEVICE


def raw_expand(z, recs, lens, aux=b"", flags=0, count=None, null=(), cap=1 << 40):
    """zes_pngpix_expand_dev with arguments as they are (pointers are never followed when no image passes the checks) ->
    (rc, out_len, status)."""
    n = len(recs) if count is None else count
    rec = W.records(z, recs)
    ln = np.array(list(lens) + [0], dtype=np.uint64)
    zero = np.zeros(n + 1, dtype=np.uint64)
    caps = np.full(n + 1, cap, dtype=np.uint64)
    out_len = np.full(n + 1, 77, dtype=np.uint64)
    status = np.full(n + 1, 77, dtype=np.int32)
    a = np.frombuffer(bytes(aux) + b"\0", dtype=np.uint8)
    p = lambda name, arr: None if name in null else arr.ctypes.data
    rc = z.lib().zes_pngpix_expand_dev(None if "d_in" in null else 0x1000, p("in_off", zero), p("in_len", ln), p("img", rec), p("aux", a), n,
                                       None if "d_out" in null else 0x2000, p("out_off", zero), p("out_cap", caps), p("out_len", out_len), p("status", status),
                                       flags)
    return rc, [int(x) for x in out_len[:n]], [int(x) for x in status[:n]]


def test_expand_before_the_device(z):
    import torch

    table = W.bad_records()
    ignored = [(r, n, s) for r, n, s in table if r[4] > 6]  # the filter field says nothing here: no status from it
    bad = [(r, n, s) for r, n, s in table if r[4] <= 6]
    assert len(ignored) == 1 and len(bad) == 17 and [s for _, _, s in bad].count(UNS) == 1
    aux = bytes(sum(r[6] + r[7] for r, _, _ in bad))
    rc, out_len, status = raw_expand(z, [r for r, _, _ in bad], [n for _, n, _ in bad], aux=aux)
    assert rc == 0 and status == [s for _, _, s in bad] and out_len == [0] * len(bad)
    for k, (r, n, s) in enumerate(bad):  # and one by one
        assert raw_expand(z, [r], [n], aux=bytes(r[6] + r[7])) == (0, [0], [s]), k
    # count == 0, and a batch with nothing to write: ZES_OK, no device
    assert raw_expand(z, [], [])[0] == 0
    assert raw_expand(z, [], [], null=("img", "in_len", "in_off", "out_off", "out_cap", "out_len", "status", "aux", "d_in", "d_out"))[0] == 0
    good, pal = (4, 3, 8, 0, 0, 0, 0, 0), (4, 3, 8, 3, 0, 0, 6, 1)
    assert raw_expand(z, [good, pal], [12, 12], aux=bytes(7), cap=47) == (0, [48, 48], [-16, -16])  # no room: the size needed
    assert raw_expand(z, [good], [12], null=("d_out",)) == (0, [48], [-16])
    assert raw_expand(z, [(5, 3, 1, 0, 0, 0, 0, 0)], [3], cap=59) == (0, [60], [-16])
    # the whole call
    for name in ("img", "in_len", "in_off", "out_off", "out_cap", "out_len", "status", "d_in"):
        assert raw_expand(z, [good], [12], null=(name,))[0] == ARG, name
    assert raw_expand(z, [pal], [12], aux=bytes(7), null=("aux",))[0] == ARG
    for flags in (1, 2, 8, 16, 32, 64, 4 | 1, 0x80000000):
        assert raw_expand(z, [good], [12], flags=flags)[0] == ARG, flags
    assert raw_expand(z, [good], [0], null=("d_in",)) == (0, [0], [ARG])
    if not torch.cuda.is_available():  # an image that passes is a call for the device
        assert raw_expand(z, [good], [12])[0] == DEVICE
        assert raw_expand(z, [bad[0][0], good], [bad[0][1], 12])[0] == DEVICE
        assert raw_expand(z, [ignored[0][0]], [ignored[0][1]])[0] == DEVICE  # filter 7: not this call's business
        assert raw_expand(z, [good], [12], flags=4)[0] == DEVICE  # ZES_F_PIECES is let through


def test_entry_points_are_exported_and_in_the_poison_catalogue(z, oracle):
    """What tests/test_poison_cpu.py asks of every entry point, for the pixel forms: declared, exported, covered by catalogue
    entries that make the call; and the entries' expected values come out the same from the builders run again."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zes.h")).read(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"^\s*int\s+(zes_[a-z0-9_]+)\s*\(", text, flags=re.M)) if n.startswith("zes_pngpix"))
    assert names == sorted(_pngpix_poison.COVERS) == ["zes_pngpix_alloc", "zes_pngpix_dev", "zes_pngpix_expand_dev"]
    for n in names:
        assert hasattr(z.lib(), n) and n in P.COVERS and n not in P.EXEMPT, n
    entries = list(P.catalogue(z, oracle).values())
    for fn, patterns in _pngpix_poison.COVERS.items():
        for pat in patterns:
            assert any(fn in e.calls for e in P.covering(entries, pat)), (fn, pat)
    mine = [e for e in entries if any(fn in _pngpix_poison.COVERS for fn in e.calls)]
    again = {e.name: e for e in _pngpix_poison.entries(z, oracle)}
    assert len(mine) == 6 and sorted(again) == sorted(e.name for e in mine)
    for e in mine:
        assert e.source == "zlib" and e.want() == again[e.name].want() and len(e.want()) >= 11, e.name
    assert any(w[0] == "err" for e in mine for w in e.want()) and sum(w[0] == "out" for e in mine for w in e.want()) >= 100
