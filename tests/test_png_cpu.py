"""The PNG reader's host side, without a GPU: zes_png_info_get against the restated rule (tests/_png.py) on every file of the
case tables, the helper's own soundness (its unfilter inverts its filter; PIL reads its files), the argument errors, what
zes_png_decode_alloc answers before it touches a device, and the poison-catalogue facts for the PNG entry points."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import _png
import _poison_cases as P
import _png_poison
from conftest import ROOT


def info_status(z, b):
    try:
        return 0, z.png_info(b)
    except z.ZlibEsError as e:
        return e.code, None


def test_case_tables_cover_what_they_are_for():
    f = _png.geometry_facts()
    assert f["pairs"] == set(_png.PAIRS) and len(_png.PAIRS) == 15
    assert f["widths"] == set(_png.WIDTHS) and f["heights"] == set(_png.HEIGHTS)
    assert f["bpp"] == {1, 2, 3, 4, 6, 8} and f["residues"] == {0, 1, 2, 3}
    assert f["row0"] == {0, 1, 2, 3, 4} and f["ordered"] == {(a, b) for a in range(5) for b in range(5)}
    assert 38 <= f["count"] <= 45
    names = [c.name for c in _png.everything()]
    assert len(set(names)) == len(names)
    assert [c.name for c in _png.damage()] == [
        "bad signature", "no IEND", "bytes behind IEND", "split IDAT run", "colour type 3 without PLTE", "unknown critical chunk", "interlaced",
        "flipped CRC of IHDR", "flipped CRC of an IDAT", "flipped CRC of an ancillary chunk", "flipped Adler-32", "stream cut short", "one row too many",
        "one row too few", "filter byte 5", "out_cap one byte short"]
    assert [c.status for c in _png.damage()] == [-24, -24, -24, -24, -24, -23, -23, -21, -21, -21, -21, (-1, -2, -3, -4, -5, -21), -24, -24, -24, 0]


def test_info_equals_the_rule_on_every_file(z):
    seen = set()
    for c in _png.everything():
        st, want = _png.info_rule(c.blob)
        assert st == c.info_status, (c.name, st, c.info_status)
        got_st, rec = info_status(z, c.blob)
        assert got_st == st, (c.name, got_st, st)
        seen.add(st)
        if st == 0:
            assert _png.info_dict(rec) == want and not np.asarray(rec["pad"]).any(), c.name
    assert seen == {0, _png.ZES_E_PNG, _png.ZES_E_UNSUPPORTED}
    # what some cases are there for
    rule = {c.name: c for c in _png.rule_only()}
    assert int(z.png_info(rule["tRNS noted, second one ignored"].blob)["trns_len"]) == 2
    assert int(z.png_info(rule["tRNS behind IDAT not noted"].blob)["trns_pos"]) == 0
    assert int(z.png_info(rule["PLTE in a truecolour file"].blob)["plte_len"]) == 9
    assert int(z.png_info({c.name: c for c in _png.damage()}["interlaced"].blob)["interlace"]) == 1
    multi = z.png_info({c.name: c for c in _png.damage()}["flipped CRC of an IDAT"].blob)
    assert int(multi["idat_count"]) == 3 and int(multi["idat_bytes"]) > 100


def test_unfilter_inverts_filter_on_every_geometry_case():
    for k, ((colour, depth, w, h), c) in enumerate(zip(_png._GEOMETRY, _png.geometry())):
        bpp, rowbytes, size = _png.shape(w, h, colour, depth)
        filtered = _png.filter_rows(c.want, h, rowbytes, bpp, _png.pattern(h, k))
        assert _png.unfilter(filtered, h, rowbytes, bpp) == c.want, c.name
    bad = bytearray(_png.filter_rows(bytes(12), 3, 4, 1, [0, 1, 2]))
    bad[5] = 5
    assert _png.unfilter(bad, 3, 4, 1) is None


def test_pil_reads_the_writer_and_the_rule_accepts_pil():
    Image = pytest.importorskip("PIL.Image")
    modes = {(0, 8): "L", (2, 8): "RGB", (4, 8): "LA", (6, 8): "RGBA"}
    n = 0
    for (colour, depth, w, h), c in zip(_png._GEOMETRY, _png.geometry()):
        if (colour, depth) in modes:
            im = Image.open(io.BytesIO(c.blob))
            assert im.mode == modes[(colour, depth)] and im.size == (w, h) and im.tobytes() == c.want, c.name
            n += 1
    assert n >= 15
    rs = np.random.RandomState(3)
    for mode, colour in (("L", 0), ("RGB", 2), ("RGBA", 6), ("P", 3)):
        a = rs.randint(0, 256, size=(33, 21, {"L": 1, "P": 1, "RGB": 3, "RGBA": 4}[mode]), dtype=np.uint8)
        im = Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a, mode if mode != "P" else "L")
        if mode == "P":
            im = im.convert("P")
        buf = io.BytesIO()
        im.save(buf, "PNG")
        st, want = _png.info_rule(buf.getvalue())
        assert st == 0 and want["colour"] == colour and (want["width"], want["height"]) == (21, 33), mode


def test_info_accepts_pil_files(z):
    Image = pytest.importorskip("PIL.Image")
    a = np.random.RandomState(4).randint(0, 256, size=(40, 30, 3), dtype=np.uint8)
    for kw in ({}, {"optimize": True}, {"compress_level": 0}):
        buf = io.BytesIO()
        Image.fromarray(a, "RGB").save(buf, "PNG", **kw)
        rec = z.png_info(buf.getvalue())
        assert _png.info_dict(rec) == _png.info_rule(buf.getvalue())[1]
        assert (int(rec["width"]), int(rec["height"]), int(rec["bpp"]), int(rec["out_size"])) == (30, 40, 3, 3600)


def raw_info(z, a, info=True, flags=0, c=None):
    rec = np.full(1, 0, dtype=z.PNG_INFO)
    rec.view(np.uint8)[:] = 0xA5
    rc = z.lib().zes_png_info_get(a.ctypes.data if a is not None else None, (a.size if a is not None else 0) if c is None else c,
                                  rec.ctypes.data if info else None, flags)
    return rc, rec


def test_info_argument_errors_and_zeroed_record(z):
    a = np.frombuffer(_png.geometry()[0].blob, dtype=np.uint8)
    assert raw_info(z, a)[0] == 0
    assert raw_info(z, a, info=False)[0] == _png.ZES_E_ARG
    assert raw_info(z, None, c=8)[0] == _png.ZES_E_ARG
    for flags in (1, 4, 0x80000000):
        assert raw_info(z, a, flags=flags)[0] == _png.ZES_E_ARG
    rc, rec = raw_info(z, None, c=0)  # no bytes: not an argument error
    assert rc == _png.ZES_E_PNG and not rec.view(np.uint8).any()
    rc, rec = raw_info(z, np.frombuffer(_png.damage()[5].blob, dtype=np.uint8))
    assert rc == _png.ZES_E_UNSUPPORTED and not rec.view(np.uint8).any()


def raw_decode(z, blobs, count=None, alloc=True, out_len=True, status=True, lens=True, flags=0):
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
    rc = z.lib().zes_png_decode_alloc(ptrs, ln.ctypes.data if lens else None, cnt, z.ALLOC_FN(cb) if alloc else C.cast(None, z.ALLOC_FN), None,
                                      ol.ctypes.data if out_len else None, st.ctypes.data if status else None, None, flags)
    return rc, [int(x) for x in st[:cnt]], calls


def test_decode_alloc_before_the_device(z):
    import torch

    good = _png.geometry()[0].blob
    bad = [c.blob for c in _png.damage()[:7]]  # what the rule (and the interlace test) rejects on the host
    ARG = _png.ZES_E_ARG
    for flags in (1, 8, 16, 32, 4 | 64):
        assert raw_decode(z, [good], flags=flags)[0] == ARG
    assert raw_decode(z, [good], alloc=False)[0] == ARG
    assert raw_decode(z, [good], out_len=False)[0] == ARG
    assert raw_decode(z, [good], status=False)[0] == ARG
    assert raw_decode(z, [good], lens=False)[0] == ARG
    assert raw_decode(z, [good], count=0) == (0, [], [])  # nothing to do: ZES_OK, no device
    assert raw_decode(z, [], flags=4) == (0, [], [])
    assert z.png_decode_batch([]) == []
    # a batch in which no file passes the rule is answered on the host
    rc, st, calls = raw_decode(z, bad)
    assert (rc, calls) == (0, []) and st == [-24, -24, -24, -24, -24, -23, -23]
    res = z.png_decode_batch(bad)
    assert [r.code for r in res] == st
    with pytest.raises(z.ZlibEsError) as e:
        z.png_decode(bad[0])
    assert e.value.code == _png.ZES_E_PNG
    if not torch.cuda.is_available():  # anything else needs the device
        assert raw_decode(z, [good])[0] == _png.ZES_E_DEVICE
        assert raw_decode(z, bad + [good])[0] == _png.ZES_E_DEVICE


def test_status_string_and_dtype(z):
    assert z.ZES_E_PNG == -24 and "PNG" in z.strerror(-24) and "unknown" not in z.strerror(-24)
    assert z.PNG_INFO.itemsize == 72 and z.PNG_INFO.fields["trns_len"][1] == 64 and z.PNG_INFO.fields["rowbytes"][1] == 16


def test_png_entry_points_are_in_the_poison_catalogue(z, oracle):
    """What tests/test_poison_cpu.py asks of every entry point, for the PNG ones: covered by a catalogue entry that makes the
    call, or exempt for a stated reason; and the entries' expected values come out the same from the builders run again."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zes.h")).read(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"^\s*int\s+(zes_[a-z0-9_]+)\s*\(", text, flags=re.M)) if n.startswith("zes_png_"))
    assert names == sorted(list(_png_poison.COVERS) + list(_png_poison.EXEMPT)) and len(names) == 3
    for n in names:
        assert (n in P.COVERS) != (n in P.EXEMPT), n
    entries = list(P.catalogue(z, oracle).values())
    for fn, patterns in _png_poison.COVERS.items():
        for pat in patterns:
            assert any(fn in e.calls for e in P.covering(entries, pat)), (fn, pat)
    mine = [e for e in entries if any(fn in _png_poison.COVERS for fn in e.calls)]
    again = {e.name: e for e in _png_poison.entries(z, oracle)}
    assert len(mine) == 4 and sorted(again) == sorted(e.name for e in mine)
    for e in mine:
        assert e.source == "zlib" and e.want() == again[e.name].want() and len(e.want()) >= 11, e.name
