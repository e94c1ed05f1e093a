"""The TIFF reader without a GPU: tests/_tiff.py is sound (its reader inverts its writer, PIL reads its files to the same
pixels), zes_tiff_index gives what the helper's restatement of the file rule gives on every case, quirk and damaged file —
record, dirs, segment arrays, status — the damage table reaches every line of the rule, and the argument errors, the sizing
call, the record's size, zes_tiff_read_alloc's order of statuses, strerror and the exports are as include/zes.h says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _tiff as T
import _tiff_poison  # noqa: F401  (the catalogue entries and COVERS / EXEMPT lines of the new entry points)
from conftest import ROOT

ENTRY_POINTS = ("zes_tiff_index", "zes_tiff_index_dev", "zes_tiff_read_dev", "zes_tiff_read_alloc", "zes_last_tiff_read")


def all_cases():
    return list(T.grid()) + list(T.extra_cases())


def index_call(z, data, dir=0, cap=None):
    """zes_tiff_index through ctypes: (status, record as a dict, off, len, segments, dirs)."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    img = np.zeros(1, dtype=z.TIFF_IMAGE)
    nseg, dirs = C.c_uint64(99), C.c_uint32(99)
    if cap is None:
        rc = z.lib().zes_tiff_index(a.ctypes.data if a.size else None, a.size, dir, img.ctypes.data, None, None, 0, C.byref(nseg), C.byref(dirs), 0)
        if rc != T.E_NOSPACE:
            return rc, {k: int(img[0][k]) for k in T.FIELDS}, [], [], nseg.value, dirs.value
        cap = nseg.value
    off, ln = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
    rc = z.lib().zes_tiff_index(a.ctypes.data if a.size else None, a.size, dir, img.ctypes.data, off.ctypes.data, ln.ctypes.data, cap, C.byref(nseg),
                                C.byref(dirs), 0)
    return rc, {k: int(img[0][k]) for k in T.FIELDS}, [int(v) for v in off[:cap]], [int(v) for v in ln[:cap]], nseg.value, dirs.value


def test_the_helpers_reader_inverts_its_writer():
    for name, kw in all_cases():
        f, px = T.make(**kw)
        got = T.decode(f)
        assert got.shape == px.shape and got.dtype == px.dtype and (got == px).all(), name
        f2, _ = T.make(odd=False, **kw)
        assert (T.decode(f2) == px).all(), name
    f, (a, b) = T.two_directories()
    assert (T.decode(f, 0) == a).all() and (T.decode(f, 1) == b).all()
    for name, f, px in T.index_quirks():
        assert (T.decode(f) == px).all(), name
    # signed and float samples come back under their own dtype
    s = np.arange(-200, 200, dtype=np.int16).reshape(20, 20, 1)
    assert (T.decode(T.write([T.page(s, ("strips", 7), 8, 2, sample_format=2)], "MM")) == s).all()
    fl = np.linspace(-1, 1, 16 * 16 * 3, dtype=np.float32).reshape(16, 16, 3)
    got = T.decode(T.write([T.page(fl, ("tiles", 16, 16), 8, 1, sample_format=3)], "II"))
    assert got.dtype == np.float32 and (got == fl).all()


def test_pil_reads_the_helpers_files_to_the_same_pixels():
    Image = pytest.importorskip("PIL.Image")
    import io

    n = 0
    for name, kw in T.grid():
        if not ((kw["bits"] == 8 and kw["spp"] in (1, 3, 4)) or (kw["bits"] == 16 and kw["spp"] == 1)):
            continue
        f, px = T.make(**kw)
        im = Image.open(io.BytesIO(f))
        got = np.asarray(im)
        got = got.reshape(got.shape[0], got.shape[1], -1)
        assert got.shape == px.shape and (got.astype(np.uint32) == px).all(), (name, im.mode)
        n += 1
    assert n == 4 * len(T.LAYOUTS) * 2 * len(T.CODINGS)


def test_index_matches_the_rule_on_every_case(z):
    files = [(name, T.make(**kw)[0], 0) for name, kw in all_cases()] + [(name, f, 0) for name, f, _ in T.index_quirks()]
    two = T.two_directories()[0]
    files += [("two directories, the first", two, 0), ("two directories, the second", two, 1)]
    for name, f, d in files:
        rec, off, ln, dirs = T.rule(f, d)
        rc, got, goff, glen, nseg, gdirs = index_call(z, f, d)
        assert rc == T.OK, name
        assert got == rec and goff == off and glen == ln and nseg == len(off) == rec["across"] * rec["down"] and gdirs == dirs, name
    assert T.rule(two, 1)[3] == 2


def test_index_refuses_what_the_rule_refuses_and_the_table_reaches_every_line(z):
    reached = set()
    for name, f, d, status, line in T.index_damage():
        with pytest.raises(T.Refused) as r:
            T.rule(f, d)
        assert (r.value.status, r.value.line) == (status, line), name
        reached.add(line)
        rc, got, _, _, nseg, dirs = index_call(z, f, d)
        assert rc == status, name
        assert not any(got.values()) and nseg == 0, name  # with any status the record is zeros
        assert dirs == r.value.dirs, name
    assert reached == set(T.LINES) - set(T.UNREACHABLE)
    assert len(T.LINES) == len(set(T.LINES))


def test_sizing_call_capacity_and_argument_errors(z):
    f, _ = T.make(w=37, h=23, spp=3, bits=8, layout=("tiles", 16, 16), order="II", compression=8, predictor=2)
    rec, off, ln, _ = T.rule(f)
    a = np.frombuffer(f, dtype=np.uint8)
    img = np.zeros(1, dtype=z.TIFF_IMAGE)
    nseg, dirs = C.c_uint64(), C.c_uint32()
    L = z.lib()
    # cap == 0 is the sizing call: the record and the counts are filled
    assert L.zes_tiff_index(a.ctypes.data, a.size, 0, img.ctypes.data, None, None, 0, C.byref(nseg), C.byref(dirs), 0) == T.E_NOSPACE
    assert nseg.value == 6 and dirs.value == 1 and {k: int(img[0][k]) for k in T.FIELDS} == rec
    rc, got, goff, _, nseg5, _ = index_call(z, f, 0, cap=5)
    assert rc == T.E_NOSPACE and nseg5 == 6 and got == rec and goff == [0] * 5  # (nothing is written into a short array)
    rc, got, goff, glen, _, _ = index_call(z, f, 0, cap=9)
    assert rc == T.OK and goff[:6] == off and glen[:6] == ln
    # dir >= dirs: ZES_E_ARG with dirs filled
    rc, got, _, _, _, d = index_call(z, f, 1)
    assert rc == T.E_ARG and d == 1 and not any(got.values())
    two = T.two_directories()[0]
    assert index_call(z, two, 2)[0] == T.E_ARG and index_call(z, two, 2)[5] == 2
    o = np.zeros(8, dtype=np.uint64)
    args = lambda **kw: [kw.get("p", a.ctypes.data), kw.get("c", a.size), 0, kw.get("img", img.ctypes.data), kw.get("off", o.ctypes.data),
                         kw.get("len", o.ctypes.data), kw.get("cap", 8), kw.get("n", C.byref(nseg)), kw.get("dirs", C.byref(dirs)), kw.get("flags", 0)]
    assert L.zes_tiff_index(*args()) == T.OK
    for bad in (dict(img=None), dict(n=None), dict(dirs=None), dict(p=None), dict(flags=4), dict(off=None), dict(len=None)):
        assert L.zes_tiff_index(*args(**bad)) == T.E_ARG, bad
    assert L.zes_tiff_index(None, 0, 0, img.ctypes.data, None, None, 0, C.byref(nseg), C.byref(dirs), 0) == T.E_TIFF  # (no bytes: the rule's)


def test_the_record_mirror_and_the_python_forms(z):
    assert z.TIFF_IMAGE.itemsize == 48 and z.TIFF_IMAGE.names == T.FIELDS
    text = open(os.path.join(ROOT, "include", "zes.h")).read()
    assert re.search(r"typedef struct zes_tiff_image \{\s*/\* 48 bytes \*/", text)
    f, (a, b) = T.two_directories()
    info = z.tiff_info(f, 1)
    rec, off, ln, dirs = T.rule(f, 1)
    assert info == dict(rec, dirs=2)
    got, goff, glen = z.tiff_index(f, 1)
    assert got == info and list(goff) == off and list(glen) == ln
    assert z.tiff_dtype(dict(bits=16, sample_format=2)) == np.int16 and z.tiff_dtype(dict(bits=32, sample_format=3)) == np.float32
    assert z.tiff_dtype(dict(bits=32, sample_format=1)) == np.uint32 and z.tiff_dtype(dict(bits=8, sample_format=2)) == np.int8
    with pytest.raises(z.ZlibEsError) as e:
        z.tiff_info(f, 2)
    assert e.value.code == T.E_ARG and e.value.dirs == 2
    with pytest.raises(z.ZlibEsError) as e:
        z.tiff_info(b"not a TIFF file")
    assert e.value.code == T.E_TIFF == z.ZES_E_TIFF


def test_read_alloc_answers_the_rules_statuses_before_it_needs_a_device(z):
    import torch

    got = []

    def alloc(_u, _i, n):
        got.append(n)
        return None

    fn = z.ALLOC_FN(alloc)
    n = C.c_uint64(7)
    img = np.ones(1, dtype=z.TIFF_IMAGE)

    def call(f, d=0, rect=None, flags=0, fn=fn):
        a = np.frombuffer(bytes(f), dtype=np.uint8)
        r = (C.c_uint32 * 4)(*rect) if rect else None
        return z.lib().zes_tiff_read_alloc(a.ctypes.data if a.size else None, a.size, d, r, fn, None, C.byref(n), img.ctypes.data, flags)

    good, _ = T.make(w=37, h=23, spp=1, bits=8, layout=("tiles", 16, 16), order="II", compression=8, predictor=2)
    for name, f, d, status, _ in T.index_damage():
        assert call(f, d) == status, name
        assert n.value == 0 and not any(int(img[0][k]) for k in T.FIELDS), name
    assert call(good, flags=1) == T.E_ARG and call(good, fn=z.ALLOC_FN()) == T.E_ARG  # (a null allocator)
    for rect in ((0, 0, 0, 1), (0, 0, 1, 0), (37, 0, 1, 1), (30, 0, 8, 1), (0, 20, 1, 4), (0xFFFFFFFF, 0, 2, 1)):
        assert call(good, rect=rect) == T.E_ARG, rect
    if not torch.cuda.is_available():
        assert call(good) == T.E_DEVICE  # reached only behind the rule's own statuses
    assert not got


def test_strerror_header_and_exports(z):
    assert "TIFF" in z.strerror(-25) and z.strerror(-25) != z.strerror(-24)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zes.h")).read(), flags=re.S)
    assert re.search(r"ZES_E_TIFF = -25\b", text)
    declared = set(re.findall(r"^\s*int\s+(zes_[a-z0-9_]+)\s*\(", text, flags=re.M))
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert getattr(z.lib(), name) is not None, name
