"""The ZIP reader's host side, without a GPU: zes_zip_index against its restated rule (tests/_zip.py) and CPython's zipfile,
the reject list with exact statuses, the count query and the argument errors, and what zes_zip_read_alloc answers before it
touches a device."""
import ctypes as C
import io
import os
import re
import zipfile

import numpy as np
import pytest

import _zip
import _poison_cases as P
import _zip_poison
from conftest import ROOT

FIELDS = ("hdr_off", "name_pos", "csize", "usize", "crc", "name_off", "name_len", "method", "flags", "pad")


@pytest.fixture(scope="module")
def archives():
    return _zip.cpython_archives()


@pytest.fixture(scope="module")
def rejects():
    return _zip.reject_cases()


def index_status(z, b):
    """zes_zip_index through the package -> (status, entries, names)."""
    try:
        ent, names = z.zip_index(b)
    except z.ZlibEsError as e:
        return e.code, None, None
    return 0, ent, names


def same_as_rule(ent, names, b):
    st, want, want_names = _zip.index_rule(b)
    assert st == 0 and len(want) == ent.size and names == want_names
    for e, w in zip(ent, want):
        assert {f: int(e[f]) for f in FIELDS} == w


def test_builder_archives_are_read_by_zipfile():
    b, plain, _ = _zip.standard()
    fb, plan = _zip.failures()
    good = [_zip.entry(b"good/%d" % k, data, method=8 if k & 1 else 0) for k, (_, want, data) in enumerate(plan) if want == 0]
    for blob, want in ((b, plain), (_zip.build(good, prefix=b"#!stub\n" * 9, comment=b"made by the builder"), [e["data"] for e in good])):
        with zipfile.ZipFile(io.BytesIO(blob)) as zf:
            assert zf.testzip() is None
            assert [zf.read(zi) for zi in zf.infolist()] == want
    with zipfile.ZipFile(io.BytesIO(b)) as zf:
        st, ent, names = _zip.index_rule(b)
        assert st == 0 and [zi.orig_filename.encode() for zi in zf.infolist()] == names
    # the good entries of the failure archive are what zipfile reads as well (it lists the archive: the directory is sound)
    with zipfile.ZipFile(io.BytesIO(fb)) as zf:
        for zi, (what, want, data) in zip(zf.infolist(), plan):
            if want == 0:
                assert zf.read(zi) == data, what


def test_index_equals_rule_and_zipfile(z, archives):
    assert sorted(archives) == sorted(["seekable with a comment", "unseekable, bit 3", "force_zip64", "a 100-byte prefix", "no entries", "a bzip2 entry",
                                       "a UTF-8 name", "300 entries"])
    for what, b in archives.items():
        st, ent, names = index_status(z, b)
        assert st == 0, what
        same_as_rule(ent, names, b)
        info = _zip.infolist(b)
        assert len(info) == ent.size, what
        for e, zi, name in zip(ent, info, names):
            assert {f: int(e[f]) for f in ("hdr_off", "csize", "usize", "crc", "method", "flags")} == {f: zi[f] for f in zi if f != "name"}, what
            assert name.decode("utf-8" if int(e["flags"]) & 0x800 else "cp437") == zi["name"], what
            assert b[int(e["name_pos"]):int(e["name_pos"]) + int(e["name_len"])] == name, what
    # what the cases are there for
    assert all(int(e["flags"]) & 8 for e in index_status(z, archives["unseekable, bit 3"])[1])
    b = archives["force_zip64"]
    assert all(_zip.le16(b, int(e["hdr_off"]) + 28) == 20 for e in index_status(z, b)[1])
    assert [int(e["hdr_off"]) for e in index_status(z, archives["a 100-byte prefix"])[1]][0] == 100
    assert [int(e["method"]) for e in index_status(z, archives["a bzip2 entry"])[1]] == [8, 12]
    assert int(index_status(z, archives["a UTF-8 name"])[1][0]["flags"]) & 0x800


def test_reject_list(z, rejects):
    for what, (b, status, count) in rejects.items():
        st, ent, names = index_status(z, b)
        assert st == status, (what, st, status)
        if status == 0:
            assert ent.size == count, what
            same_as_rule(ent, names, b)


def raw_index(z, a, ent, cap, names, names_cap, flags=0, entries=True, names_len=True, c=None):
    n, nl = C.c_uint64(77), C.c_uint64(77)
    rc = z.lib().zes_zip_index(a.ctypes.data if a is not None else None, (a.size if a is not None else 0) if c is None else c,
                               ent.ctypes.data if ent is not None else None, cap, C.byref(n) if entries else None,
                               names.ctypes.data if names is not None else None, names_cap, C.byref(nl) if names_len else None, flags)
    return rc, n.value, nl.value


def test_count_query_and_nospace(z, archives):
    b = archives["seekable with a comment"]
    a = np.frombuffer(b, dtype=np.uint8)
    _, want, want_names = _zip.index_rule(b)
    total = sum(len(n) for n in want_names)
    assert raw_index(z, a, None, 0, None, 0) == (_zip.ZES_E_NOSPACE, len(want), total)
    empty = np.frombuffer(archives["no entries"], dtype=np.uint8)
    assert raw_index(z, empty, None, 0, None, 0) == (_zip.ZES_E_NOSPACE, 0, 0)  # the query's answer on every valid archive
    ent = np.frombuffer(b"\xA5" * 40 * (len(want) + 1), dtype=z.ZIP_ENTRY).copy()
    names = np.full(total + 8, 0xA5, dtype=np.uint8)
    assert raw_index(z, empty, ent, ent.size, names, names.size) == (0, 0, 0)
    canary = ent.tobytes()
    # either capacity too small: the counts, and nothing written
    assert raw_index(z, a, ent, len(want) - 1, names, total) == (_zip.ZES_E_NOSPACE, len(want), total)
    assert raw_index(z, a, ent, len(want), names, total - 1) == (_zip.ZES_E_NOSPACE, len(want), total)
    assert ent.tobytes() == canary and (names == 0xA5).all()
    # exact capacities: the records, the names, and nothing behind them
    assert raw_index(z, a, ent, len(want), names, total) == (0, len(want), total)
    assert ent[len(want):].tobytes() == canary[40 * len(want):] and (names[total:] == 0xA5).all()
    assert names[:total].tobytes() == b"".join(want_names)
    for e, w in zip(ent, want):
        assert {f: int(e[f]) for f in FIELDS} == w


def test_index_argument_errors(z, archives):
    a = np.frombuffer(archives["seekable with a comment"], dtype=np.uint8)
    ent = np.zeros(8, dtype=z.ZIP_ENTRY)
    names = np.zeros(256, dtype=np.uint8)
    ARG = _zip.ZES_E_ARG
    assert raw_index(z, a, ent, 8, names, 256, entries=False)[0] == ARG
    assert raw_index(z, a, ent, 8, names, 256, names_len=False)[0] == ARG
    assert raw_index(z, None, ent, 8, names, 256, c=22)[0] == ARG
    for flags in (1, 4, 64, 0x80000000):
        assert raw_index(z, a, ent, 8, names, 256, flags=flags)[0] == ARG
    assert raw_index(z, a, None, 8, names, 256)[0] == ARG
    assert raw_index(z, a, ent, 8, None, 256)[0] == ARG
    assert raw_index(z, None, None, 0, None, 0, c=0)[0] == _zip.ZES_E_ZIP  # no bytes: not an argument error


def raw_read(z, a, ent, sel, count, alloc=True, out_len=True, status=True, flags=0, nent=None, c=None):
    calls = []

    def cb(_user, i, n):
        calls.append((i, n))
        return None

    fn = z.ALLOC_FN(cb)
    ol = (C.c_uint64 * max(count, 1))()
    st = (C.c_int32 * max(count, 1))()
    s = None if sel is None else np.ascontiguousarray(sel, dtype=np.uint32)
    rc = z.lib().zes_zip_read_alloc(a.ctypes.data if a is not None else None, (a.size if a is not None else 0) if c is None else c,
                                    ent.ctypes.data if ent is not None else None, (ent.size if ent is not None else 0) if nent is None else nent,
                                    s.ctypes.data if s is not None else None, count, fn if alloc else C.cast(None, z.ALLOC_FN),
                                    None, ol if out_len else None, st if status else None, flags)
    return rc, calls


def test_read_alloc_before_the_device(z, archives):
    import torch

    b = archives["seekable with a comment"]
    a = np.frombuffer(b, dtype=np.uint8)
    ent, _ = z.zip_index(b)
    ARG = _zip.ZES_E_ARG
    assert raw_read(z, a, ent, None, ent.size + 1)[0] == ARG  # count > nent without sel
    assert raw_read(z, a, ent, [0, ent.size], 2)[0] == ARG  # sel[i] >= nent
    for flags in (1, 8, 16, 32, 4 | 64):
        assert raw_read(z, a, ent, None, 1, flags=flags)[0] == ARG
    assert raw_read(z, None, ent, None, 1, c=a.size)[0] == ARG
    assert raw_read(z, a, None, None, 1, nent=ent.size)[0] == ARG
    assert raw_read(z, a, ent, None, 1, alloc=False)[0] == ARG
    assert raw_read(z, a, ent, None, 1, out_len=False)[0] == ARG
    assert raw_read(z, a, ent, None, 1, status=False)[0] == ARG
    assert raw_read(z, a, ent, None, 0) == (0, [])  # nothing to do: ZES_OK, no device
    assert raw_read(z, a, ent, [], 0, flags=4) == (0, [])
    assert z.zip_read(b, (ent, None), sel=[]) == []
    if not torch.cuda.is_available():  # anything else needs the device
        assert raw_read(z, a, ent, None, ent.size) == (_zip.ZES_E_DEVICE, [])
        assert raw_read(z, a, ent, [1], 1) == (_zip.ZES_E_DEVICE, [])


def test_status_strings(z):
    assert (z.ZES_E_ZIP, z.ZES_E_UNSUPPORTED) == (-22, -23)
    assert "ZIP" in z.strerror(-22) and "unsupported" in z.strerror(-23)


def test_zip_entry_points_are_in_the_poison_catalogue(z, oracle):
    """What tests/test_poison_cpu.py asks of every entry point, for the ZIP ones: covered by a catalogue entry that makes the
    call, or exempt for a stated reason; and the entries' expected values come out the same from the builders run again."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zes.h")).read(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"^\s*int\s+(zes_[a-z0-9_]+)\s*\(", text, flags=re.M)) if n.startswith("zes_zip_"))
    assert names == sorted(list(_zip_poison.COVERS) + list(_zip_poison.EXEMPT)) and len(names) == 4
    for n in names:
        assert (n in P.COVERS) != (n in P.EXEMPT), n
    entries = list(P.catalogue(z, oracle).values())
    for fn, patterns in _zip_poison.COVERS.items():
        for pat in patterns:
            assert any(fn in e.calls for e in P.covering(entries, pat)), (fn, pat)
    mine = [e for e in entries if any(fn in _zip_poison.COVERS for fn in e.calls)]
    again = {e.name: e for e in _zip_poison.entries(z, oracle)}
    assert len(mine) == 4 and sorted(again) == sorted(e.name for e in mine)
    for e in mine:
        assert e.source == "zlib" and e.want() == again[e.name].want() and len(e.want()) >= 18, e.name
