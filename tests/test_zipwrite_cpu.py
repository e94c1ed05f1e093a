"""The ZIP writer's host side, without a GPU: the bound, the archive of no entries, the argument errors and what is refused
before any device work; and the expectation itself — the archives tests/_zipwrite.py builds from the CPU oracle are read back by
CPython's zipfile and accepted by the restated index rule, and the methods come out as include/zes.h says."""
import ctypes as C
import io
import os
import re
import zipfile

import numpy as np
import pytest

import _zip
import _zipwrite as W
import _poison_cases as P
import _zipwrite_poison
from conftest import ROOT

END0 = b"PK\x05\x06" + bytes(18)


def test_bound_is_the_formula(z):
    es = W.cases(z)
    assert z.zip_bound([len(d) for _, d in es], [len(n) for n, _ in es]) == W.bound(es)
    assert z.zip_bound([], []) == 22
    assert z.zip_bound([0], [0]) == 30 + 46 + 22
    assert z.zip_bound([0xFFFFFFFE, 5], [65535, 1]) == (30 + 65535 + 0xFFFFFFFE) + (30 + 1 + 5) + (46 + 65535) + (46 + 1) + 22
    cap = C.c_uint64()
    ln, nl = np.array([5], dtype=np.uint64), np.array([1], dtype=np.uint16)
    lib = z.lib()
    assert lib.zes_zipwrite_bound(ln.ctypes.data, nl.ctypes.data, 1, None) == _zip.ZES_E_ARG
    assert lib.zes_zipwrite_bound(None, nl.ctypes.data, 1, C.byref(cap)) == _zip.ZES_E_ARG
    assert lib.zes_zipwrite_bound(ln.ctypes.data, None, 1, C.byref(cap)) == _zip.ZES_E_ARG
    assert lib.zes_zipwrite_bound(None, None, 0, C.byref(cap)) == 0 and cap.value == 22
    # an archive of stored entries only has exactly the bound's size
    stored = [(n, d) for n, d in es if W.entry(n, d)["method"] == 0]
    assert len(stored) >= 10 and len(W.expect(stored)) == W.bound(stored)
    assert len(W.expect(es)) < W.bound(es)


def test_no_entries_is_the_end_record(z):
    rc, n, out, ent = W.host_write(z, [], cap=22)
    assert (rc, n) == (0, 22) and out[:22].tobytes() == END0 == W.expect([]) and (out[22:] == 0xA5).all()
    rc, n, out, _ = W.host_write(z, [], cap=21)
    assert (rc, n) == (_zip.ZES_E_NOSPACE, 22) and (out == 0xA5).all()
    assert W.host_write(z, [], cap=0, null_out=True)[:2] == (_zip.ZES_E_NOSPACE, 22)
    assert W.host_write(z, [], cap=30, flags=W.PIECES, want_ent=False)[:2] == (0, 22)
    arch, (ent, names) = z.zip_write([])
    assert arch.tobytes() == END0 and ent.size == 0 and names == []
    assert _zip.index_rule(END0) == (0, [], [])


def test_the_expected_archives_are_zip_files(z):
    """The expectation, pinned: CPython's zipfile reads every entry of the expected archives back, dated 1980-01-01, the
    restated index rule lists them, and every method is the one the rule's description names for that shape."""
    es = W.cases(z)
    assert max(len(d) for _, d in es) == 300000 and any(len(n) == 300 for n, _ in es) and any(n == b"" for n, _ in es)
    assert [len(d) for n, d in es if n.startswith(b"same/")] == [20000, 20000]
    want = W.want_methods(z)
    for (n, d) in es:
        e = W.entry(n, d)
        assert n not in want or e["method"] == want[n], n
        assert e["flags"] == (0x0800 if max(n, default=0) >= 0x80 else 0)
        assert e["method"] == 0 or len(e["body"]) < len(d)
    assert sum(1 for n, _ in es if W.name_flags(n)) == 1
    for what, arch in [("the case list", es), ("nine entries", W.nine(z)), ("six entries", W.slots(z))] + [(repr(n[:24]), [(n, d)]) for n, d in es]:
        blob = W.expect(arch)
        with zipfile.ZipFile(io.BytesIO(blob)) as zf:
            infos = zf.infolist()
            assert zf.testzip() is None, what
            assert [zf.read(zi) for zi in infos] == [d for _, d in arch], what
            assert all(zi.date_time == (1980, 1, 1, 0, 0, 0) for zi in infos), what
            assert [zi.orig_filename.encode("utf-8" if zi.flag_bits & 0x800 else "cp437") for zi in infos] == [n for n, _ in arch], what
        st, ent, names = _zip.index_rule(blob)
        assert st == 0 and names == [n for n, _ in arch], what
        assert [(e["method"], e["usize"]) for e in ent] == [(W.entry(n, d)["method"], len(d)) for n, d in arch], what
        for e in ent:
            assert _zip.entry_rule(blob, e)[0] == 0, what
        # the library's bound holds for it, and is its size when nothing is deflated
        cap = z.zip_bound([len(d) for _, d in arch], [len(n) for n, _ in arch])
        assert len(blob) <= cap and (len(blob) == cap) == all(e["method"] == 0 for e in ent), what
    assert len(W.nine(z)) == 9 and W.groups(W.nine(z), W.PIECES) == [4, 4, 1] and W.groups(W.nine(z)) == [9]
    # six entries whose groups end at the slots' bytes: more groups than their number alone makes
    assert W.groups(W.slots(z), W.PIECES) == [2, 2, 2] and W.groups(W.slots(z)) == [6] and W.groups(es) == [len(es)]
    assert min(W.groups(es, W.PIECES)[:-1]) < 4  # (one of the case list's groups ends at its slots as well)
    # a stream as long as its data is stored: the search of tests/_zipwrite.py, run again where its finds lie
    assert W.exact_search(z, range(2, 65)) == [(k, n) for n in range(2, 65) for k in ("itext", "zeros") if (k, n) in W.EXACT]
    assert len(W.EXACT) == 4 and all(W.entry(b"x", bytes(n) if k == "zeros" else z.gen("itext", 7, n).tobytes())["method"] == 0 for k, n in W.EXACT)


def test_argument_errors(z):
    es = [(b"a", b"hello hello hello"), (b"bb", b"")]
    ARG = _zip.ZES_E_ARG
    assert W.host_write(z, es, out_len=False)[0] == ARG
    assert W.host_write(z, es, ptrs=False)[0] == ARG
    assert W.host_write(z, es, in_len=False)[0] == ARG
    assert W.host_write(z, es, name_len=False)[0] == ARG
    assert W.host_write(z, es, names=False)[0] == ARG
    assert W.host_write(z, es, null_out=True)[0] == ARG  # (cap != 0)
    assert W.host_write(z, es, null_in=0)[0] == ARG  # in[0] null, in_len[0] != 0
    for flags in (1, 2, 8, 16, 32, 64, 4 | 1, 0x80000000):
        assert W.host_write(z, es, flags=flags)[0] == ARG
    rc, n, out, _ = W.host_write(z, es, null_in=0)
    assert n == 0 and (out == 0xA5).all()
    # the device form decides the same from its arguments (no device is touched: the pointers are never followed)
    off, ln = np.zeros(2, dtype=np.uint64), np.array([17, 0], dtype=np.uint64)
    blob, nl = W.names_arrays(es)
    n = C.c_uint64(77)
    dev = lambda d_in=0x1000, off=off, ln=ln, blob=blob, nl=nl, d_out=0x2000, cap=1 << 20, n=n, flags=0: z.lib().zes_zipwrite_dev(
        d_in, W.ptr(off) if off is not None else None, W.ptr(ln) if ln is not None else None, W.ptr(blob) if blob is not None else None,
        W.ptr(nl) if nl is not None else None, 2, d_out, cap, C.byref(n) if n is not None else None, None, flags)
    assert dev(d_in=None) == ARG and dev(off=None) == ARG and dev(ln=None) == ARG and dev(blob=None) == ARG and dev(nl=None) == ARG
    assert dev(d_out=None) == ARG and dev(n=None) == ARG and dev(flags=1) == ARG and dev(flags=4 | 64) == ARG


def test_unsupported_is_decided_before_the_data_is_read(z):
    UNS = _zip.ZES_E_UNSUPPORTED
    # a length no ZIP entry without ZIP64 has: the pointer leads to three bytes, which are not read
    assert W.host_write(z, [(b"big", b"abc")], lens=[0xFFFFFFFF], cap=64)[:2] == (UNS, 0)
    assert W.host_write(z, [(b"ok", b"abcd"), (b"big", b"abc")], lens=[4, 1 << 40], cap=64)[:2] == (UNS, 0)
    many = [(b"", b"x")] * 65535
    assert W.host_write(z, many, cap=64)[:2] == (UNS, 0)
    off, ln, nl = np.zeros(65535, dtype=np.uint64), np.ones(65535, dtype=np.uint64), np.zeros(65535, dtype=np.uint16)
    n = C.c_uint64(77)
    dev = lambda cnt, ln: z.lib().zes_zipwrite_dev(0x1000, off.ctypes.data, ln.ctypes.data, None, nl.ctypes.data, cnt, 0x2000, 1 << 20, C.byref(n), None, 0)
    assert dev(65535, ln) == UNS and n.value == 0
    ln2 = ln.copy()
    ln2[1] = 0xFFFFFFFF
    assert dev(2, ln2) == UNS


def test_device_error_without_a_gpu(z):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_zipwrite.py runs these calls")
    es = [(b"a", b"hello hello hello hello hello hello hello hello hello")]
    assert W.host_write(z, es)[:2] == (_zip.ZES_E_DEVICE, 0)
    assert W.host_write(z, [(b"", b"")])[0] == _zip.ZES_E_DEVICE  # one entry of no bytes is still a call for the device
    assert W.host_write(z, [], cap=22)[0] == 0  # no entries: none is needed
    with pytest.raises(z.ZlibEsError) as e:
        z.zip_write(es)
    assert e.value.code == _zip.ZES_E_DEVICE


def test_entry_points_are_exported_and_in_the_poison_catalogue(z, oracle):
    """What tests/test_zip_cpu.py checks for the reader's four: declared, exported, covered by a catalogue entry that makes the
    call or exempt for a stated reason, and the entries' expected values come out the same from the builders run again."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zes.h")).read(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"^\s*int\s+(zes_[a-z0-9_]+)\s*\(", text, flags=re.M)) if n.startswith("zes_zipwrite"))
    assert names == ["zes_zipwrite", "zes_zipwrite_bound", "zes_zipwrite_dev"] == sorted(list(_zipwrite_poison.COVERS) + list(_zipwrite_poison.EXEMPT))
    for n in names:
        assert hasattr(z.lib(), n), n
        assert (n in P.COVERS) != (n in P.EXEMPT), n
    assert not any(n.startswith("zes_zip_") for n in names)
    entries = list(P.catalogue(z, oracle).values())
    for fn, patterns in _zipwrite_poison.COVERS.items():
        for pat in patterns:
            assert any(fn in e.calls for e in P.covering(entries, pat)), (fn, pat)
    mine = [e for e in entries if any(fn in _zipwrite_poison.COVERS for fn in e.calls)]
    again = {e.name: e for e in _zipwrite_poison.entries(z, oracle)}
    assert len(mine) == 6 and sorted(again) == sorted(e.name for e in mine)
    for e in mine:
        assert e.source == "oracle" and all(c.startswith("zes_zipwrite") for c in e.calls), e.name
        assert e.want() == again[e.name].want() and e.want()[0] == "out" and e.want()[1] > 100000, e.name
    assert "reader only" not in open(os.path.join(ROOT, "include", "zes.h")).read()
