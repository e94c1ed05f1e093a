"""The gzip batch forms without a GPU (include/zes.h: "zes_gzip_batch*", "zes_gunzip_batch*"): the bound's arithmetic, the
expected-file builder of tests/_gzip_batch.py against CPython's gzip, the reader's case lists against the verdicts they claim,
the argument rules that are decided before the device, and the entry points' place in the poison catalogue."""
import ctypes as C
import gzip
import os
import re
import struct
import zlib

import numpy as np
import pytest

import _gzip_batch as G
import _gzip_batch_poison
import _poison_cases as P
from conftest import ROOT


def test_bound_values(z):
    lens = sorted(G.BOUNDS)
    assert lens == [0, 1, 65535, 65536, 131070, 131071]
    assert z.gzip_batch_bound(lens) == [G.BOUNDS[n] for n in lens] == [G.bound(n) for n in lens]
    assert z.gzip_batch_bound([]) == []
    assert z.gzip_batch_bound([1 << 32, (1 << 32) - 1]) == [0, G.bound((1 << 32) - 1)]  # (a length that ISIZE cannot state has no file)
    cap = np.zeros(1, dtype=np.uint64)
    assert z.lib().zes_gzip_batch_bound(None, 1, cap.ctypes.data) == G.E_ARG and z.lib().zes_gzip_batch_bound(cap.ctypes.data, 1, None) == G.E_ARG


def test_the_builders_stored_files_decode_with_gzip(z):
    seen = set()
    for name, data in G.writer_cases(z):
        f, kind = G.expect(data)
        assert gzip.decompress(f) == data and struct.unpack("<II", f[-8:]) == (zlib.crc32(data), len(data)), name
        assert f[:10] == G.HEADER and len(f) <= G.bound(len(data)), name
        if kind != "stream":
            body = G.stored_body(data)
            assert len(f) == G.bound(len(data)) == 18 + body.size and zlib.decompress(body.tobytes(), -15) == data, name
            blocks = max(1, -(-len(data) // 65535))
            seen.add("two blocks" if blocks >= 2 else "one block")
            assert body[0] == (1 if blocks == 1 else 0) and body[(blocks - 1) * 65540] == 1, name
        seen.add(kind)
    assert seen == {"stream", "longer", "refused", "one block", "two blocks"}
    assert G.stored_body(b"").tobytes() == bytes([1, 0, 0, 0xFF, 0xFF])
    assert [n for n, _ in G.nine(z)][8] == "text 300000" and len(G.nine(z)) == 9


def test_the_readers_files_have_the_verdicts_the_lists_claim(z):
    good = G.good_files(z)
    assert len(good) == 10 and {len(p) % 16 == 0 for _, _, p in good} == {True, False}
    for name, f, plain in good:
        assert G.py_verdict(f) == plain and len(f) >= 18, name
    assert any(f[3] == 4 for _, f, _ in good) and any(f[3] == 8 for _, f, _ in good) and any(f[3] == 16 for _, f, _ in good) and any(f[3] == 28 for _, f, _ in good)
    files = G.serial_files(z)
    assert len(files) == 22 and len({n for n, _, _, _ in files}) == 22
    for name, f, verdict, delta in files:
        assert G.py_verdict(f) == verdict, name
        assert delta == 0 or verdict, name
    lens = {n: len(f) for n, f, _, _ in files}
    assert (lens["no bytes"], lens["10 bytes"], lens["17 bytes"], lens["40 bytes claiming 0xFFFFFFF0"]) == (0, 10, 17, 40)
    f40, plain = G.forty_good(z)
    assert len(f40) == 40 and gzip.decompress(f40) == plain
    assert set(_gzip_batch_poison.STATED) <= set(lens)


def _arrays(n):
    return np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.int32)


def test_argument_rules_are_decided_before_the_device(z):
    L = z.lib()
    a = np.arange(100, dtype=np.uint8)
    ln, out_len, status = _arrays(1)
    ln[0] = 100
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    nul = (C.c_void_p * 1)(None)
    keep = []

    def alloc(_u, _i, n):
        keep.append(np.empty(max(int(n), 1), dtype=np.uint8))
        return keep[-1].ctypes.data

    fn = z.ALLOC_FN(alloc)
    for host in (L.zes_gzip_batch, L.zes_gunzip_batch_alloc):
        assert host(ptrs, ln.ctypes.data, 0, fn, None, out_len.ctypes.data, status.ctypes.data, 0) == 0  # no files: no device work
        assert host(None, None, 0, fn, None, None, None, 0) == 0
        assert host(ptrs, ln.ctypes.data, 1, z.ALLOC_FN(), None, out_len.ctypes.data, status.ctypes.data, 0) == G.E_ARG
        assert host(None, ln.ctypes.data, 1, fn, None, out_len.ctypes.data, status.ctypes.data, 0) == G.E_ARG
        assert host(nul, ln.ctypes.data, 1, fn, None, out_len.ctypes.data, status.ctypes.data, 0) == G.E_ARG
        assert host(ptrs, None, 1, fn, None, out_len.ctypes.data, status.ctypes.data, 0) == G.E_ARG
        assert host(ptrs, ln.ctypes.data, 1, fn, None, None, status.ctypes.data, 0) == G.E_ARG
        assert host(ptrs, ln.ctypes.data, 1, fn, None, out_len.ctypes.data, None, 0) == G.E_ARG
        assert host(ptrs, ln.ctypes.data, 1, fn, None, out_len.ctypes.data, status.ctypes.data, 1) == G.E_ARG  # ZES_F_NO_FASTPATH
    assert L.zes_gzip_batch(ptrs, ln.ctypes.data, 1, fn, None, out_len.ctypes.data, status.ctypes.data, G.SERIAL) == G.E_ARG
    off = np.zeros(1, dtype=np.uint64)
    for dev in (L.zes_gzip_batch_dev, L.zes_gunzip_batch_dev):
        assert dev(None, None, None, 0, None, None, None, None, None, 0) == 0
        assert dev(None, off.ctypes.data, ln.ctypes.data, 1, None, off.ctypes.data, off.ctypes.data, out_len.ctypes.data, status.ctypes.data, 0) == G.E_ARG
        assert dev(None, off.ctypes.data, off.ctypes.data, 1, None, off.ctypes.data, off.ctypes.data, out_len.ctypes.data, status.ctypes.data, 8) == G.E_ARG
        assert dev(None, None, off.ctypes.data, 1, None, off.ctypes.data, off.ctypes.data, out_len.ctypes.data, status.ctypes.data, 0) == G.E_ARG
        assert dev(None, off.ctypes.data, off.ctypes.data, 1, None, None, off.ctypes.data, out_len.ctypes.data, status.ctypes.data, 0) == G.E_ARG
        assert dev(None, off.ctypes.data, off.ctypes.data, 1, None, off.ctypes.data, None, out_len.ctypes.data, status.ctypes.data, 0) == G.E_ARG
    assert not keep  # no allocator call without a result
    # a length that ISIZE cannot state is that file's ZES_E_UNSUPPORTED before any launch: alone in its call, no device is needed
    ln[0] = 1 << 32
    status[0], out_len[0] = 7, 7
    assert L.zes_gzip_batch(ptrs, ln.ctypes.data, 1, fn, None, out_len.ctypes.data, status.ctypes.data, 0) == 0
    assert (status[0], out_len[0]) == (G.E_UNSUPPORTED, 0) and not keep


def test_no_cpu_fallback_without_gpu(z):
    """As tests/test_cabi_cpu.py expects of a compute call: without the library's device the batch calls answer ZES_E_DEVICE."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for call in (lambda: z.gzip_batch([b"some bytes to write"]), lambda: z.gunzip_batch([gzip.compress(b"some bytes to read")])):
        with pytest.raises(z.ZlibEsError) as ei:
            call()
        assert ei.value.code == G.E_DEVICE
    assert z.gzip_batch([]) == [] and z.gunzip_batch([]) == [] and z.last_gunzip_batch() == (0, 0)


def test_entry_points_are_exported_and_in_the_poison_catalogue(z, oracle):
    """What tests/test_zipwrite_cpu.py checks for the ZIP writer's three: declared, exported, covered by a catalogue entry that
    makes the call or exempt for a stated reason, and the entries' expected values come out the same from the builders run again."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zes.h")).read(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"^\s*int\s+(zes_[a-z0-9_]+)\s*\(", text, flags=re.M)) if "zip_batch" in n)
    assert names == ["zes_gunzip_batch_alloc", "zes_gunzip_batch_dev", "zes_gzip_batch", "zes_gzip_batch_bound", "zes_gzip_batch_dev", "zes_last_gunzip_batch"]
    assert names == sorted(list(_gzip_batch_poison.COVERS) + list(_gzip_batch_poison.EXEMPT))
    for n in names:
        assert hasattr(z.lib(), n), n
        assert (n in P.COVERS) != (n in P.EXEMPT), n
    entries = list(P.catalogue(z, oracle).values())
    for fn, patterns in _gzip_batch_poison.COVERS.items():
        for pat in patterns:
            assert any(fn in e.calls for e in P.covering(entries, pat)), (fn, pat)
    mine = [e for e in entries if any(fn in _gzip_batch_poison.COVERS for fn in e.calls)]
    again = {e.name: e for e in _gzip_batch_poison.entries(z, oracle)}
    assert len(mine) == 6 and sorted(again) == sorted(e.name for e in mine)
    for e in mine:
        assert e.want() == again[e.name].want(), e.name
    for name in ("gunzip_batch_dev both routes", "host gunzip_batch both routes"):
        verdicts, routes = again[name].want()
        assert routes == (10, 13) and sum(1 for v in verdicts if v[0] == "err") == 8 and len(verdicts) == 23
