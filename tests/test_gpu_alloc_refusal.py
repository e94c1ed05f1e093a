"""An allocator that refuses, in the three batch forms that hand their results out through zes_alloc_fn (zes_zip_read_alloc,
zes_png_decode_alloc, zes_pngwrite): an item whose allocator call returns NULL gets ZES_E_ARG and out_len 0, the call still
returns 0, and every other item comes out exactly as in a call in which nothing is refused.

Each form runs on four small items that all check out (the standard archive of tests/_zip.py has 18 entries: four of them
are selected, DEFLATE and stored), once with no refusal and then with item 0, item 2 and every item refused.  The results'
buffers are 16 bytes longer than asked for and filled with 0xA5: the bytes behind a result stay as they were."""
import ctypes as C

import numpy as np
import pytest

import _png
import _pngwrite as W
import _zip

pytestmark = pytest.mark.gpu

ZES_E_ARG = _png.ZES_E_ARG
REFUSALS = ({0}, {2}, {0, 1, 2, 3})
ZIP_SEL = [3, 6, 15, 7]  # 16 and 4096 bytes of DEFLATE, 17 bytes stored behind a descriptor bit, 5000 bytes of DEFLATE


def allocator(z, refuse):
    """-> (the callback, results by item, the calls as (item, size))."""
    got, calls = {}, []

    def alloc(_user, i, n):
        calls.append((int(i), int(n)))
        if i in refuse:
            return None
        got[i] = np.full(int(n) + 16, 0xA5, dtype=np.uint8)
        return got[i].ctypes.data

    return z.ALLOC_FN(alloc), got, calls


def refusals(what, call):
    """call(refuse) -> (rc, statuses, out_len, results, calls), for no refusal and then for every set of REFUSALS."""
    rc, status, out_len, base, calls = call(set())
    assert rc == 0 and status == [0] * 4 and all(n > 0 for n in out_len), (what, rc, status, out_len)
    assert sorted(calls) == [(i, out_len[i]) for i in range(4)], (what, calls)
    for i in range(4):
        assert base[i].size == out_len[i] + 16 and (base[i][out_len[i]:] == 0xA5).all(), (what, i)
    for refuse in REFUSALS:
        rc, status, got_len, got, calls = call(refuse)
        assert rc == 0, (what, refuse, rc)
        assert sorted(calls) == [(i, out_len[i]) for i in range(4)], (what, refuse, calls)  # once per item that checked out
        assert sorted(got) == [i for i in range(4) if i not in refuse], (what, refuse)
        for i in range(4):
            if i in refuse:
                assert (status[i], got_len[i]) == (ZES_E_ARG, 0), (what, refuse, i, status[i], got_len[i])
            else:
                assert (status[i], got_len[i]) == (0, out_len[i]), (what, refuse, i, status[i], got_len[i])
                assert got[i].tobytes() == base[i].tobytes(), (what, refuse, i)  # the result and the 0xA5 behind it
    return base, out_len


def test_zip_read_alloc(z, gpu):
    blob, plain, _ = _zip.standard()
    ent, _names = z.zip_index(blob)
    a = np.frombuffer(blob, dtype=np.uint8)
    sel = np.ascontiguousarray(ZIP_SEL, dtype=np.uint32)
    assert {int(ent[k]["method"]) for k in ZIP_SEL} == {0, 8}

    def call(refuse):
        fn, got, calls = allocator(z, refuse)
        out_len, status = (C.c_uint64 * 4)(), (C.c_int32 * 4)()
        rc = z.lib().zes_zip_read_alloc(a.ctypes.data, a.size, ent.ctypes.data, ent.size, sel.ctypes.data, 4, fn, None, out_len, status, 0)
        return rc, list(status), list(out_len), got, calls

    base, out_len = refusals("zes_zip_read_alloc", call)
    assert [base[i][:out_len[i]].tobytes() for i in range(4)] == [plain[k] for k in ZIP_SEL]


def test_png_decode_alloc(z, gpu):
    cases = sorted(_png.geometry(), key=lambda c: (len(c.want), len(c.blob)))[:4]
    arrs = [np.frombuffer(c.blob, dtype=np.uint8) for c in cases]
    ptrs = (C.c_void_p * 4)(*[x.ctypes.data for x in arrs])
    ln = np.array([x.size for x in arrs], dtype=np.uint64)

    def call(refuse):
        fn, got, calls = allocator(z, refuse)
        out_len, status = np.full(4, 77, dtype=np.uint64), np.full(4, 77, dtype=np.int32)
        info = np.zeros(4, dtype=z.PNG_INFO)
        rc = z.lib().zes_png_decode_alloc(ptrs, ln.ctypes.data, 4, fn, None, out_len.ctypes.data, status.ctypes.data, info.ctypes.data, 0)
        assert [int(r["out_size"]) for r in info] == [len(c.want) for c in cases]  # the records do not depend on the allocator
        return rc, [int(s) for s in status], [int(n) for n in out_len], got, calls

    base, out_len = refusals("zes_png_decode_alloc", call)
    assert [base[i][:out_len[i]].tobytes() for i in range(4)] == [c.want for c in cases]


def test_pngwrite(z, gpu, oracle):
    ims = W.nine()[:4]
    datas = [np.frombuffer(im.raw, dtype=np.uint8) for im in ims]
    ptrs = (C.c_void_p * 4)(*[d.ctypes.data for d in datas])
    ln = np.array([d.size for d in datas], dtype=np.uint64)
    rec = W.records(z, ims)
    aux = np.frombuffer(W.aux_of(ims) + b"\0", dtype=np.uint8)

    def call(refuse):
        fn, got, calls = allocator(z, refuse)
        out_len, status = np.full(4, 77, dtype=np.uint64), np.full(4, 77, dtype=np.int32)
        rc = z.lib().zes_pngwrite(ptrs, ln.ctypes.data, rec.ctypes.data, aux.ctypes.data, 4, fn, None, out_len.ctypes.data, status.ctypes.data, 0)
        return rc, [int(s) for s in status], [int(n) for n in out_len], got, calls

    base, out_len = refusals("zes_pngwrite", call)
    assert [base[i][:out_len[i]].tobytes() for i in range(4)] == [W.expect(im, oracle)[0] for im in ims]
