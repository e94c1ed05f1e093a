"""zes_deflate_join_dev / k_bits_place on synthetic pieces: every seam shift against every tail length, pieces shorter
than a dword, empty pieces, the grid-stride loop's second trip, the output's edges, the Adler-32 trailer and the
argument checks.  Expected streams come from tests/_bitref.py and CPython's zlib.adler32 (tests/_seam_cases.py); every
source bit beyond a piece's nbits is set, and the output starts as 0xA5 everywhere.
"""
import ctypes as C

import numpy as np
import pytest

import _seam_cases as sc

pytestmark = pytest.mark.gpu

FILL = 0xA5
NOSPACE, ARG = -16, -18


def up16(n):
    return (n + 15) // 16 * 16


def up4(n):
    return (n + 3) // 4 * 4


class Arena:
    """The pieces of many cases in 16-byte aligned slots of one device tensor, and one 0xA5-filled output tensor with a
    slot per case (the result rounded up to 16 bytes, and 32 guard bytes): one upload, one download."""

    def __init__(self, cases, gpu):
        import torch

        self.cases = cases
        self.src_off, self.out_off = [], []
        pos = 0
        for c in cases:
            offs = []
            for p in c.pieces:
                offs.append(None if p is None else pos)
                pos += 0 if p is None else up16(len(p))
            self.src_off.append(offs)
        host = np.full(max(pos, 16), 0xFF, dtype=np.uint8)
        for c, offs in zip(cases, self.src_off):
            for p, o in zip(c.pieces, offs):
                if p is not None:
                    host[o: o + len(p)] = p
        pos = 0
        for c in cases:
            self.out_off.append(pos)
            pos += up16(len(c.want)) + 32
        self.src = torch.from_numpy(host).to(gpu)
        self.out = torch.full((pos,), FILL, dtype=torch.uint8, device=gpu)
        assert self.src.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def slot(self, i):
        return self.out_off[i], (self.out_off[i + 1] if i + 1 < len(self.cases) else self.out.numel())

    def join(self, z, i, cap=None):
        c = self.cases[i]
        cnt = len(c.pieces)
        ptrs = (C.c_void_p * cnt)(*[None if o is None else self.src.data_ptr() + o for o in self.src_off[i]])
        lo, hi = self.slot(i)
        n = C.c_uint64(0xDEAD)
        rc = z.lib().zes_deflate_join_dev(ptrs, (C.c_uint64 * cnt)(*c.nbits), (C.c_uint32 * cnt)(*c.adlers), (C.c_uint64 * cnt)(*c.lens), cnt,
                                          self.out.data_ptr() + lo, (hi - lo) if cap is None else cap, C.byref(n))
        return rc, n.value

    def check(self, host_out, i):
        """All out_len bytes, zeros up to the dword's end, 0xA5 from there to the end of the slot."""
        c = self.cases[i]
        lo, hi = self.slot(i)
        got, n = host_out[lo:hi], len(c.want)
        assert got[:n].tobytes() == c.want.tobytes(), c.name
        assert not got[n: up4(n)].any(), c.name
        assert (got[up4(n):] == FILL).all(), c.name


def run_all(z, gpu, cases):
    ar = Arena(cases, gpu)
    for i, c in enumerate(cases):
        rc, n = ar.join(z, i)
        assert rc == 0 and n == len(c.want), (c.name, rc, n)
    host = ar.out.cpu().numpy()
    for i in range(len(cases)):
        ar.check(host, i)


def test_every_shift_against_every_tail(z, gpu):
    cases = sc.shift_tail_cases()
    assert len(cases) == 352
    run_all(z, gpu, cases)


def test_many_short_pieces_in_one_call(z, gpu):
    cases = sc.many_short_cases()
    assert all(len(c.pieces) == 300 for c in cases)
    run_all(z, gpu, cases)


def test_empty_pieces_and_a_single_piece(z, gpu):
    cases = sc.empty_piece_cases()
    assert any(c.pieces[0] is None for c in cases) and any(c.pieces[-1] is None for c in cases) and any(len(c.pieces) == 1 for c in cases)
    run_all(z, gpu, cases)


def test_grid_stride_wrap(z, gpu):
    """A piece above 4096 x 256 dwords: the kernel's loop goes round a second time for its last dwords."""
    c = sc.wrap_case()
    assert (c.nbits[1] + 63) // 32 > 4096 * 256 and (16 + c.nbits[0]) % 32 == 13
    run_all(z, gpu, [c])


def test_output_edges(z, gpu):
    """cap == out_len rounded up to 4 is enough and nothing behind it is touched; one byte less is ZES_E_NOSPACE with the
    length in *out_len and the buffer as it was."""
    cases = sc.edge_cases()
    assert sorted(len(c.want) % 4 for c in cases) == [0, 1, 2, 3]
    ar = Arena(cases, gpu)
    for i, c in enumerate(cases):
        rc, n = ar.join(z, i, cap=up4(len(c.want)) - 1)
        assert rc == NOSPACE and n == len(c.want), (c.name, rc, n)
    assert (ar.out.cpu().numpy() == FILL).all()
    for i, c in enumerate(cases):
        rc, n = ar.join(z, i, cap=up4(len(c.want)))
        assert rc == 0 and n == len(c.want), (c.name, rc, n)
    host = ar.out.cpu().numpy()
    for i in range(len(cases)):
        ar.check(host, i)


def test_adler_trailer(z, gpu):
    """The trailer of the device join over the lengths and contents where s1 and s2 pass the modulus, and over zero-byte
    pieces of 2^32 - 1, 2^32 + 5 and 2^40 bytes; the body is one byte per piece."""
    import torch

    lists = sc.adler_lists()
    most = max(len(parts) for _, parts, _ in lists)
    src = torch.full((16 * most,), 0x5A, dtype=torch.uint8, device=gpu)
    out = torch.full((up16(most + 6) + 16,), FILL, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    L = z.lib()
    got = {}
    for name, parts, want in lists:
        cnt = len(parts)
        n = C.c_uint64()
        rc = L.zes_deflate_join_dev((C.c_void_p * cnt)(*[src.data_ptr() + 16 * k for k in range(cnt)]), (C.c_uint64 * cnt)(*[8] * cnt),
                                    (C.c_uint32 * cnt)(*[a for a, _ in parts]), (C.c_uint64 * cnt)(*[ln for _, ln in parts]), cnt,
                                    out.data_ptr(), out.numel(), C.byref(n))
        assert rc == 0 and n.value == cnt + 6, name
        h = out[: n.value].cpu().numpy()
        assert h[:2].tolist() == [0x78, 0x9C] and (h[2: 2 + cnt] == 0x5A).all(), name
        got[name] = int.from_bytes(h[-4:].tobytes(), "big")
    bad = [(name, hex(got[name]), hex(want)) for name, _, want in lists if got[name] != want]
    assert not bad, bad[:5]


def test_argument_errors(z, gpu):
    import torch

    src = torch.zeros(64, dtype=torch.uint8, device=gpu)
    out = torch.full((64,), FILL, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    L = z.lib()
    n = C.c_uint64()
    one = lambda v, t=C.c_uint64: (t * 1)(v)
    good = ((C.c_void_p * 1)(src.data_ptr()), one(20), one(1, C.c_uint32), one(0))
    assert L.zes_deflate_join_dev(*good, 1, out.data_ptr(), 64, C.byref(n)) == 0  # (the calls below differ from this one in one thing)
    out.fill_(FILL)
    torch.cuda.synchronize()
    assert L.zes_deflate_join_dev(*good, 0, out.data_ptr(), 64, C.byref(n)) == ARG
    assert L.zes_deflate_join_dev(None, good[1], good[2], good[3], 1, out.data_ptr(), 64, C.byref(n)) == ARG
    for k in (1, 4, 8, 15):
        assert L.zes_deflate_join_dev(*good, 1, out.data_ptr() + k, 48, C.byref(n)) == ARG, k
    for k in (1, 2, 3):
        assert L.zes_deflate_join_dev((C.c_void_p * 1)(src.data_ptr() + k), good[1], good[2], good[3], 1, out.data_ptr(), 64, C.byref(n)) == ARG, k
    assert L.zes_deflate_join_dev((C.c_void_p * 1)(None), good[1], good[2], good[3], 1, out.data_ptr(), 64, C.byref(n)) == ARG
    # a misaligned or null pointer of a piece without bits is never read (include/zes.h allows it)
    two = ((C.c_void_p * 2)(src.data_ptr() + 1, src.data_ptr()), (C.c_uint64 * 2)(0, 20), (C.c_uint32 * 2)(1, 1), (C.c_uint64 * 2)(0, 0))
    assert L.zes_deflate_join_dev(*two, 2, out.data_ptr(), 64, C.byref(n)) == 0 and n.value == 2 + 3 + 4
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert h[:9].tolist() == [0x78, 0x9C, 0, 0, 0, 0, 0, 0, 1] and not h[9:12].any() and (h[12:] == FILL).all()
