"""zes_deflate_range_dev and zes_inflate_range_dev at their seams: block ranges whose matches run up to the boundary, the
258-byte halo, and bit ranges whose lo_bit / own_bit sit on a block start and one bit to either side of it, pieces
aligned every possible way under the range, pieces that end early, short capacities, damaged blocks.

Expected values come from the oracle alone (tests/_range_cases.py): oracle.deflate_range for the encoder, the map of
oracle.inflate_blocks and the header's half-open rule (blocks with lo_bit <= start < own_bit) for the decoder.  The C
entry points are called directly, so the test chooses the piece; outputs are poisoned, with a guard behind cap.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import _range_cases as rc
import _seam_cases as sc

pytestmark = pytest.mark.gpu

BLOCK = rc.BLOCK
POISON = 0xC3
GUARD = BLOCK
OK, CORRUPT, NOSPACE, ARG, NOTRANGE = 0, -3, -16, -18, -19


def to_dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# =====================================================================================================================
# zes_deflate_range_dev
# =====================================================================================================================
class Deflater:
    def __init__(self, z, gpu, a):
        import torch

        self.z, self.a, self.t = z, a, to_dev(a, gpu)
        self.out = torch.empty(z.deflate_bound(2 * BLOCK) + GUARD, dtype=torch.uint8, device=gpu)
        assert self.t.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0

    def run(self, lo, n, final, readable=None, cap=None, t=None):
        """-> (rc, bits or the capacity needed, adler)"""
        import torch

        t = self.t if t is None else t
        self.out.fill_(POISON)
        torch.cuda.synchronize()
        cap = self.z.deflate_bound(n) if cap is None else cap
        readable = min(t.numel() - lo, n + 258) if readable is None else readable
        bits, ad = C.c_uint64(0), C.c_uint32(0)
        rc = self.z.lib().zes_deflate_range_dev(t.data_ptr() + lo, n, readable, 1 if final else 0, self.out.data_ptr(), cap, C.byref(bits), C.byref(ad))
        self.cap = cap
        return rc, bits.value, ad.value

    def piece(self, bits):
        return self.out[: (bits + 7) // 8].cpu().numpy()

    def guard_intact(self):
        return bool((self.out[self.cap:] == POISON).all())


@pytest.mark.parametrize("name", rc.DEFLATE_INPUTS)
def test_deflate_ranges_equal_the_oracles(z, oracle, gpu, name):
    """Every single-block range and every two-block range: the oracle's piece, bit count and CPython's Adler-32; the
    single-block pieces joined are oracle.deflate of the whole."""
    a = rc.deflate_input(z, name)
    n = len(a)
    d = Deflater(z, gpu, a)
    nblk = (n + BLOCK - 1) // BLOCK
    singles = []
    for width in (1, 2):
        for b in range(nblk - width + 1):
            lo, hi = b * BLOCK, min(n, (b + width) * BLOCK)
            rcode, bits, ad = d.run(lo, hi - lo, hi == n)
            want, want_bits = oracle.deflate_range(a, lo, hi - lo, hi == n)
            assert rcode == OK and bits == want_bits, (name, b, width, rcode, bits, want_bits)
            assert d.piece(bits).tobytes() == want.tobytes(), (name, b, width)
            assert ad == zlib.adler32(a[lo:hi].tobytes()), (name, b, width)
            assert d.guard_intact()
            if width == 1:
                singles.append((d.out[: (bits + 7) // 8 + 8].clone(), bits, ad, hi - lo))
    got = z.deflate_join_tensors([s[0] for s in singles], [s[1] for s in singles], [s[2] for s in singles], [s[3] for s in singles])
    assert got.cpu().numpy().tobytes() == oracle.deflate(a).tobytes(), name


@pytest.mark.parametrize("name", ("period258", "period259", "one_byte"))
def test_deflate_range_reads_its_halo_and_no_further(z, oracle, gpu, name):
    a = rc.deflate_input(z, name)
    n = len(a)
    d = Deflater(z, gpu, a)
    for lo, ln in ((0, BLOCK), (BLOCK, BLOCK), (BLOCK, 2 * BLOCK)):
        want, want_bits = oracle.deflate_range(a, lo, ln, False)
        # n_readable == n + 258 exactly
        rcode, bits, _ = d.run(lo, ln, False, readable=ln + 258)
        assert rcode == OK and bits == want_bits and d.piece(bits).tobytes() == want.tobytes(), (name, lo, ln)
        # a copy that differs from byte lo + n + 258 on: the same piece, bit for bit
        b = a.copy()
        b[lo + ln + 258:] ^= 0x5C
        rcode, bits2, _ = d.run(lo, ln, False, readable=ln + 258, t=to_dev(b, gpu))
        assert rcode == OK and bits2 == want_bits and d.piece(bits2).tobytes() == want.tobytes(), (name, lo, ln)
        # ... and other bytes inside the halo: whatever the oracle makes of them
        b = a.copy()
        b[lo + ln + 100: lo + ln + 258] ^= 0x5C
        want_b, want_b_bits = oracle.deflate_range(b, lo, ln, False)
        rcode, bits3, _ = d.run(lo, ln, False, readable=ln + 258, t=to_dev(b, gpu))
        assert rcode == OK and bits3 == want_b_bits and d.piece(bits3).tobytes() == want_b.tobytes(), (name, lo, ln)
    # the final range at the very end of its tensor, n_readable == n
    lo = 3 * BLOCK
    want, want_bits = oracle.deflate_range(a, lo, n - lo, True)
    rcode, bits, ad = d.run(lo, n - lo, True, readable=n - lo)
    assert rcode == OK and bits == want_bits and d.piece(bits).tobytes() == want.tobytes() and ad == zlib.adler32(a[lo:].tobytes())


def test_deflate_range_refusals(z, gpu):
    a = rc.deflate_input(z, "lowent4k")
    d = Deflater(z, gpu, a)
    assert d.run(0, BLOCK + 5, False)[0] == ARG  # only the last range may end inside a block
    assert d.run(0, BLOCK - 1, False)[0] == ARG
    assert d.run(0, BLOCK, False, readable=BLOCK - 1)[0] == ARG
    assert d.run(BLOCK, BLOCK + 777, True, readable=BLOCK + 776)[0] == ARG
    assert d.run(0, BLOCK + 1, True)[0] == CORRUPT  # the reference throws on a 1-byte last block
    assert d.run(BLOCK, 1, True)[0] == CORRUPT
    assert d.guard_intact() and bool((d.out == POISON).all())
    for n, final in ((BLOCK, False), (777, True), (2 * BLOCK, False)):
        need = z.deflate_bound(n)
        rcode, bits, _ = d.run(3 * BLOCK if final else 0, n, final, cap=need - 1)
        assert rcode == NOSPACE and bits == need, (n, rcode, bits, need)
        assert bool((d.out == POISON).all())  # nothing written at all, behind cap or in front of it
        assert d.run(3 * BLOCK if final else 0, n, final, cap=need)[0] == OK and d.guard_intact()


# =====================================================================================================================
# zes_inflate_range_dev
# =====================================================================================================================
class Ranger:
    """One stream on the device (4 KiB of other bytes behind it), its plain bytes, and a poisoned output of cap + GUARD."""

    def __init__(self, z, gpu, s, comp=None):
        import torch

        self.z, self.s = z, s
        self.comp = s.comp if comp is None else comp
        self.t = to_dev(np.concatenate([self.comp, np.full(4096, 0xEE, dtype=np.uint8)]), gpu)
        self.a = to_dev(s.a, gpu)
        self.cap = len(s.starts) * BLOCK
        self.out = torch.empty(self.cap + GUARD, dtype=torch.uint8, device=gpu)
        assert self.t.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0

    def byte0(self, lo):
        b = (lo >> 3) & ~15  # the largest 16-byte aligned start that keeps lo_bit - 8 * byte0 >= 16
        return b - 16 if (lo - 8 * b) < 16 else b

    def call(self, lo, own, exact, byte0=None, end=None, cap=None):
        """The call over stream bits [lo, own) on the piece comp[byte0:end] -> (rc, results in stream coordinates)."""
        import torch

        byte0 = self.byte0(lo) if byte0 is None else byte0
        end = len(self.comp) if end is None else end
        self.used_cap = self.cap if cap is None else cap
        self.out.fill_(POISON)
        torch.cuda.synchronize()
        n, fb, eb, nb, fin = C.c_uint64(77), C.c_uint64(77), C.c_uint64(77), C.c_uint32(77), C.c_int32(77)
        rcode = self.z.lib().zes_inflate_range_dev(self.t.data_ptr() + byte0, end - byte0, lo - 8 * byte0, own - 8 * byte0, 1 if exact else 0,
                                                 self.out.data_ptr(), self.used_cap, C.byref(n), C.byref(fb), C.byref(eb), C.byref(nb), C.byref(fin))
        return rcode, {"out_len": n.value, "first_bit": fb.value + 8 * byte0, "end_bit": eb.value + 8 * byte0, "nblocks": nb.value, "final": fin.value}

    def check(self, got, want, what):
        """want: Stream.expect's record, or None for ZES_E_NOTRANGE."""
        import torch

        rcode, res = got
        cap = self.used_cap
        assert bool((self.out[cap:] == POISON).all()), ("guard behind cap", what)
        if want is None:
            assert rcode == NOTRANGE, (what, rcode, res)
            return
        assert rcode == (NOSPACE if want["out_len"] > cap else OK), (what, rcode, res, want)
        for key in ("out_len", "first_bit", "end_bit", "nblocks", "final"):
            assert res[key] == want[key], (what, key, res, want)
        if rcode == OK:
            n = want["out_len"]
            assert torch.equal(self.out[:n], self.a[want["out_lo"]: want["out_lo"] + n]), ("bytes", what)
            assert bool((self.out[n:] == POISON).all()), ("behind out_len", what)

    def run(self, lo, own, exact, what, **kw):
        self.check(self.call(lo, own, exact, **kw), self.s.expect(lo, own, exact), (self.s.kind, what, lo, own, exact))


@pytest.fixture(scope="module")
def rangers(z, oracle, gpu):
    return {kind: Ranger(z, gpu, rc.range_stream(z, oracle, kind)) for kind in rc.RANGE_STREAMS}


KINDS = sorted(rc.RANGE_STREAMS)


@pytest.mark.parametrize("kind", KINDS)
def test_lo_bit_and_own_bit_on_every_block_start(rangers, kind):
    r = rangers[kind]
    st, nb, stream_end = r.s.starts, len(r.s.starts), 8 * len(r.s.comp)
    calls = 0
    for k in range(1, nb):
        s = st[k]
        own = st[k + 2] if k + 2 < nb else stream_end  # two blocks, or what is left
        lo = st[max(k - 2, 0)]
        r.run(s, own, True, "lo on the start, exact")          # first own block: k
        r.run(s, own, False, "lo on the start, searched")      # first own block: k
        r.run(s + 1, own, False, "lo one bit behind")          # first own block: k + 1 (none, for the final block)
        r.run(s + 1, own, True, "lo one bit behind, exact")    # ZES_E_NOTRANGE
        r.run(lo, s, True, "own on the start")                 # block k is not owned: end_bit == s
        r.run(lo, s + 1, True, "own one bit behind")           # block k is owned
        calls += 6
        assert r.s.expect(s, own, True)["first_bit"] == s and r.s.expect(s + 1, own, True) is None
        assert r.s.expect(lo, s, True)["end_bit"] == s and r.s.expect(lo, s + 1, True)["nblocks"] == r.s.expect(lo, s, True)["nblocks"] + 1
    assert calls == 6 * (nb - 1)


def test_range_without_a_block_start(z, rangers):
    """lo = s_k + 1, own = s_(k+1): ZES_OK, no blocks, no bytes, output untouched, first_bit == end_bit == lo_bit — whether
    the kernel finds no own candidate (the whole rest of the stream as the piece), the search finds none at all (the piece
    ends with the range) or the piece is too short to be searched (c * 8 < lo_bit + 64).  The same through the wrapper."""
    import torch

    r = rangers["xorshift"]
    st = r.s.starts
    for k in range(len(st) - 1):
        lo, own = st[k] + 1, st[k + 1]
        want = r.s.expect(lo, own, False)
        assert want["nblocks"] == 0 and want["first_bit"] == want["end_bit"] == lo
        r.run(lo, own, False, "empty, long piece")
        r.run(lo, own, False, "empty, piece ends with the range", end=(own + 7) // 8)
        b0 = r.byte0(lo)
        short = b0 + (lo - 8 * b0 + 63) // 8
        assert (short - b0) * 8 < lo - 8 * b0 + 64
        r.run(lo, own, False, "empty, piece too short to search", end=short)
        r.check(r.call(lo, own, True, end=short), None, "exact start on a piece too short to search")
        r.out.fill_(POISON)
        torch.cuda.synchronize()
        assert z.inflate_range_tensor(r.t[: len(r.s.comp)], lo, own, False, r.out) == (0, lo, lo, 0, False), k
        assert bool((r.out == POISON).all())


@pytest.mark.parametrize("kind", KINDS)
def test_piece_alignment(rangers, kind):
    """Every 16-byte aligned piece start from the closest one down to 256 bytes below it: the same results in stream
    coordinates (for lowent4k the lower ones put real block starts in front of lo_bit, inside the piece)."""
    r = rangers[kind]
    st = r.s.starts
    mid = (st[1] + st[2]) // 2
    for lo, own, exact in ((st[2], st[4] + 1, True), (mid, st[4], False)):
        top = r.byte0(lo)
        assert lo - 8 * top >= 16 and lo - 8 * (top + 16) < 16
        for b0 in range(top, top - 257, -16):
            r.run(lo, own, exact, "byte0 = top - %d" % (top - b0), byte0=b0)


@pytest.mark.parametrize("kind", KINDS)
def test_piece_end(rangers, kind):
    r = rangers[kind]
    st, nb = r.s.starts, len(r.s.starts)
    lo, own = st[1], st[3]  # blocks 1 and 2, neither final
    # as documented: the range, the last own block to its end, the header of the block behind it (below 1 KiB)
    r.run(lo, own, True, "documented piece", end=st[3] // 8 + 1024)
    r.run(lo, own - 7, True, "documented piece, own inside block 2", end=st[3] // 8 + 1024)
    # the piece stops with the last byte of block 2: the block behind it cannot be seen, so the chain of own blocks has
    # nothing to end on — refused, never other values
    last_byte = (st[3] - 1) // 8
    got = r.call(lo, own, True, end=last_byte + 1)
    assert got[0] == NOTRANGE, (kind, got)
    r.check(got, None, "piece ends with its last own block")
    # the final range, fed up to the Adler-32 trailer
    end = len(r.s.comp) - 4
    for lo2, exact in ((st[nb - 2], True), (st[nb - 1], True), (st[nb - 2] + 1, False)):
        want = r.s.expect(lo2, 8 * end, exact)
        assert want["final"] == 1 and want["end_bit"] == r.s.end_bit
        r.run(lo2, 8 * end, exact, "final range up to the trailer", end=end)


@pytest.mark.parametrize("kind", KINDS)
def test_capacity(rangers, kind):
    r = rangers[kind]
    st, nb, stream_end = r.s.starts, len(r.s.starts), 8 * len(r.s.comp)
    for lo, own, what in ((st[1], st[3], "whole blocks"), (st[nb - 1], stream_end, "the final block"), (st[nb - 3], stream_end, "blocks and the final one")):
        n = r.s.expect(lo, own, True)["out_len"]
        r.run(lo, own, True, what + ", cap == out_len", cap=n)
        got = r.call(lo, own, True, cap=n - 1)
        assert got[0] == NOSPACE and got[1]["out_len"] == n, (kind, what, got)
        r.check(got, r.s.expect(lo, own, True), what + ", cap == out_len - 1")


@pytest.mark.parametrize("kind", KINDS)
def test_damaged_block(z, oracle, gpu, rangers, kind):
    """One flipped bit in the body of block k (positions and oracle outcomes: tests/_range_cases.py).  Ranges that own only
    blocks before k give the map's values, every range that owns k is refused, and z.inflate of the whole damaged stream
    is the oracle's answer."""
    s = rangers[kind].s
    st, nb, stream_end = s.starts, len(s.starts), 8 * len(s.comp)
    for k, bit, want in rc.RANGE_FLIPS[kind]:
        bad = rc.flip(s.comp, bit)
        r = Ranger(z, gpu, s, comp=bad)
        for j in range(k):
            r.run(st[j], st[j + 1], True, ("flip", bit, "block", j))
        r.run(16, st[k], True, ("flip", bit, "all blocks before", k))
        if k >= 2:
            r.run(st[k - 2] + 1, st[k], False, ("flip", bit, "searched, the block before", k))
        for lo, own, exact in ((st[k], st[k + 1], True), (st[k], st[k] + 1, True), (st[k - 1], st[k + 1], True), (st[k - 1] + 1, st[k + 1], False),
                               (st[k], stream_end, True), (16, stream_end, True), (16, st[k] + 1, True)):
            assert k in s.owned(lo, own)
            r.check(r.call(lo, own, exact), None, (kind, "flip", bit, "a range that owns block", k, lo, own))
        got, want_bytes = rc.outcome(oracle, bad)
        assert got == want
        try:
            mine = z.inflate(bad)
            assert want_bytes is not None and mine.tobytes() == want_bytes.tobytes(), (kind, bit)
        except z.ZlibEsError as e:
            assert want == ("err", e.code), (kind, bit, e.code)


def test_range_refusals(rangers):
    r = rangers["itext"]
    L = r.z.lib()
    st = r.s.starts
    outs = [C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_int32()]
    refs = [C.byref(x) for x in outs]
    d_in, c, d_out, cap = r.t.data_ptr(), len(r.s.comp), r.out.data_ptr(), r.cap
    assert L.zes_inflate_range_dev(d_in, c, 16, st[1], 1, d_out, cap, *refs) == OK  # (the calls below differ from this one in one thing)
    assert L.zes_inflate_range_dev(d_in, c, 15, st[1], 1, d_out, cap, *refs) == ARG
    assert L.zes_inflate_range_dev(d_in, c, 0, st[1], 0, d_out, cap, *refs) == ARG
    assert L.zes_inflate_range_dev(d_in, c, st[1], st[1], 1, d_out, cap, *refs) == ARG
    assert L.zes_inflate_range_dev(d_in, c, st[1], st[1] - 1, 1, d_out, cap, *refs) == ARG
    for k in (1, 4, 8):
        assert L.zes_inflate_range_dev(d_in + k, c - k, 16 + 8 * (16 - k), st[1], 0, d_out, cap, *refs) == ARG, k
        assert L.zes_inflate_range_dev(d_in, c, 16, st[1], 1, d_out + k, cap - 16, *refs) == ARG, k
    assert L.zes_inflate_range_dev(d_in, 1 << 29, 16, st[1], 1, d_out, cap, *refs) == ARG  # (refused before anything is read)


@pytest.mark.parametrize("kind,seed", [("itext", 1093), ("xorshift", 1025)])
def test_streams_with_a_header_lookalike_inside_a_block(z, oracle, gpu, kind, seed):
    """The two 1 MiB inputs whose streams hold a valid-looking dynamic header in the middle of a block, through four
    ranges each: the default search drops the lookalike (it breaks the reference's run-length rules), so every range
    gives the map's values and the outputs concatenate to the input."""
    import torch

    shard = sc.load_shard()
    s = rc.Stream(z, oracle, kind, seed, 1 << 20)
    t = to_dev(s.comp, gpu)
    table, outs = [], []
    for rank, (lo, own) in enumerate(shard.split_bits(len(s.comp), 4)):
        out = torch.full((len(s.a) + BLOCK,), POISON, dtype=torch.uint8, device=gpu)
        res = z.inflate_range_tensor(t, lo, own, rank == 0, out)
        want = s.expect(max(lo, 16), own, rank == 0)
        assert res is not None and want is not None, (kind, rank)
        assert res == (want["out_len"], want["first_bit"], want["end_bit"], want["nblocks"], bool(want["final"])), (kind, rank, res, want)
        table.append([1, res[1], res[2], res[3], res[0], int(res[4])])
        outs.append(out[: res[0]])
    assert shard.check_chain(table)
    assert torch.cat(outs).cpu().numpy().tobytes() == s.a.tobytes()


def test_whole_stream_whose_final_block_ends_with_the_buffer(z, gpu, rangers):
    """zes_inflate_dev of the xorshift stream without its Adler-32 trailer (the reference ignores the trailer,
    src/zlib.ts:11-23): the 2-byte final block ends two bits in front of the buffer's end.  The block-start search of
    every tier asks each code-length symbol of a header for its own bits only, not for 14 bits of data behind it, so the
    block is found and the stream stays in the block-parallel tier."""
    import torch

    s = rangers["xorshift"].s
    assert 8 * (len(s.comp) - 4) - s.end_bit < 14
    t = to_dev(s.comp[:-4], gpu)
    out = torch.full((s.n + 16,), POISON, dtype=torch.uint8, device=gpu)
    back = z.inflate_tensor(t, out)
    assert back.numel() == s.n and torch.equal(back, rangers["xorshift"].a) and bool((out[s.n:] == POISON).all())
    assert z.last_inflate_tier() == 1
