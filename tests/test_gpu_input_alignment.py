"""The deflate kernels' unaligned-input paths, on every route of the encoder.

include/zes.h lets the deflate device forms read their input at any alignment; the kernels then leave their 16-byte loads
for fallbacks of their own: k_lz_sort (sort_ld16 in four filter passes, stage_block), k_lz_index (idx_ld20), k_lz_match and
k_lz_match_lazy (the block and its 258-byte halo staged dword by dword from bytes, bounded by `avail`) and adler_chunk
(k_adler, k_adler_blocks: the one-load loop for a whole chunk).  Here every input of tests/_encoder_cases.py — one per sort,
index, match and parse route and per rule of the reference's encoder — meets every misalignment 1..15, standing between
the surroundings of tests/_align_cases.py: a copy of its own first bytes in front, and behind it a run of its last byte or
its last period, so that a fallback that starts at the rounded-down address or reads past the input's end computes
something else (tests/test_align_cases_cpu.py shows that with the oracle).  Every pointer handed over lies inside such an
array, FRONT + a bytes behind its first byte and BEHIND bytes in front of its end: nothing here reads outside a live
tensor, and nothing is meant to fault.

Everything is bit-exact: tokens and the route record against the oracle and the case's expected route (a route is a
function of the bytes alone: it must not move with the address), whole streams against the hashes recorded from the
reference (tests/golden/encoder_cases.json)."""
import ctypes as C
import hashlib
import struct
import zlib

import numpy as np
import pytest

import _align_cases as al
import _encoder_cases as ec
from conftest import golden
from test_gpu_encoder_cases import same_tokens, want_tokens

pytestmark = pytest.mark.gpu
GOLD = golden("encoder_cases.json")
NAMES = sorted(GOLD)
CANARY = 64
GZIP_HEADER = bytes.fromhex("1f8b08000000000000ff")
_STREAMS = {}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def up16(n):
    return (n + 15) // 16 * 16


@pytest.fixture(scope="module")
def cases(z):
    return ec.cases(z)


def period_of(oracle, cases, name):
    """The "period" fill's distance: that of the last match in the oracle's tokens of the input's last block."""
    d = cases[name].data
    return al.last_match_dist(want_tokens(oracle, cases, name, (d.size - 1) // ec.BLK * ec.BLK))


def upload(gpu, d, a, fill, dist):
    """front || d || behind on the GPU -> (tensor, byte of d's first byte); the tensor starts on a 16-byte boundary."""
    import torch

    arr, at = al.surround(d, a, fill, dist)
    t = torch.from_numpy(arr).to(gpu)
    assert t.data_ptr() % 16 == 0 and (t.data_ptr() + at) % 16 == a
    assert at >= al.FRONT and t.numel() - (at + d.size) >= al.BEHIND
    return t, at


def want_stream(oracle, cases, name):
    """The reference's zlib stream of a case: the oracle's bytes, which must be the recorded ones (once per case)."""
    if name not in _STREAMS:
        comp = oracle.deflate(cases[name].data)
        assert (comp.size, _sha(comp)) == (GOLD[name]["deflate_len"], GOLD[name]["deflate_sha256"])
        _STREAMS[name] = comp.tobytes()
    return _STREAMS[name]


def dev_call(z, gpu, fn, t, at, n, cap):
    """fn(d_in = t + at, n, d_out, cap, &out_len) with d_out a 16-byte aligned slot of `cap` bytes (a multiple of 16) that
    has CANARY bytes behind it, all 0xA5 -> (status, the result's bytes).  The library writes whole 16-byte groups: the
    bytes behind the result rounded up to 16 must be intact, the slot's own and the ones behind the slot."""
    import torch

    assert cap % 16 == 0 and 0 < at and at + n < t.numel()
    buf = torch.full((cap + CANARY,), 0xA5, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    m = C.c_uint64()
    rc = fn(t.data_ptr() + at, n, buf.data_ptr(), cap, C.byref(m))
    h = buf.cpu().numpy()
    assert rc != 0 or m.value <= cap
    assert (h[up16(m.value) if rc == 0 else cap:] == 0xA5).all(), "bytes behind the rounded-up result changed"
    return rc, h[: m.value].tobytes() if rc == 0 else b""


# a ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_stage(name, z, oracle, cases, gpu):
    """The case's block (every block of the multi-block cases) through the stage entry at every misalignment and with both
    fills behind it: the oracle's tokens, the route the case was built for, and the same record at every address (a = 0
    comes first: the record of the aligned loads is what the others are held against)."""
    k = cases[name]
    n = k.data.size
    dist = period_of(oracle, cases, name)
    starts = list(range(0, n, ec.BLK)) if n > ec.BLK else [k.start]
    records = {}
    for a in range(16):
        for fill in al.FILLS:
            t, at = upload(gpu, k.data, a, fill, dist)
            view = t[at: at + n]
            assert view.data_ptr() % 16 == a and view.numel() == n
            for start in starts:
                what = "%s, block at %d, input at 16 k + %d, %s behind it" % (name, start, a, fill)
                length = min(ec.BLK, n - start)
                tok = z.stage_lz77_tensor(view, start, length)
                words = z.stage_lz77_route()
                same_tokens(tok, want_tokens(oracle, cases, name, start), what)
                route = ec.decode_route(words, length)
                assert route["ntok"] == tok.size, what
                if start == k.start:
                    assert ec.route_matches(route, k.route), "%s took %r, built for %r" % (what, route, k.route)
                first = records.setdefault(start, (what, words))
                assert (words == first[1]).all(), "%s: %r, but %s: %r" % (what, list(words), first[0], list(first[1]))


# b ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_whole_stream(name, z, oracle, cases, gpu):
    """zes_deflate_dev with d_in at every misalignment: the reference's stream (Adler-32 trailer included: k_adler_blocks on
    an unaligned buffer; block_border and mixed_four_blocks: the halo into the next block, blocks of different routes in one
    launch).  At 1 and 15 also the raw and the gzip form."""
    k = cases[name]
    n = k.data.size
    dist = period_of(oracle, cases, name)
    want = want_stream(oracle, cases, name)
    gz = GZIP_HEADER + want[2:-4] + struct.pack("<II", zlib.crc32(k.data.tobytes()), n & 0xFFFFFFFF)
    for a in range(1, 16):
        t, at = upload(gpu, k.data, a, al.FILLS[a % 2], dist)
        rc, got = dev_call(z, gpu, z.lib().zes_deflate_dev, t, at, n, up16(z.deflate_bound(n)))
        assert rc == 0, (name, a)
        assert (len(got), _sha(np.frombuffer(got, dtype=np.uint8))) == (GOLD[name]["deflate_len"], GOLD[name]["deflate_sha256"]), \
            "%s, input at 16 k + %d: not the reference's stream" % (name, a)
        if a in (1, 15):
            rc, got = dev_call(z, gpu, z.lib().zes_deflate_raw_dev, t, at, n, up16(z.deflate_bound(n)))
            assert rc == 0 and got == want[2:-4], "%s, input at 16 k + %d: the raw form" % (name, a)
            rc, got = dev_call(z, gpu, z.lib().zes_gzip_dev, t, at, n, up16(z.gzip_bound(n)))
            assert rc == 0 and got[:10] == gz[:10] and got[10:-8] == gz[10:-8], "%s, input at 16 k + %d: gzip header or body" % (name, a)
            assert got[-8:] == gz[-8:], "%s, input at 16 k + %d: gzip CRC-32 or ISIZE" % (name, a)


# c ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", range(16))
def test_one_batch_mixed_alignments(r, z, oracle, cases, gpu):
    """All one-block cases in one zes_deflate_batch_dev call, buffer i at in_off[i] % 16 == (5 i + r) % 16: aligned and
    unaligned blocks of every route side by side in each launch; over the sixteen rotations every case meets every
    misalignment once.  run_to_end stands directly in front of run_crossing, as in test_one_batch."""
    import torch

    names = [n for n in NAMES if cases[n].data.size <= ec.BLK]
    names.remove("run_crossing")
    names.insert(names.index("run_to_end") + 1, "run_crossing")
    assert len(names) == 44
    mis = [(5 * i + r) % 16 for i in range(len(names))]
    arena, in_off = al.arena([(cases[n].data, a, al.FILLS[(i + r) % 2], period_of(oracle, cases, n)) for i, (n, a) in enumerate(zip(names, mis))])
    lens = [cases[n].data.size for n in names]
    assert [o % 16 for o in in_off] == mis
    assert all(o >= al.FRONT and o + ln + al.BEHIND <= arena.size for o, ln in zip(in_off, lens))
    caps = [z.deflate_bound(ln) for ln in lens]
    out_off = [int(x) for x in np.cumsum([0] + [up16(c) for c in caps])]
    out = torch.full((out_off[-1] + CANARY,), 0xA5, dtype=torch.uint8, device=gpu)
    assert out.data_ptr() % 16 == 0 and all(o % 16 == 0 for o in out_off)
    olen, st = z.deflate_batch_tensor(torch.from_numpy(arena).to(gpu), in_off, lens, out, out_off[:-1], caps)
    host = out.cpu().numpy()
    assert (host[out_off[-1]:] == 0xA5).all()
    for n, a, off, ln, s in zip(names, mis, out_off, olen, st):
        assert s == 0, (n, a)
        assert (int(ln), _sha(host[off: off + int(ln)])) == (GOLD[n]["deflate_len"], GOLD[n]["deflate_sha256"]), \
            "%s at 16 k + %d: not the reference's stream" % (n, a)


# d ------------------------------------------------------------------------------------------------
ADLER_LENGTHS = (1, 15, 16, 17, 16383, 16384, 16385, 65535, 65536, 65537, 3 * 65536 + 5)


@pytest.fixture(scope="module")
def adler_data(z, gpu):
    """kind -> (host array, tensor): FRONT + 15 bytes, the longest input and BEHIND bytes; what stands around an input is the
    array's own other bytes (the 0xFF array: 0x5A in front and behind)."""
    import torch

    size = al.FRONT + 16 + max(ADLER_LENGTHS) + al.BEHIND
    ff = np.full(size, 0x5A, dtype=np.uint8)
    ff[al.FRONT: al.FRONT + 15 + max(ADLER_LENGTHS)] = 0xFF
    host = {"xorshift": z.gen("xorshift", 515, size), "ff": ff}
    return {kind: (h, torch.from_numpy(h.copy()).to(gpu)) for kind, h in host.items()}


@pytest.mark.parametrize("n", ADLER_LENGTHS)
def test_adler32_dev_at_every_address(n, z, oracle, gpu, adler_data):
    """zes_adler32_dev (k_adler) at the round and chunk seams of adler_chunk, from every address 16 k + a: a = 0 takes the
    four-loads-in-flight rounds, every other a the one-load loop."""
    import torch

    torch.cuda.synchronize()
    for kind, (h, t) in adler_data.items():
        assert t.data_ptr() % 16 == 0
        for a in range(16):
            # (the 0xFF bytes begin at FRONT: an input of them starts at FRONT + a and stays inside them whatever a is)
            at = al.FRONT + a
            assert at + n + al.BEHIND <= t.numel()
            data = h[at: at + n]
            assert kind != "ff" or (data == 0xFF).all()
            got = C.c_uint32()
            assert z.lib().zes_adler32_dev(t.data_ptr() + at, n, C.byref(got)) == 0
            assert got.value == oracle.adler32(data), (kind, n, a)


# range form ---------------------------------------------------------------------------------------
def test_range_form_asks_for_an_aligned_input(z, oracle, cases, gpu):
    """zes_deflate_range_dev is the one deflate device form that does not take an unaligned d_in (include/zes.h): ZES_E_ARG,
    decided on the host before any launch; the same bytes from an aligned address go through."""
    import torch

    d = cases["text_short"].data
    cap = up16(z.deflate_bound(d.size))
    out = torch.zeros(cap, dtype=torch.uint8, device=gpu)
    bits, ad = C.c_uint64(), C.c_uint32()
    for a in range(1, 16):
        t, at = upload(gpu, d, a, "run", 1)
        assert z.lib().zes_deflate_range_dev(t.data_ptr() + at, d.size, d.size, 1, out.data_ptr(), cap, C.byref(bits), C.byref(ad)) == z.ZES_E_ARG, a
    t, at = upload(gpu, d, 0, "run", 1)
    torch.cuda.synchronize()
    assert z.lib().zes_deflate_range_dev(t.data_ptr() + at, d.size, d.size, 1, out.data_ptr(), cap, C.byref(bits), C.byref(ad)) == 0
    raw = want_stream(oracle, cases, "text_short")[2:-4]
    assert (bits.value + 7) // 8 == len(raw) and out.cpu().numpy()[: len(raw)].tobytes() == raw and ad.value == oracle.adler32(d)
