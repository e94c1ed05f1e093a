"""The position form of match-poor blocks on the inputs of tests/_poor_cases.py: block lengths at the seams of a lane's
group, a wave's run, the tile and the block; matches at those seams, back to back, covered, longest, shortest, nearest,
farthest; a full match list and one match more; blocks of this route beside the lazy matcher's.

Every case goes through zes_deflate_dev with its input at 16 k + 0, 1, 2 and 3 (the kernels read the input in aligned
words from the word its first byte lies in) and must be the oracle's stream, its length and every byte; zes_inflate_dev of
that gives the input back; and the stage entry's route record shows that every block went where the case says.  The batch
form takes several cases in one call, the range form two and three pieces of one input, joined.

(A range piece that starts inside a byte of its output, ZES_BUF_CONT, is made by the pipelined host call alone, from
48 MiB on: tests/test_gpu_configs.py::test_pipelined_host_calls runs it on random bytes.)"""
import ctypes as C

import numpy as np
import pytest

import _encoder_cases as ec
import _poor_cases as pc

pytestmark = pytest.mark.gpu
BLK = pc.BLK
NAMES = pc.NAMES
FRONT, BEHIND = 16, 320
_WANT = {}


@pytest.fixture(scope="module")
def cases(z):
    c = pc.cases(z)
    assert sorted(c) == NAMES
    return c


def want(oracle, cases, name):
    """The oracle's stream of a case (computed once, shared, never changed)."""
    if name not in _WANT:
        w = oracle.deflate(cases[name].data)
        w.setflags(write=False)
        _WANT[name] = w
    return _WANT[name]


def up16(n):
    return (n + 15) // 16 * 16


def same_stream(got, w, what):
    assert got.size == w.size, "%s: %d bytes, the oracle has %d" % (what, got.size, w.size)
    bad = np.flatnonzero(got != w)
    assert bad.size == 0, "%s: %d bytes differ, the first at %d of %d" % (what, bad.size, bad[0], w.size)


def upload(gpu, d, a):
    """0x5A bytes, d from byte FRONT + a on, 0x5A bytes -> (tensor on a 16-byte boundary, where d begins in it)."""
    import torch

    arr = np.full(FRONT + a + d.size + BEHIND, 0x5A, dtype=np.uint8)
    arr[FRONT + a: FRONT + a + d.size] = d
    t = torch.from_numpy(arr).to(gpu)
    assert t.data_ptr() % 16 == 0
    return t, FRONT + a


@pytest.mark.parametrize("name", NAMES)
def test_case(name, z, oracle, cases, gpu):
    import torch

    k = cases[name]
    n = k.data.size
    w = want(oracle, cases, name)
    cap = up16(z.deflate_bound(n))
    for a in range(4):
        t, at = upload(gpu, k.data, a)
        out = torch.zeros(cap, dtype=torch.uint8, device=gpu)
        torch.cuda.synchronize()
        m = C.c_uint64()
        assert z.lib().zes_deflate_dev(t.data_ptr() + at, n, out.data_ptr(), cap, C.byref(m)) == 0, (name, a)
        same_stream(out[: m.value].cpu().numpy(), w, "%s, input at 16 k + %d" % (name, a))
        if a == 0:
            back = torch.zeros(n, dtype=torch.uint8, device=gpu)
            res = z.inflate_tensor(out[: m.value].clone(), back)
            assert res.numel() == n and (res.cpu().numpy() == k.data).all(), name
            view = t[at: at + n]
            for b, route in enumerate(k.routes):
                length = min(BLK, n - b * BLK)
                tok = z.stage_lz77_tensor(view, b * BLK, length)
                got = ec.decode_route(z.stage_lz77_route(), length)
                assert got["parse"] == route, "%s, block %d took %r" % (name, b, got)
                if b * BLK == k.start and k.matches is not None:
                    assert pc.token_matches(tok) == sorted(k.matches), name


def test_batch(z, oracle, cases, gpu):
    """pc.BATCH in one zes_deflate_batch_dev call, buffer i at in_off % 4 == (i + 1) % 4."""
    import torch

    in_off, out_off, at, ot = [], [], FRONT, 0
    for i, n in enumerate(pc.BATCH):
        at = up16(at) + (i + 1) % 4
        in_off.append(at)
        out_off.append(ot)
        at += cases[n].data.size + BEHIND
        ot += up16(z.deflate_bound(cases[n].data.size))
    arena = np.full(at, 0x5A, dtype=np.uint8)
    for n, off in zip(pc.BATCH, in_off):
        arena[off: off + cases[n].data.size] = cases[n].data
    assert [o % 4 for o in in_off] == [1, 2, 3, 0]
    out = torch.zeros(ot, dtype=torch.uint8, device=gpu)
    caps = [z.deflate_bound(cases[n].data.size) for n in pc.BATCH]
    olen, st = z.deflate_batch_tensor(torch.from_numpy(arena).to(gpu), in_off, [cases[n].data.size for n in pc.BATCH], out, out_off, caps)
    host = out.cpu().numpy()
    for n, off, ln, s in zip(pc.BATCH, out_off, olen, st):
        assert s == 0, n
        same_stream(host[off: off + int(ln)], want(oracle, cases, n), n + " in the batch")


@pytest.mark.parametrize("cuts", [(0, 1, 3), (0, 1, 2, 3), (0, 2, 3)])
def test_ranges_joined(cuts, z, oracle, cases, gpu):
    """Block ranges of three match-poor blocks (random bytes; the last one short) through zes_deflate_range_dev, each the
    oracle's bits, and joined: the stream of the whole."""
    import torch

    a = np.concatenate([cases["flagship"].data, cases["alternating"].data[2 * BLK: 3 * BLK], cases["planted_4095"].data[:5003]])
    n = a.size
    assert all(pc.found_upper(a[s: s + BLK]) <= pc.MLIST_CAP and ec.sort_model(a[s: s + BLK])[0] == "two" for s in range(0, n, BLK))
    if "ranges" not in _WANT:
        _WANT["ranges"] = oracle.deflate(a)
    t = torch.from_numpy(a.copy()).to(gpu)
    pieces, bits, adlers, lens = [], [], [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        lo, hi = lo * BLK, min(n, hi * BLK)
        p, nb, ad = z.deflate_range_tensor(t, lo, hi, final=(hi == n))
        want_p, want_bits = oracle.deflate_range(a, lo, hi - lo, hi == n)
        assert nb == want_bits and p.cpu().numpy().tobytes() == want_p.tobytes(), (cuts, lo)
        assert ad == oracle.adler32(a[lo:hi])
        pieces.append(p.clone())
        bits.append(nb)
        adlers.append(ad)
        lens.append(hi - lo)
    same_stream(z.deflate_join_tensors(pieces, bits, adlers, lens).cpu().numpy(), _WANT["ranges"], "joined %r" % (cuts,))
