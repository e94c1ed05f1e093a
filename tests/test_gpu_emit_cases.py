"""k_emit on the inputs of tests/_emit_cases.py: token counts at the seams of its header copy, of a wave's run and of
its tile, the fewest and the most bits an item can have, groups with and without matches.  Every case goes through
z.deflate_tensor (the batch through z.deflate_batch_tensor) and must be the oracle's stream: its length and every byte.

The pools are not cleared between calls: test_order runs every case after every other on one context, forwards and
backwards."""
import numpy as np
import pytest

import _emit_cases as em

pytestmark = pytest.mark.gpu
NAMES = sorted(["ntok_%d" % n for n in em.COUNTS] + ["literals_full", "literals_two_blocks_5", "one_byte_full", "one_byte_full_7", "two_symbols",
                                                      "deep_long_items", "match_every_group", "random_block"])
_WANT = {}


@pytest.fixture(scope="module")
def cases(z):
    c = em.cases(z)
    assert sorted(c) == NAMES
    return c


@pytest.fixture(scope="module")
def on_gpu(cases, gpu):
    import torch

    return {name: torch.from_numpy(a.copy()).to(gpu) for name, a in cases.items()}


def want(oracle, cases, name):
    """The oracle's stream of a case (computed once, shared, never changed)."""
    if name not in _WANT:
        w = oracle.deflate(cases[name])
        w.setflags(write=False)
        _WANT[name] = w
    return _WANT[name]


def same_stream(got, w, name):
    assert got.size == w.size, "%s: %d bytes, the oracle has %d" % (name, got.size, w.size)
    bad = np.flatnonzero(got != w)
    assert bad.size == 0, "%s: %d bytes differ, the first at %d of %d" % (name, bad.size, bad[0], w.size)


@pytest.mark.parametrize("name", NAMES)
def test_case(name, z, oracle, cases, on_gpu):
    same_stream(z.deflate_tensor(on_gpu[name]).cpu().numpy(), want(oracle, cases, name), name)


def test_one_token_blocks_throw(z, gpu):
    import torch

    for n in (1, em.BLK + 1):
        with pytest.raises(z.ZlibEsError):
            z.deflate_tensor(torch.full((n,), 7, dtype=torch.uint8, device=gpu))


def test_batch(z, oracle, cases, gpu):
    import torch

    def up(x):
        return (x + 15) // 16 * 16

    in_off, out_off, at, ot = [], [], 0, 0
    for n in em.BATCH:
        in_off.append(at)
        out_off.append(ot)
        at += up(cases[n].size) + 16
        ot += up(z.deflate_bound(cases[n].size))
    arena = np.zeros(at, dtype=np.uint8)
    for n, off in zip(em.BATCH, in_off):
        arena[off: off + cases[n].size] = cases[n]
    out = torch.zeros(ot, dtype=torch.uint8, device=gpu)
    caps = [z.deflate_bound(cases[n].size) for n in em.BATCH]
    olen, st = z.deflate_batch_tensor(torch.from_numpy(arena).to(gpu), in_off, [cases[n].size for n in em.BATCH], out, out_off, caps)
    host = out.cpu().numpy()
    for n, off, ln, s in zip(em.BATCH, out_off, olen, st):
        assert s == 0, n
        same_stream(host[off: off + int(ln)], want(oracle, cases, n), n)


def test_order(z, oracle, cases, on_gpu):
    """Every case after every other on one context, then in reverse: the oracle's stream both times."""
    seen = {}
    for name in NAMES + NAMES[::-1]:
        got = z.deflate_tensor(on_gpu[name]).cpu().numpy()
        same_stream(got, want(oracle, cases, name), name)
        if name in seen:
            assert (got == seen[name]).all(), "%s: another stream after its successors than after its predecessors" % name
        seen[name] = got
