"""k_lz_sort's two-level route on the blocks of tests/_sort_two_cases.py: the second filter level over the list of the
first level's survivors, at the seams of that list, and the walk over all positions that a block takes when its list
does not fit.  Every block goes through the stage entry: its tokens are the oracle's, the route record says two levels,
and the count the match finder got is the one the numpy restatement of the filter gives (ec.sort_model).

The pools are not cleared between calls: test_order runs every case after every other on one context, forwards and
backwards."""
import numpy as np
import pytest

import _encoder_cases as ec
import _sort_two_cases as sc
from test_gpu_encoder_cases import same_tokens

pytestmark = pytest.mark.gpu
NAMES = sorted(sc.KEPT)
_TOKENS = {}


@pytest.fixture(scope="module")
def cases(z):
    return sc.cases(z)


@pytest.fixture(scope="module")
def on_gpu(cases, gpu):
    """name -> the case's bytes on the device; an `odd` case one byte into its tensor."""
    import torch

    out = {}
    for name, k in cases.items():
        if k.odd:
            t = torch.zeros(k.data.size + 1, dtype=torch.uint8, device=gpu)[1:]
            t.copy_(torch.from_numpy(k.data.copy()))
            assert t.data_ptr() % 2 == 1
        else:
            t = torch.from_numpy(k.data.copy()).to(gpu)
        out[name] = t
    return out


def want_tokens(oracle, cases, name):
    """The oracle's tokens of a case's block (computed once, shared, never changed)."""
    if name not in _TOKENS:
        k = cases[name]
        t = oracle.lz77_block(k.data, k.start, sc.block(k).size)
        t.setflags(write=False)
        _TOKENS[name] = t
    return _TOKENS[name]


def stage(z, t, k):
    length = sc.block(k).size
    tok = z.stage_lz77_tensor(t, k.start, length)
    return tok, z.stage_lz77_route(), length


@pytest.mark.parametrize("name", NAMES)
def test_case(name, z, oracle, cases, on_gpu):
    k = cases[name]
    tok, words, length = stage(z, on_gpu[name], k)
    same_tokens(tok, want_tokens(oracle, cases, name), name)
    route = ec.decode_route(words, length)
    print(name, [hex(int(w)) for w in words], route)
    assert route["sort"] == "two"
    assert route["kept"] == ec.sort_model(sc.block(k))[1] == sc.KEPT[name]


def test_order(z, oracle, cases, on_gpu):
    """Every case after every other on one context, then in reverse: the same tokens and the same record both times."""
    seen = {}
    for name in NAMES + NAMES[::-1]:
        tok, words, _ = stage(z, on_gpu[name], cases[name])
        same_tokens(tok, want_tokens(oracle, cases, name), name)
        if name in seen:
            assert (words == seen[name]).all(), "%s: %r after its successors, %r after its predecessors" % (name, list(words), list(seen[name]))
        seen[name] = words
