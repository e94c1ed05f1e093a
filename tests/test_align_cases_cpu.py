"""The surroundings of tests/_align_cases.py would be noticed: with the oracle alone, no GPU.  tests/test_gpu_input_alignment.py
hands the kernels inputs that stand at an unaligned address between a `front` and a `behind`; a kernel that reads past the
input's end, or from in front of it, computes what the oracle computes on the longer input.  Here the oracle is run on
that longer input: for the cases named below its tokens are other ones, so such a kernel fails those cases."""
import numpy as np
import pytest

import _align_cases as al
import _encoder_cases as ec
from conftest import golden

NAMES = sorted(golden("encoder_cases.json"))
END_CASES = {"run_to_end", "end_plus1", "one_literal", "periodic_short"}


@pytest.fixture(scope="module")
def cases(z):
    return ec.cases(z)


def last_block(d):
    start = (d.size - 1) // ec.BLK * ec.BLK
    return start, d.size - start


def covering(tok, pos):
    """(token, its first position) of the token of a block that covers the block's position `pos`."""
    at = 0
    for t in tok:
        step = ((int(t) >> 16) & 0xFF) + 3 if t & 0x80000000 else 1
        if at + step > pos:
            return int(t), at
        at += step
    raise AssertionError("position %d is behind the tokens" % pos)


@pytest.mark.parametrize("fill", al.FILLS)
def test_reading_past_the_end_changes_tokens(fill, cases, oracle):
    """The last block's tokens with the true n, and with `behind` counted as input (same block start): the cases whose
    tokens change within the true ones' count."""
    changed = set()
    for name in NAMES:
        d = cases[name].data
        start, length = last_block(d)
        true = oracle.lz77_block(d, start, length)
        ext = np.concatenate([d, al.behind_of(d, fill, al.last_match_dist(true))])
        longer = oracle.lz77_block(ext, start, min(ec.BLK, ext.size - start))
        if longer.size < true.size or (longer[: true.size] != true).any():
            changed.add(name)
    print(fill, sorted(changed))
    assert changed and END_CASES <= changed, "not changed: %s" % sorted(END_CASES - changed)
    claim = {n for n in NAMES if "run_to_input_end" in cases[n].rules}
    assert claim and claim <= changed


@pytest.mark.parametrize("name", ["nokeys_300", "random_short", "ntok_4097"])
def test_reading_in_front_changes_tokens(name, cases, oracle):
    """front || d taken as one input: where d starts stands a match that reaches back over the whole of `front`, where d
    alone has a literal (the three cases repeat no key, so nothing but `front` can give that match)."""
    d = cases[name].data
    alone = oracle.lz77_block(d, 0, min(ec.BLK, d.size))
    assert covering(alone, 0) == (int(d[0]), 0)
    for a in range(16):
        ext = np.concatenate([al.front_of(d, a), d])
        tok, at = covering(oracle.lz77_block(ext, 0, min(ec.BLK, ext.size)), al.FRONT + a)
        assert at == al.FRONT + a and tok & 0x80000000, (name, a)
        assert (tok & 0x7FFF) + 1 == al.FRONT + a and ((tok >> 16) & 0xFF) + 3 >= al.FRONT, (name, a)


def test_layout(cases, oracle):
    assert al.FRONT % 16 == 0 and al.FRONT >= 32 and al.BEHIND >= 258 + 32
    for name in NAMES:
        d = cases[name].data
        n = d.size
        dist = al.last_match_dist(oracle.lz77_block(d, *last_block(d)))
        assert 1 <= dist <= n
        for a in range(16):
            for fill in al.FILLS:
                arr, at = al.surround(d, a, fill, dist)
                assert at == al.FRONT + a and arr.size == at + n + al.BEHIND and arr.dtype == np.uint8
                assert (arr[at: at + n] == d).all(), "the input's bytes changed"
                front, behind = arr[:at], arr[at + n:]
                assert (front == np.resize(d, at)).all()
                if fill == "run":
                    assert (behind == d[-1]).all()
                else:
                    assert (arr[at + n:] == arr[at + n - dist: arr.size - dist]).all()


def test_arena(cases):
    """The batch layout: every input in its own surroundings, at the misalignment asked for."""
    names = [n for n in NAMES if cases[n].data.size <= ec.BLK]
    items = [(cases[n].data, (5 * i + 3) % 16, al.FILLS[i % 2], 1) for i, n in enumerate(names)]
    arr, in_off = al.arena(items)
    assert arr.size % 16 == 0 and len(in_off) == len(items)
    end = 0
    for (d, a, fill, dist), off in zip(items, in_off):
        assert off % 16 == a and off - (al.FRONT + a) >= end and (off - (al.FRONT + a)) % 16 == 0
        one, at = al.surround(d, a, fill, dist)
        assert (arr[off - at: off - at + one.size] == one).all()
        end = off - at + one.size
    assert end <= arr.size
