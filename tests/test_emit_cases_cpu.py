"""tests/_emit_cases.py: every case sits where its name says, by the oracle's tokens (oracle.lz77_block) and the
oracle's code lengths (oracle.huff_lengths)."""
import numpy as np
import pytest

import _emit_cases as em

BLK, W, T = em.BLK, em.W, em.T


@pytest.fixture(scope="module")
def cases(z):
    return em.cases(z)


@pytest.fixture(scope="module")
def tokens(cases, oracle):
    """name -> the oracle's tokens of every block of the case."""
    out = {}
    for name, a in cases.items():
        out[name] = [oracle.lz77_block(a, s, min(BLK, a.size - s)) for s in range(0, a.size, BLK)]
    return out


def test_constants_and_names(cases):
    assert (W, T) == (512, 8192) and T % W == 0
    assert em.COUNTS == [2, 5, 255, 256, 257, 511, 512, 513, 8191, 8192, 8193, 16387]
    assert {"ntok_%d" % n for n in em.COUNTS} <= set(cases)
    assert set(em.BATCH) <= set(cases) and len(em.BATCH) == 3
    assert len({cases[n].size for n in em.BATCH}) == 3


@pytest.mark.parametrize("n", em.COUNTS)
def test_token_counts(n, cases, tokens):
    (tok,) = tokens["ntok_%d" % n]
    assert cases["ntok_%d" % n].size == n
    assert tok.size == n and not em.is_match(tok).any()


def test_no_block_of_one_token(oracle):
    """A block of one token is a block of one byte; those inputs throw."""
    for n in (1, BLK + 1):
        with pytest.raises(oracle.OracleError):
            oracle.deflate(np.full(n, 7, dtype=np.uint8))


def test_literal_blocks(tokens):
    (tok,) = tokens["literals_full"]
    assert tok.size == BLK and not em.is_match(tok).any()
    assert [t.size for t in tokens["literals_two_blocks_5"]] == [BLK, BLK, 5]
    assert not any(em.is_match(t).any() for t in tokens["literals_two_blocks_5"])


def test_fewest_bits(cases, tokens):
    (tok,) = tokens["one_byte_full"]
    bits = em.item_bits(tok)[2]
    assert bits.min() >= 1 and bits.max() <= 3
    assert bits.sum() < 1400 and tok.size < 2 * W  # all of it in the first two waves' runs
    first, second = tokens["one_byte_full_7"]
    assert first.size == tok.size and second.size == 7
    (tok,) = tokens["two_symbols"]
    assert tok.size == cases["two_symbols"].size == 10 and not em.is_match(tok).any()
    assert sorted(set(em.item_bits(tok)[2].tolist())) == [1, 2]


def test_longest_items(tokens):
    (tok,) = tokens["deep_long_items"]
    ll, dl, bits, xl, xd = em.item_bits(tok)
    assert ll.max() == 15
    assert bits.max() >= 45
    assert ((xl == 5) & (xd == 13) & (bits >= 45)).any()
    q, d, length = em.DEEP_FAR
    at = int(np.flatnonzero(em.token_positions(tok) == q)[0])
    assert em.is_match(tok[at: at + 1]).all() and int(tok[at] & 0x7FFF) + 1 == d and int((tok[at] >> 16) & 0xFF) + 3 == length
    assert bits[at] == bits.max()


def test_match_in_every_group(tokens):
    (tok,) = tokens["match_every_group"]
    assert tok.size > 6 * T
    assert em.group_has_match(tok).all()


def test_random_block_mixes_paths(tokens):
    (tok,) = tokens["random_block"]
    g = em.group_has_match(tok)
    assert 100 < g.sum() < g.size // 64
    # a wave's group: 64 lanes' groups of four, 256 consecutive tokens; its two groups of a tile lie in one run of W
    full = tok.size // W * W
    wave_group = em.is_match(tok[:full]).reshape(-1, 2, 256).any(axis=2)
    assert (wave_group[:, 0] != wave_group[:, 1]).any(), "a wave with one literal group and one with a match"
    assert wave_group.all(axis=1).any() and (~wave_group).all(axis=1).any()
