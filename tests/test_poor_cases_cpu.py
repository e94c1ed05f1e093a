"""tests/_poor_cases.py: every case sits where its name says.  The oracle's tokens (oracle.lz77_block) show the matches
a case was built for; ec's restatements of k_lz_sort's and k_lz_match's decisions (ec.sort_model, ec.prev_same_key) show
that every block named "list" has between 0 and 4095 found matches and is not the lazy matcher's, and that the blocks
meant to leave that route do leave it."""
import numpy as np
import pytest

import _encoder_cases as ec
import _poor_cases as pc

BLK, W, T = pc.BLK, pc.W, pc.T
NAMES = pc.NAMES


@pytest.fixture(scope="module")
def cases(z):
    return pc.cases(z)


@pytest.fixture(scope="module")
def matches(cases, oracle):
    """name -> (position, length, distance) of every match in the oracle's tokens of the block under test."""
    return {name: pc.token_matches(oracle.lz77_block(k.data, k.start, k.length)) for name, k in cases.items()}


def blocks(k):
    return [k.data[s: s + BLK] for s in range(0, k.data.size, BLK)]


def test_constants_and_names(cases):
    assert sorted(cases) == NAMES
    assert (W, T, pc.MLIST_CAP) == (512, 8192, 4095) and T % W == 0
    assert pc.LENGTHS == [2, 3, 4, 5, 255, 256, 257, 8191, 8192, 8193, 131071, 131072]
    assert set(pc.BATCH) <= set(cases) and len(pc.BATCH) == 4
    for name, k in cases.items():
        assert k.start % BLK == 0 and k.length == min(BLK, k.data.size - k.start) and len(k.routes) == len(blocks(k)), name
        assert k.data.size <= 3 * BLK + 3000, name
    assert cases["second_2"].data.size == BLK + 2 and cases["second_2"].length == 2


@pytest.mark.parametrize("name", NAMES)
def test_routes(name, cases):
    """Every block of every case: the route its case states, by the kernels' own integer decisions."""
    for b, route in zip(blocks(cases[name]), cases[name].routes):
        sort, kept = ec.sort_model(b)
        if route == "mask":
            assert sort in ("dense", "to_index"), (name, sort)
            continue
        assert sort in ("nokeys", "two"), (name, sort)  # (k_lz_sort keeps few positions of it: k_lz_match's block)
        if route == "list":
            assert 0 <= pc.found_upper(b) <= pc.MLIST_CAP, name
        else:
            assert route == "maps" and ec.eager_matches(b) > pc.MLIST_CAP, name


@pytest.mark.parametrize("name", NAMES)
def test_matches_as_built(name, cases, matches):
    if cases[name].matches is not None:
        assert matches[name] == sorted(cases[name].matches), name


def test_found_counts(cases):
    assert ec.eager_matches(cases["planted_4095"].data) == pc.MLIST_CAP
    assert ec.eager_matches(cases["planted_4096"].data) == pc.MLIST_CAP + 1
    assert 100 < pc.found_upper(cases["flagship"].data) < 400
    for n in pc.LENGTHS:
        assert pc.found_upper(cases["len_%d" % n].data) == 0


def test_seams(cases, matches):
    """The planted matches lie where the kernels' loops turn."""
    for n in pc.END_EXACT:
        ((p, ln, _),) = matches["end_exact_%d" % n]
        assert p + ln == n - 3
    ((p, ln, _),) = matches["tile_seam"]
    assert p % T == T - 1 and ln > 1
    at = [p for p, _, _ in matches["run_seam"]]
    assert at[0] % W == 255 and at[1] % W == W - 1 and at[2] % W == W - 1 and at[2] > T
    for name in ("back_to_back", "back_to_back_3"):
        (p1, l1, _), (p2, _, _) = matches[name]
        assert p1 + l1 == p2
    (p1, l1, _), (p2, _, _) = matches["back_to_back_3"]
    assert p1 % 4 == 0 and l1 == 3 and p2 // 4 == p1 // 4
    assert sorted(ln for _, ln, _ in matches["len_258_3"]) == [3, 42, 258]
    assert set(pc.DIST_1_MAX) <= set(matches["dist_1_max"])
    assert not any(32768 + 1990 < p < 32768 + 2012 for p, _, _ in matches["dist_1_max"]), "a repeat 32769 apart is no match"


def test_covered_start(cases, matches):
    """covered_longer: k_lz_match finds a match at 2003 (the key there stands at 300 too), ten bytes long; the greedy parse
    has taken five bytes from 2000 and goes on at 2005, inside it."""
    a = cases["covered_longer"].data
    assert ec.prev_same_key(a)[2003] == 2003 - 300 and (a[2003: 2013] == a[300: 310]).all() and a[2013] != a[310]
    assert matches["covered_longer"] == [(2000, 5, 1950), (2005, 8, 1703)]


def test_alternating_blocks(cases, oracle):
    k = cases["alternating"]
    share = [pc.token_matches(oracle.lz77_block(k.data, s, min(BLK, k.data.size - s))) for s in range(0, k.data.size, BLK)]
    assert len(share[0]) < 400 and len(share[2]) < 400 and len(share[1]) > 10000 and len(share[3]) > 100
