"""tests/_sort_two_cases.py: every case's block is on k_lz_sort's two-level route and keeps the count the case states,
by the numpy restatement of the filter (ec.sort_model); and each case is at the seam it is named for."""
import numpy as np
import pytest

import _encoder_cases as ec
import _sort_two_cases as sc


@pytest.fixture(scope="module")
def cases(z):
    return sc.cases(z)


def test_every_case_stated(cases):
    assert sorted(cases) == sorted(sc.KEPT)
    assert {"len_%d" % n for n in sc.LENGTHS} <= set(cases)


@pytest.mark.parametrize("name", sorted(sc.KEPT))
def test_route_and_count(name, cases):
    assert ec.sort_model(sc.block(cases[name])) == ("two", sc.KEPT[name])


def test_lengths(cases):
    for n in sc.LENGTHS:
        assert sc.block(cases["len_%d" % n]).size == n
        assert sc.KEPT["len_%d" % n] > 0 or n < 18
    k = cases["second_1000"]
    assert k.start == sc.BLK and sc.block(k).size == 1000
    assert cases["odd_address"].odd


def test_seams(cases):
    key = ec._keys_le(sc.block(cases["seams"]))
    T = sc.BLK
    for p, q in ((127, 128), (8191, 8192), (65535, 65536), (70001, T - 3), (87, 168), (8091, 8292), (65528, 65543)):
        assert key[p] == key[q], (p, q)
    assert key.size - 1 == T - 3


def test_groups(cases):
    key = ec._keys_le(sc.block(cases["groups"]))
    assert sorted(np.nonzero(key == key[1005])[0]) == [1005, 3005, 9003]
    assert sorted(np.nonzero(key == key[2006])[0]) == [2006, 31007, 52009, 77011, 120013]
    assert key[40005] == key[40005 + 32768] and key[50006] == key[50006 + 32769]


def test_collisions(cases):
    blk = sc.block(cases["collisions"])
    key = ec._keys_le(blk)
    alone = np.bincount(key, minlength=1 << 24)[key] == 1
    k1 = sc.level1_kept(blk)
    h2 = sc.hash2(key)
    k2 = k1 & (np.bincount(h2[k1], minlength=1 << 19)[h2] >= 2)
    p, q = sc.COLLISIONS["level1"]
    assert alone[p] and alone[q] and key[p] != key[q]
    assert ec._h19(key[[p]], 0x9E3779B1) == ec._h19(key[[q]], 0x9E3779B1) and k1[p] and k1[q] and not k2[p] and not k2[q]
    r, s = sc.COLLISIONS["level2"]
    assert alone[r] and alone[s] and key[r] != key[s]
    assert h2[r] == h2[s] and k2[r] and k2[s]


def test_tiles_and_capacity(cases):
    for n in (sc.SORT_TILE - 1, sc.SORT_TILE, sc.SORT_TILE + 1):
        assert sc.KEPT["tile_%d" % n] == n
        assert sc.level1_kept(sc.block(cases["tile_%d" % n])).sum() <= sc.LIST_CAP  # the list holds them
    assert sc.level1_kept(sc.block(cases["cap_fits"])).sum() == sc.LIST_CAP
    assert sc.level1_kept(sc.block(cases["cap_over"])).sum() > sc.LIST_CAP
    assert sc.level1_kept(sc.block(cases["flagship"])).sum() <= sc.LIST_CAP


def test_overfull(cases):
    blk = sc.block(cases["overfull"])
    assert sc.level1_kept(blk).sum() * 2 > blk.size - 2, "the first level keeps more than half"
    assert sc.level1_kept(blk).sum() > sc.LIST_CAP
    assert sc.KEPT["overfull"] > sc.SORT_TILE
