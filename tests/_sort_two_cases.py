"""Blocks for k_lz_sort's two-level route, built at the seams of the list its second level runs over.

The first filter level's survivors are listed as 16-bit entries, a thread's run of 128 positions after the other, and
shared out over the waves two entries a word; the second level's survivors are listed again, and the sort takes that
list.  A block on this route that keeps more than a quarter of its positions walks all of them instead.  The cases:

    len_<n>        random bytes of every block length at which a loop bound, the 16-bit split or the tile of the sort
                   changes, with a few planted repeats so that something is kept (3 and 4 bytes hold no repeat)
    second_1000    the second block, 1 000 bytes, of a two-block input
    odd_address    a block that starts at an odd device address (the test uploads it one byte into its tensor)
    seams          repeated keys whose two positions lie on both sides of a thread's run (127 | 128), a wave's share
                   (8191 | 8192), the 16-bit split (65535 | 65536), and at the last key of the block
    groups         a key present three and five times, and pairs exactly 32768 and 32769 apart
    collisions     no plant at all: a pair of unlike keys in one bucket of the first level (both dropped by the second)
                   and a pair in one bucket of the second (both kept), at the positions stated in COLLISIONS
    tile_<n>       pairs planted until the final list has SORT_TILE - 1, SORT_TILE and SORT_TILE + 1 entries
    cap_fits, cap_over  the first level keeps exactly LIST_CAP positions, every register of the list in use, and a few more
    overfull       the sample sees random bytes, the rest comes from eight letters: the first level keeps three
                   quarters of the positions, the list does not fit and the block takes the walk over all positions
    flagship       bench.py's random64 leg, its first block

No bytes are stored: numpy's generators and the library's make them again.  KEPT states what ec.sort_model gives for
every case; tests/test_sort_two_cases_cpu.py checks that, so the route is a property of the bytes."""
import collections

import numpy as np

import _encoder_cases as ec

BLK = ec.BLK
SORT_TILE = 8192
LIST_CAP = 32768  # first-level survivors the list holds (SORT_LIST_CAP of zes_deflate.hip)

Case = collections.namedtuple("Case", "data start odd")

LENGTHS = [3, 4, 18, 127, 128, 129, 1023, 1025, 8191, 8193, 65535, 65536, 65537, 131071, 131072]

# (pairs, third copies) planted for a final list of the stated length (found by counting up; tests/test_sort_two_cases_cpu.py checks them)
TILE_LEN = 65536  # (a full block with so many plants keeps more than LIST_CAP at the first level)
TILE_PAIRS = {8191: (3886, 0), 8192: (3886, 1), 8193: (3887, 0)}

# (pairs, third copies) in a full block for a first-level count of exactly LIST_CAP, and the next count above it
CAP_PAIRS = {"cap_fits": (2571, 2), "cap_over": (2572, 0)}

# collisions: (p, q) unlike keys, one first-level bucket; (r, s) unlike keys kept by the first level, one second-level bucket
COLLISIONS = {"level1": (4500, 129271), "level2": (8696, 12501)}

# positions the sort takes, per case (ec.sort_model's count)
KEPT = {"len_3": 0, "len_4": 0, "len_18": 2, "len_127": 8, "len_128": 8, "len_129": 8, "len_1023": 8, "len_1025": 8, "len_8191": 14,
        "len_8193": 10, "len_65535": 363, "len_65536": 337, "len_65537": 355, "len_131071": 2421, "len_131072": 2464,
        "second_1000": 8, "odd_address": 465, "seams": 2399, "groups": 2410, "collisions": 2468, "tile_8191": 8191,
        "tile_8192": 8192, "tile_8193": 8193, "cap_fits": 7665, "cap_over": 7665, "overfull": 97610, "flagship": 2477}


def _random(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _copy3(d, a, b):
    d[b: b + 3] = d[a: a + 3]


def _planted_len(n):
    """Random bytes with up to four planted repeats: the second position of a pair at 3 .. 13 of its run of sixteen, so
    that no sampled key (every sixteenth position) changes."""
    d = _random(1000 + n, n)
    slots = [s for s in range(0, n - 2, 16) if s + 8 <= n]  # bytes s + 5 .. s + 7 of run s
    if len(slots) >= 2:
        rng = np.random.default_rng(n)
        pick = rng.permutation(len(slots))[: min(8, len(slots) // 2 * 2)]
        for a, b in zip(pick[0::2], pick[1::2]):
            _copy3(d, slots[a] + 5, slots[b] + 5)
    elif n >= 18:
        _copy3(d, 1, 5)
    return d


def _slot(s):
    """Byte offset of plant slot s: three to a run of sixteen (bytes 3 .. 5, 7 .. 9, 11 .. 13), none on a sampled key."""
    return 16 * (s // 3) + 3 + 4 * (s % 3)


def _plant_pairs(d, npairs, ntriples, seed):
    """npairs repeats between distinct slots, no plant touching another; then a third copy of the first ntriples keys."""
    order = [int(s) for s in np.random.default_rng(seed).permutation(d.size // 16 * 3)]
    for i in range(npairs):
        _copy3(d, _slot(order[2 * i]), _slot(order[2 * i + 1]))
    for i in range(ntriples):
        _copy3(d, _slot(order[2 * i]), _slot(order[2 * npairs + i]))
    return d


def _seams():
    d = _random(21, BLK)
    for p in (127, 8191, 65535):  # four equal bytes: positions p and p + 1 hold one key
        d[p: p + 4] = d[p]
    _copy3(d, 70001, BLK - 3)  # the last key of the block
    _copy3(d, 127 - 40, 128 + 40)  # and pairs further apart over the same seams
    _copy3(d, 8191 - 100, 8192 + 100)
    _copy3(d, 65535 - 7, 65536 + 7)
    return d


def _groups():
    d = _random(22, BLK)
    for b in (3005, 9003):  # key of 1005 three times
        _copy3(d, 1005, b)
    for b in (31007, 52009, 77011, 120013):  # key of 2006 five times
        _copy3(d, 2006, b)
    _copy3(d, 40005, 40005 + 32768)
    _copy3(d, 50006, 50006 + 32769)
    return d


def _overfull():
    rng = np.random.default_rng(1)
    d = rng.integers(0, 256, BLK, dtype=np.uint8)
    low = rng.integers(0, 8, BLK, dtype=np.uint8) + 97
    keep = (np.arange(BLK) % 16) < 3
    return np.where(keep, d, low).astype(np.uint8)


def cases(z):
    """name -> Case(data, start, odd): the block is data[start: start + BLK]."""
    out = {}
    for n in LENGTHS:
        out["len_%d" % n] = Case(_planted_len(n), 0, False)
    two = np.concatenate([_random(31, BLK), _planted_len(1000)])
    out["second_1000"] = Case(two, BLK, False)
    out["odd_address"] = Case(_planted_len(70001), 0, True)
    out["seams"] = Case(_seams(), 0, False)
    out["groups"] = Case(_groups(), 0, False)
    out["collisions"] = Case(_random(23, BLK), 0, False)
    for n, pairs in sorted(TILE_PAIRS.items()):
        out["tile_%d" % n] = Case(_plant_pairs(_random(24, TILE_LEN), pairs[0], pairs[1], 25), 0, False)
    for name, pairs in sorted(CAP_PAIRS.items()):
        out[name] = Case(_plant_pairs(_random(26, BLK), pairs[0], pairs[1], 27), 0, False)
    out["overfull"] = Case(_overfull(), 0, False)
    out["flagship"] = Case(z.gen("xorshift", 12345, BLK), 0, False)
    for k in out.values():
        k.data.setflags(write=False)
    return out


def block(k):
    return k.data[k.start: k.start + BLK]


def level1_kept(blk):
    """Positions the first filter level keeps (sort_model's first hash and counters)."""
    key = ec._keys_le(blk)
    h = ec._h19(key, 0x9E3779B1)
    return np.bincount(h, minlength=1 << 19)[h] >= 2


def hash2(key):
    return (((key ^ (key >> 11)).astype(np.uint64) * 0xC2B2AE35) & 0xFFFFFFFF) >> 13
