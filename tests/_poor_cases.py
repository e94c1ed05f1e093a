"""Inputs for the position form of match-poor blocks, built at the seams of the two kernels that share it.

A block in which k_lz_match finds at most 4095 matches is parsed from the list of them (k_lz_parse_small).  In the
pipeline such a block has no token list: the parse leaves a bit per position for "on the greedy chain" and one for "a
taken match starts here", and k_emit makes its items from positions, a tile of T at a time: a wave owns a run of W
positions of the tile, a lane two groups of four consecutive positions in it, 256 apart.  A position on the chain is the
literal of its input byte or, at a taken start, the match word k_lz_match left there; a position inside a match has no
bits; end-of-block is the item behind the last position.  The input may begin at any byte: the kernels read it in whole
aligned words.  The cases, each a Case(data, start, length, routes, matches):

    len_<n>             n bytes in which no 3-byte key repeats (no match at all), for the shortest blocks, a group of
                        lanes' and a wave's share (255, 256, 257), the tile (8191, 8192, 8193) and the block (131071, 131072)
    second_2            a second block of two bytes behind a full one
    end_exact_<n>       one match that ends where the reference lets the last one end: three bytes in front of the block's
                        end (src/lz77.ts: the last three bytes are never inside a match), at a short, a tile-seam and the
                        full length
    tile_seam           a match that starts on a tile's last position and covers into the next tile
    run_seam            matches that start on the last position of a wave's first group and of a wave's run
    back_to_back        two matches, the second starting where the first ends
    back_to_back_3      the same with a first match of three bytes at a position 4 k: both starts in one lane's group
    covered_longer      a found match the greedy parse does not take because the one before covers its start, and which
                        reaches further than that one: its start bit must be cleared, and the parse goes on inside it
    len_258_3           a repeat of 300 bytes (a match of 258, the rest back to back) and a match of 3
    dist_1_max          distance 1 (a run of one byte) and 32768, the largest there is; a repeat 32769 apart is no match
    planted_4095        exactly 4095 found matches: the list is full
    planted_4096        one more: the block leaves the route (k_lz_parse's exit maps, a token list)
    flagship            bench.py's random64 leg, its first block: about 216 matches by accident
    alternating         random bytes, text, random bytes, text: blocks of this route and of the lazy one side by side

`matches` is what the oracle's tokens of the block under test must show: every (position, length, distance), or None
where the bytes are not built match by match.  `routes` names the parse route of every block of the input ("list", "mask"
or "maps", ec.decode_route's words).  No bytes are stored: numpy's generators and the library's make them again.
tests/test_poor_cases_cpu.py proves with the oracle and ec's models of the kernels' decisions that every case sits where
its name says."""
import collections

import numpy as np

import _encoder_cases as ec

BLK = ec.BLK
EMIT_WAVE_RUN = 512  # W: positions of a tile that one wave owns (EMIT_WAVE_RUN of zes_deflate.hip)
EMIT_TILE = 8192     # T: positions per tile (EMIT_TILE of zes_deflate.hip)
W, T = EMIT_WAVE_RUN, EMIT_TILE
MLIST_CAP = ec.MLIST_CAP

Case = collections.namedtuple("Case", "data start length routes matches")

LENGTHS = [2, 3, 4, 5, 255, 256, 257, T - 1, T, T + 1, BLK - 1, BLK]
END_EXACT = [600, T + 1, BLK]
SEAM_LEN = 3 * T + 100  # the length of the blocks with planted matches, unless the case needs another
DIST_1_MAX = [(201, 59, 1), (1000 + 32768, 8, 32768)]  # dist_1_max: the run's match and the farthest one; none at 2000 + 32769
NAMES = sorted(["len_%d" % n for n in LENGTHS] + ["end_exact_%d" % n for n in END_EXACT] +
               ["second_2", "tile_seam", "run_seam", "back_to_back", "back_to_back_3", "covered_longer", "len_258_3", "dist_1_max",
                "planted_4095", "planted_4096", "flagship", "alternating"])  # every case of cases(z)
BATCH = ["alternating", "flagship", "len_257", "back_to_back_3"]  # buffers of one zes_deflate_batch_dev call, at in_off % 4 = 1, 2, 3, 0


def _one(data, matches, route="list"):
    return Case(data, 0, data.size, [route], matches)


def _copy(a, src, dst, n):
    """a[dst : dst + n] = a[src : src + n], the bytes in front of and behind the two places made different: a match of n
    exactly at dst, from src."""
    a[dst: dst + n] = a[src: src + n]
    a[dst - 1] = a[src - 1] ^ 0x80
    a[dst + n] = a[src + n] ^ 0x80
    return (dst, n, dst - src)


def _two_in_a_row(z, seed, n1, n2):
    """Matches of n1 and n2 bytes at 2000 and 2000 + n1, from 50 and 300."""
    a = ec._unique(z, seed, SEAM_LEN).copy()
    p, q = 2000, 2000 + n1
    a[p: p + n1] = a[50: 50 + n1]
    a[q: q + n2] = a[300: 300 + n2]
    a[p - 1] = a[49] ^ 0x80
    a[50 + n1] = a[q] ^ 0x55       # the first match ends where the second begins
    a[299] = a[q - 1] ^ 0x33       # the second does not begin earlier
    a[q + n2] = a[300 + n2] ^ 0x80
    return _one(a, [(p, n1, p - 50), (q, n2, q - 300)])


def cases(z):
    """name -> Case."""
    c = {}
    for n in LENGTHS:
        c["len_%d" % n] = _one(ec._unique(z, 900 + n % 97, n).copy(), [])
    a = np.concatenate([ec._unique(z, 911, BLK), np.array([0x31, 0x32], dtype=np.uint8)])
    c["second_2"] = Case(a, BLK, 2, ["list", "list"], [])
    for n in END_EXACT:
        a = ec._unique(z, 920 + n % 89, n).copy()
        dst = n - 3 - 12
        c["end_exact_%d" % n] = _one(a, [_copy(a, max(100, dst - 1000), dst, 12)])
    a = ec._unique(z, 931, SEAM_LEN).copy()
    c["tile_seam"] = _one(a, [_copy(a, 100, T - 1, 20)])
    a = ec._unique(z, 932, SEAM_LEN).copy()
    c["run_seam"] = _one(a, [_copy(a, 40, W + 255, 9), _copy(a, 60, 3 * W - 1, 11), _copy(a, 90, T + 5 * W - 1, 7)])
    c["back_to_back"] = _two_in_a_row(z, 933, 7, 6)
    c["back_to_back_3"] = _two_in_a_row(z, 934, 3, 8)
    # X (5 bytes) at 50 and 2000; Y (10 bytes, its first two are X's last two) at 300 and 2003
    a = ec._unique(z, 935, SEAM_LEN).copy()
    a[300: 302] = a[53: 55]
    a[2000: 2003] = a[50: 53]
    a[2003: 2013] = a[300: 310]
    a[1999], a[55], a[2013] = a[49] ^ 0x80, a[302] ^ 0x80, a[310] ^ 0x80
    c["covered_longer"] = _one(a, [(2000, 5, 1950), (2005, 8, 1703)])
    a = ec._unique(z, 936, SEAM_LEN).copy()
    a[5000: 5300] = a[100: 400]
    a[4999], a[5300] = a[99] ^ 0x80, a[400] ^ 0x80
    c["len_258_3"] = _one(a, [(5000, 258, 4900), (5258, 42, 4900), _copy(a, 8000, 9000, 3)])
    a = np.concatenate([ec._unique(z, 937, 3000), z.gen("xorshift", 938, 40000 - 3000)])
    a[199], a[200: 260], a[260] = 0x11, 0x58, 0x22
    w1, w2 = z.gen("xorshift", 939, 8), z.gen("xorshift", 940, 8)
    a[1000: 1008], a[1000 + 32768: 1008 + 32768] = w1, w1
    a[2000: 2008], a[2000 + 32769: 2008 + 32769] = w2, w2
    a[999 + 32768], a[1008 + 32768] = a[999] ^ 0x80, a[1008] ^ 0x80
    c["dist_1_max"] = _one(a, None)  # (DIST_1_MAX: the matches the case is about, among the few its random bytes hold by accident)
    c["planted_4095"] = _one(ec._planted(z, 62, MLIST_CAP), None)
    c["planted_4096"] = _one(ec._planted(z, 63, MLIST_CAP + 1), None, route="maps")
    c["flagship"] = _one(z.gen("xorshift", 12345, BLK), None)
    a = np.concatenate([z.gen("xorshift", 951, BLK), z.gen("itext", 952, BLK), z.gen("xorshift", 953, BLK), z.gen("itext", 954, 3000)])
    c["alternating"] = Case(a, 0, BLK, ["list", "mask", "list", "mask"], None)
    for k in c.values():
        k.data.setflags(write=False)
    return c


def token_matches(tok):
    """(position, length, distance) of every match among a block's tokens."""
    m = (tok & 0x80000000) != 0
    ln, ds = ((tok >> 16) & 0xFF).astype(np.int64) + 3, (tok & 0x7FFF).astype(np.int64) + 1
    pos = np.concatenate([[0], np.cumsum(np.where(m, ln, 1))[:-1]]) if tok.size else np.zeros(0, dtype=np.int64)
    return [(int(p), int(l), int(d)) for p, l, d in zip(pos[m], ln[m], ds[m])]


def found_upper(block):
    """No more matches than this does k_lz_match find in a block: the positions whose nearest earlier position of the same
    key lies within the window (ec.eager_matches, without its demand on the block's tail: a match there may not count)."""
    if len(block) < 3:
        return 0
    d = ec.prev_same_key(block)
    return int(((d > 0) & (d <= ec.WINDOW)).sum())
