"""Inputs for k_emit, built at the seams of its tile loop.

The kernel takes a block's tokens a tile of T at a time; inside a tile a wave owns a contiguous run of W tokens, a lane
two groups of four in it.  A group in which no lane of the wave holds a match is packed as one piece of literals; every
other group keeps its four items.  The header bits are copied in front of the loop, end-of-block is the item behind the
last token.  The cases:

    ntok_<n>            n bytes in which no 3-byte key repeats: n literal tokens, for every n at which the header copy, a
                        wave's run or the tile ends (a block of one token would be a block of one byte: inputs of 1 and
                        of 131072 k + 1 bytes throw by design, so there is none)
    literals_full       131072 literal tokens: the flagship's shape
    literals_two_blocks_5   two such blocks and five bytes: the dword two blocks share, and a last block of five tokens
    one_byte_full, one_byte_full_7   one repeated byte: items of one to three bits, fewer bits than the header has,
                        most waves without any; with seven bytes more, a second block of the same kind
    two_symbols         two byte values and no match: literals of one and two bits
    deep_long_items     literal/length lengths reach 15, distance lengths 13; one match has 5 extra length bits and 13
                        extra distance bits: an item of 46 bits
    match_every_group   a literal, then a copy of four earlier bytes, over and over: a match in every group of four tokens
    random_block        bench.py's random64 leg, its first block: a match in about one group in 150, so a wave packs
                        some of its groups as literals and some item by item

No bytes are stored: numpy's generators and the library's make them again.  tests/test_emit_cases_cpu.py proves with the
oracle that every case sits where its name says."""
import numpy as np

import _encoder_cases as ec
import _oracle

BLK = ec.BLK
EMIT_WAVE_RUN = 512  # W: tokens of a tile that one wave owns (EMIT_WAVE_RUN of zes_deflate.hip)
EMIT_TILE = 8192     # T: tokens per tile (EMIT_TILE of zes_deflate.hip)
W, T = EMIT_WAVE_RUN, EMIT_TILE

COUNTS = [2, 5, 255, 256, 257, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 3]
BATCH = ["match_every_group", "ntok_%d" % (T + 1), "one_byte_full_7"]  # three buffers of unlike kinds and lengths

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_XBITS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_XBITS = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]

# deep_long_items: the far match (position, distance, length) and the planted 3-byte matches (count per distance code)
DEEP_FAR = (96000, 24600, 140)
DEEP_CODES = list(range(7, 20))
DEEP_PLANTS = [1, 2, 3, 5, 9, 16, 29, 50, 88, 154, 270, 472, 826]  # each more than 1.618 times the one before: one code tree


def is_match(tok):
    return (tok & 0x80000000) != 0


def token_positions(tok):
    """Byte position of every token inside its block."""
    step = np.where(is_match(tok), ((tok >> 16) & 0xFF).astype(np.int64) + 3, 1)
    return np.concatenate([[0], np.cumsum(step)[:-1]])


def item_bits(tok):
    """(literal/length code lengths, distance code lengths, bits of every token's item, extra length bits, extra distance
    bits) of a block with these tokens, the lengths by the oracle's restatement of the reference's code builder."""
    m = is_match(tok)
    ln, ds = ((tok[m] >> 16) & 0xFF).astype(np.int64) + 3, (tok[m] & 0x7FFF).astype(np.int64) + 1
    lc, dc = np.searchsorted(LEN_BASE, ln, side="right") - 1, np.searchsorted(DIST_BASE, ds, side="right") - 1
    hl, hd = np.zeros(286, dtype=np.uint32), np.zeros(30, dtype=np.uint32)
    np.add.at(hl, tok[~m].astype(np.int64), 1)
    np.add.at(hl, 257 + lc, 1)
    np.add.at(hd, dc, 1)
    hl[256] = 1
    ll, dl = _oracle.huff_lengths(hl, 15).astype(np.int64), _oracle.huff_lengths(hd, 15).astype(np.int64)
    bits = np.zeros(tok.size, dtype=np.int64)
    lx, dx = np.asarray(LEN_XBITS)[lc], np.asarray(DIST_XBITS)[dc]
    bits[~m] = ll[tok[~m].astype(np.int64)]
    bits[m] = ll[257 + lc] + lx + dl[dc] + dx
    xl, xd = np.zeros(tok.size, dtype=np.int64), np.zeros(tok.size, dtype=np.int64)
    xl[m], xd[m] = lx, dx
    return ll, dl, bits, xl, xd


def group_has_match(tok):
    """Per complete group of four tokens: does it hold a match."""
    n = tok.size // 4 * 4
    return is_match(tok[:n]).reshape(-1, 4).any(axis=1)


def _match_every_group(z):
    fresh = z.gen("xorshift", 9, BLK)
    rng = np.random.default_rng(5)
    buf = [97, 98, 99, 97, 98, 99]
    i = 0
    while len(buf) < BLK - 16:
        buf.append(int(fresh[i]))
        i += 1
        p = int(rng.integers(max(0, len(buf) - 3000), len(buf) - 4))
        buf.extend(buf[p: p + 4])
    return np.array(buf, dtype=np.uint8)


def _deep_long_items(z):
    """Literal counts that double from level to level (as ec's deep_code_far_match, three times over), 3-byte matches
    planted with DEEP_PLANTS[i] copies at the first distance of code DEEP_CODES[i], and the far match.  Matches the bytes
    hold by accident, and plants that found another candidate, are then broken one byte at a time."""
    counts = [1, 2, 4, 8, 16, 32, 64] + [64] * 2 + [64] * 4 + [64] * 8 + [128] * 8 + [128] * 16 + [256] * 16 + [256] * 32 + [256] * 64
    a = np.repeat(np.arange(len(counts), dtype=np.uint8), 3 * np.array(counts))
    a = ec._no_repeat(z, 332, a[np.argsort(ec._rnd32(z, 331, a.size), kind="stable")])
    q, d, length = DEEP_FAR
    a[q: q + length] = a[q - d: q - d + length]
    keep = list(range(q - d - 1, q - d + length + 1)) + list(range(q - 1, q + length + 1))
    planted = {q}
    slots = [x for x in range(1000, q - 100, 41) if not q - d - 100 <= x < q - d + 200]  # (no distance is within 5 of a multiple of 41)
    np.random.default_rng(1).shuffle(slots)
    for cnt, code in zip(DEEP_PLANTS, DEEP_CODES):
        dd = DIST_BASE[code]
        for _ in range(cnt):
            s = slots.pop(0)
            a[s: s + 3] = a[s - dd: s - dd + 3]
            keep += list(range(s - dd - 1, s - dd + 4)) + list(range(s - 1, s + 4))
            planted.add(s)
    a = ec._no_repeat(z, 333, a, keep=keep).copy()
    rng = np.random.default_rng(9)
    for _ in range(8):
        tok = _oracle.lz77_block(a, 0, a.size)
        m = is_match(tok)
        far = ((tok & 0x7FFF).astype(np.int64) + 1) > 1024
        stray = [int(p) for p, f in zip(token_positions(tok)[m], far[m]) if (int(p) not in planted or f) and int(p) != q]
        if not stray:
            return a
        for p in stray:
            if q - 10 <= p < q + length + 10:
                continue
            v = rng.integers(100, 150)
            a[p + 1] = v
            if q - d - 10 <= p < q - d + length + 10:
                a[p + 1 + d] = v
    raise AssertionError("accidental matches remain")


def cases(z):
    """name -> bytes."""
    out = {}
    for n in COUNTS:
        out["ntok_%d" % n] = ec._unique(z, 800 + n % 89, n)
    out["literals_full"] = ec._unique(z, 811, BLK)
    out["literals_two_blocks_5"] = ec._unique(z, 812, 2 * BLK + 5)
    out["one_byte_full"] = np.full(BLK, 0x41, dtype=np.uint8)
    out["one_byte_full_7"] = np.full(BLK + 7, 0x41, dtype=np.uint8)
    out["two_symbols"] = np.frombuffer(b"aaababbbaa", dtype=np.uint8).copy()  # every 3-letter word over {a, b} once
    out["deep_long_items"] = _deep_long_items(z)
    out["match_every_group"] = _match_every_group(z)
    out["random_block"] = z.gen("xorshift", 12345, BLK)
    for a in out.values():
        a.setflags(write=False)
    return out
