"""Synthetic piece lists for the two joins (shard.join_host on the CPU, zes_deflate_join_dev on the GPU) and the piece
lists of the Adler-32 combination, with what they must give by tests/_bitref.py and CPython's zlib.adler32.

A piece is kept as the device form wants it read: whole dwords up to the one that holds its last bit, one dword more,
and EVERY bit beyond its nbits set — the rest of the last byte, of the last dword and the dword behind it — so that a
join that forgets to mask the tail puts ones into its neighbour's bits.
"""
import importlib.util
import os
import zlib

import numpy as np

import _bitref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_shard():
    """zlib.es_amd/shard.py as a module of its own (the package directory has a dot in its name)."""
    spec = importlib.util.spec_from_file_location("zlibes_amd_shard", os.path.join(ROOT, "zlib.es_amd", "shard.py"))
    shard = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shard)
    return shard


TAILS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97)  # the middle piece of the shift sweep, in bits
WRAP_BYTES = (4 << 20) + 100  # above 4096 x 256 dwords: k_bits_place's grid-stride loop goes round twice
ADLER_MOD = 65521
ADLER_LENS = (1, 5551, 5552, 5553, 65520, 65521, 65522, 3 * 65521)
HUGE_ZERO_LENS = ((1 << 32) - 1, (1 << 32) + 5, 1 << 40)


def dirty(bits):
    """A piece of len(bits) bits as bytes: whole dwords plus one, every bit beyond the piece set."""
    n = int(len(bits))
    full = np.ones(32 * ((n + 31) // 32) + 32, dtype=np.uint8)
    full[:n] = bits
    return np.packbits(full, bitorder="little")


class JoinCase:
    """pieces[i]: dirty bytes (None: an empty piece handed over as a null pointer), nbits[i]; adlers[i] / lens[i]: the
    checksum and length of the input bytes piece i stands for; want: the joined zlib stream."""

    def __init__(self, name, bit_lists, rng):
        self.name = name
        self.nbits = [int(len(b)) for b in bit_lists]
        self.pieces = [dirty(b) if len(b) else None for b in bit_lists]
        datas = [rng.integers(0, 256, (7 * i) % 23 + 1 if len(b) else 0, dtype=np.uint8).tobytes() for i, b in enumerate(bit_lists)]
        self.adlers = [zlib.adler32(d) for d in datas]
        self.lens = [len(d) for d in datas]
        clean = [np.packbits(np.asarray(b, dtype=np.uint8), bitorder="little") for b in bit_lists]
        body, total = _bitref.concat_bits(clean, self.nbits)
        assert total == sum(self.nbits)
        self.want = _bitref.zlib_frame(body, zlib.adler32(b"".join(datas)))


def _bits(rng, n):
    return rng.integers(0, 2, n, dtype=np.uint8)


def shift_tail_cases():
    """Every seam shift against every tail: s random bits (left out for s = 0), L bits, 37 bits — 32 x 11 lists.  The body
    starts at bit 16 of the stream, so the L-bit piece lands at shift (16 + s) % 32: all 32 shifts."""
    rng = np.random.default_rng(20240601)
    out = []
    for s in range(32):
        for L in TAILS:
            lists = ([_bits(rng, s)] if s else []) + [_bits(rng, L), _bits(rng, 37)]
            out.append(JoinCase("s%d_L%d" % (s, L), lists, rng))
    return out


def many_short_cases():
    """300 pieces of 1..130 bits, three seeds: many sit wholly inside one destination dword, shared with both neighbours."""
    out = []
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        out.append(JoinCase("short300_seed%d" % seed, [_bits(rng, int(n)) for n in rng.integers(1, 131, 300)], rng))
    return out


def empty_piece_cases():
    """Pieces of no bits at the front, in the middle and at the end (null pointers), and a list of one piece."""
    rng = np.random.default_rng(77)
    e = np.zeros(0, dtype=np.uint8)
    return [JoinCase("empty_front", [e, _bits(rng, 45), _bits(rng, 70)], rng),
            JoinCase("empty_middle", [_bits(rng, 45), e, e, _bits(rng, 70)], rng),
            JoinCase("empty_end", [_bits(rng, 45), _bits(rng, 70), e], rng),
            JoinCase("empty_everywhere", [e, _bits(rng, 3), e, _bits(rng, 129), e], rng),
            JoinCase("single_13", [_bits(rng, 13)], rng),
            JoinCase("single_4099", [_bits(rng, 4099)], rng)]


def wrap_case():
    """One piece of 4 MiB + 100 bytes at shift 13 (29 bits in front of it: 16 + 29 = 45 = 32 + 13), then 5 bits."""
    rng = np.random.default_rng(4100)
    big = np.unpackbits(rng.integers(0, 256, WRAP_BYTES, dtype=np.uint8), bitorder="little")
    return JoinCase("wrap", [_bits(rng, 29), big, _bits(rng, 5)], rng)


def edge_cases():
    """Lists whose result length is 0, 1, 2 and 3 above a multiple of 4 (the output is written in whole dwords)."""
    rng = np.random.default_rng(99)
    out = []
    for body_bytes in (10, 11, 12, 13):  # result = 2 + body + 4 bytes
        out.append(JoinCase("edge_len%d" % (body_bytes + 6), [_bits(rng, 21), _bits(rng, 8 * body_bytes - 21 - 3)], rng))
    return out


def small_cases():
    """Everything but the 4 MiB piece: what the CPU test and the GPU sweep share."""
    return shift_tail_cases() + many_short_cases() + empty_piece_cases() + edge_cases()


# ---- Adler-32 of a concatenation ------------------------------------------------------------------------------------
def adler_zero(n):
    """Adler-32 of n zero bytes in closed form: s1 stays 1, s2 counts the bytes."""
    return ((n % ADLER_MOD) << 16) | 1


def adler_append_zeros(a, n):
    """Adler-32 of (bytes with checksum a) followed by n zero bytes: s1 stays, s2 grows by n * s1."""
    s1, s2 = a & 0xFFFF, a >> 16
    return (((s2 + (n % ADLER_MOD) * s1) % ADLER_MOD) << 16) | s1


def adler_lists():
    """[(name, [(adler, length), ...], adler of the concatenation)]: real byte strings at the lengths where s1 and s2 pass
    the modulus (0xFF bytes), stay at their floor (zeros) and in between (random), then zero-byte pieces too long to exist."""
    rng = np.random.default_rng(65521)
    out = []
    for cname in ("ff", "zero", "random"):
        bufs = []
        for n in ADLER_LENS:
            bufs.append(bytes([0xFF]) * n if cname == "ff" else bytes(n) if cname == "zero" else rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        lists = [("all", bufs), ("reversed", bufs[::-1])] + [("%d+%d" % (len(a), len(b)), [a, b]) for a in bufs for b in bufs]
        for lname, parts in lists:
            out.append(("%s_%s" % (cname, lname), [(zlib.adler32(p), len(p)) for p in parts], zlib.adler32(b"".join(parts))))
    for n in HUGE_ZERO_LENS:
        out.append(("zeros_%d" % n, [(adler_zero(n), n)], adler_zero(n)))
        for m in HUGE_ZERO_LENS:
            out.append(("zeros_%d+%d" % (n, m), [(adler_zero(n), n), (adler_zero(m), m)], adler_zero(n + m)))
        ff = bytes([0xFF]) * 65521
        a = zlib.adler32(ff)
        out.append(("ff65521+zeros_%d" % n, [(a, len(ff)), (adler_zero(n), n)], adler_append_zeros(a, n)))
    return out
