"""Inputs, maps and recorded damage for the tests of the piecewise paths (zes_deflate_range_dev, zes_inflate_range_dev,
the pipelined host inflate).  Everything expected comes from the oracle: its map of a stream's blocks
(oracle.inflate_blocks), its block-range encoder (oracle.deflate_range) and oracle.inflate of a damaged stream.

The damage positions were chosen with the oracle alone, on a CPU, and are literals here together with the outcome they
were chosen for; tests/test_seam_damage_cpu.py holds the oracle to these outcomes without a GPU.
"""
import zlib

import numpy as np

BLOCK = 131072

# ---- zes_inflate_range_dev: three streams, every block start a seam --------------------------------------------------
RANGE_STREAMS = {  # kind: (seed, bytes)
    "itext": (501, 6 * BLOCK + 999),     # ~46 KiB of stream per block, a short final block
    "xorshift": (502, 5 * BLOCK + 2),    # ~128 KiB of stream per block (incompressible), a 2-byte final block
    "lowent4k": (503, 12 * BLOCK),       # ~5 KiB of stream per block: several block starts per KiB-sized piece
}
# One flipped bit in the last quarter of block k's bits (its body, behind the header), k neither first nor final, chosen
# so that oracle.inflate of the stream fails or gives another length: (k, stream bit, outcome).
RANGE_FLIPS = {
    "itext": ((5, 2252303, ("out", 787432, 978588813)), (2, 1101956, ("out", 787429, 3361882348)), (4, 1827396, ("out", 787445, 811410155))),
    "xorshift": ((1, 1953824, ("out", 655366, 1770130924)), (2, 2992536, ("err", -3)), (4, 5123462, ("err", -2))),
    "lowent4k": ((3, 158693, ("out", 1572095, 3929775200)), (9, 410461, ("out", 1572095, 248593194)), (4, 197313, ("out", 1573377, 3671918049))),
}

# ---- the pipelined host inflate: the smallest streams that enter it (8 MiB) ------------------------------------------
PIPE_INPUTS = {  # name: (kind, seed, bytes, stream bytes)
    "xorshift9": ("xorshift", 601, (9 << 20) + 12345, 9459031),   # a block is ~128 KiB of stream: piece boundaries fall inside blocks
    "itext24": ("itext", 602, (24 << 20) + 4097, 8943105),        # a block is ~45 KiB of stream: some twenty block starts per MiB piece
    "xorshift13": ("xorshift", 603, (13 << 20) + 7, 13645201),    # two thirds of it are still above 8 MiB
}
# (input, name, ("flip", stream bit) | ("cut", bytes kept), oracle outcome).  "first" lies in the stream's first MiB,
# "middle" within 300 KB of its half, "last" in its last 600 KB: with 1 MiB pieces the first, a middle and the last piece.
# "_byte" flips change one literal (the stream still chains), "_break" flips sit in a block's header and end the decode
# or change its length.
PIPE_DAMAGE = (
    ("xorshift9", "first_byte", ("flip", 2672353), ("out", 9449529, 1876872461)),
    ("xorshift9", "first_break", ("flip", 6297760), ("err", -3)),
    ("xorshift9", "middle_byte", ("flip", 35449407), ("out", 9449529, 2503003412)),
    ("xorshift9", "middle_break", ("flip", 37786840), ("err", -3)),
    ("xorshift9", "last_byte", ("flip", 73040172), ("out", 9449529, 3395734764)),
    ("xorshift9", "last_break", ("flip", 73474103), ("out", 9177122, 517873512)),
    ("xorshift9", "cut_two_thirds", ("cut", 6306020), ("err", -5)),
    ("xorshift9", "cut_3_before_end", ("cut", 9459028), ("out", 9449529, 1324731660)),
    ("itext24", "first_longer", ("flip", 2536957), ("out", 25169922, 3893078195)),
    ("itext24", "first_break", ("flip", 5588842), ("err", -3)),
    ("itext24", "middle_byte", ("flip", 37631672), ("out", 25169921, 341501239)),
    ("itext24", "middle_break", ("flip", 37624958), ("err", -3)),
    ("itext24", "last_byte", ("flip", 69155405), ("out", 25169921, 3825519366)),
    ("itext24", "last_break", ("flip", 67058657), ("err", -4)),
    ("itext24", "cut_two_thirds", ("cut", 5962070), ("err", -5)),
    ("itext24", "cut_3_before_end", ("cut", 8943102), ("out", 25169921, 3012414217)),
    ("xorshift13", "middle_ends_early", ("flip", 56680379), ("out", 7078776, 2934962474)),
    ("xorshift13", "cut_two_thirds", ("cut", 9096800), ("err", -5)),  # (the cut stream is itself above 8 MiB)
)


def flip(comp, bit):
    d = comp.copy()
    d[bit >> 3] ^= 1 << (bit & 7)
    return d


def damaged(comp, how):
    return flip(comp, how[1]) if how[0] == "flip" else comp[: how[1]].copy()


def outcome(oracle, comp):
    """("out", length, adler32) or ("err", code) of oracle.inflate, and the bytes (None on an error)."""
    try:
        b = oracle.inflate(comp)
    except oracle.OracleError as e:
        return ("err", e.code), None
    return ("out", len(b), zlib.adler32(b.tobytes())), b


class Stream:
    """A reference-made stream with its map: starts[k] the bit block k starts at, ends[k] the output length behind it,
    end_bit the bit behind the final block (16 + the bits oracle.deflate_range gives for the whole input)."""

    def __init__(self, z, oracle, kind, seed, n):
        self.kind, self.n = kind, n
        self.a = z.gen(kind, seed, n)
        self.comp = oracle.deflate(self.a)
        self.starts, self.ends = oracle.inflate_blocks(self.comp)
        self.end_bit = 16 + oracle.deflate_range(self.a, 0, n, True)[1]
        assert len(self.starts) == (n + BLOCK - 1) // BLOCK and self.ends[-1] == n
        assert (self.end_bit + 7) // 8 == len(self.comp) - 4  # (the Adler-32 trailer follows the last byte with bits)

    def owned(self, lo, own):
        return [k for k, s in enumerate(self.starts) if lo <= s < own]

    def expect(self, lo, own, exact):
        """What a call over [lo, own) must report by the header's half-open rule alone; None: ZES_E_NOTRANGE (exact_start on a
        bit where no block starts)."""
        ks = self.owned(lo, own)
        if exact and lo not in self.starts:
            return None
        if not ks:
            return {"nblocks": 0, "out_len": 0, "first_bit": lo, "end_bit": lo, "final": 0, "out_lo": 0}
        last = ks[-1] == len(self.starts) - 1
        out_lo = self.ends[ks[0] - 1] if ks[0] else 0
        return {"nblocks": len(ks), "out_len": self.ends[ks[-1]] - out_lo, "first_bit": self.starts[ks[0]],
                "end_bit": self.end_bit if last else self.starts[ks[-1] + 1], "final": int(last), "out_lo": out_lo}


def range_stream(z, oracle, kind):
    seed, n = RANGE_STREAMS[kind]
    return Stream(z, oracle, kind, seed, n)


# ---- zes_deflate_range_dev: inputs whose matches run up to and across a range boundary -------------------------------
DEFLATE_N = 3 * BLOCK + 777
DEFLATE_INPUTS = ("one_byte", "period258", "period259", "period32768", "lowent4k")


def deflate_input(z, name):
    if name == "one_byte":
        return np.full(DEFLATE_N, 0x61, dtype=np.uint8)
    if name == "lowent4k":
        return z.gen("lowent4k", 701, DEFLATE_N)
    period = int(name[len("period"):])
    return np.resize(z.gen("xorshift", 700 + period % 97, period), DEFLATE_N).copy()
