"""The segmented Adler-32 kernel's arithmetic, restated with Python integers, and the case list its tests share.

k_adler_seg (zlib.es_amd/csrc/zes_deflate.hip) cuts a segment into chunks at 64 KiB steps of memory, counted from the
16-byte boundary at or below the segment's first byte.  A chunk that covers the segment offsets [s, e) of a len-byte
segment adds

    A_c mod 65521                                  to the segment's first sum,  A_c = sum of b[j],
    (B_c + A_c * ((len - e) mod 65521)) mod 65521  to its second,               B_c = sum of (e - j) * b[j],  s <= j < e

and the host finishes: s1 = (1 + sum0) mod 65521, s2 = (len mod 65521 + sum1) mod 65521, adler = s2 << 16 | s1.  A segment
of no bytes has no chunk and the value 1.
"""
import numpy as np

MOD = 65521
CHUNK = 65536

ALIGNS = (0, 1, 7, 8, 15)
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4095, 65519, 65520, 65521, 65535, 65536, 65537, 131072 + 3, 200000)

# the arena: zeros, then 0xFF, then xorshift bytes up to the last byte (every region starts on a 16-byte boundary)
ARENA = 1 << 20
ZERO_AT, FF_AT, XS_AT = 0, 262144, 589824


def chunks(addr, n):
    """The (s, e) segment offsets of the chunks of an n-byte segment whose first byte has the address `addr`."""
    if n == 0:
        return []
    end = addr + n
    lo, top = addr & ~15, (end + 15) & ~15
    out = []
    while lo < top:
        hi = min(lo + CHUNK, top)
        out.append((max(addr, lo) - addr, min(end, hi) - addr))
        lo += CHUNK
    return out


def adler_by_chunks(data, addr):
    """Adler-32 of `data` (a uint8 array) as the kernel and the host compute it for a segment at address `addr`."""
    n = int(data.size)
    sum0 = sum1 = 0
    for s, e in chunks(addr, n):
        b = data[s:e].astype(np.int64)
        a_c = int(b.sum())
        b_c = int((b * np.arange(e - s, 0, -1, dtype=np.int64)).sum())  # (e - j for j = s .. e - 1; below 2^40 for 64 KiB of 0xFF)
        sum0 += a_c % MOD
        sum1 += (b_c + a_c * ((n - e) % MOD)) % MOD
    return ((n % MOD + sum1) % MOD) << 16 | (1 + sum0) % MOD


def arena(gen_xorshift):
    """The arena's bytes; gen_xorshift(n) gives n xorshift bytes."""
    a = np.zeros(ARENA, dtype=np.uint8)
    a[FF_AT:XS_AT] = 0xFF
    a[XS_AT:] = gen_xorshift(ARENA - XS_AT)
    return a


def grid():
    """(label, offset, length) of the alignment x length grid over the three contents, and the 0xFF case whose
    `len - e` passes 65521."""
    out = []
    for name, base in (("zero", ZERO_AT), ("ff", FF_AT), ("xorshift", XS_AT)):
        for a in ALIGNS:
            # ... and the lengths that put the end on, one below and one above a 64 KiB step counted from the aligned start
            for n in LENGTHS + (65536 - a - 1, 65536 - a, 65536 - a + 1, 131072 - a):
                out.append(("%s+%d,%d" % (name, a, n), base + a, n))
    for a in ALIGNS:
        out.append(("ff+%d,300000" % a, FF_AT + a, 300000))
    return out


def overlapping():
    """Overlapping and identical segments, and one that ends at the arena's last byte."""
    return [("same", XS_AT + 5, 70000), ("same again", XS_AT + 5, 70000), ("inside", XS_AT + 100, 1000), ("across", XS_AT + 60000, 20000),
            ("over the ff/xorshift border", XS_AT - 33, 100), ("to the last byte", ARENA - 70001, 70001), ("the last byte", ARENA - 1, 1)]


def many_short(count=3000):
    """`count` segments of 1 to 40 bytes at every alignment."""
    out, pos = [], XS_AT + 3
    for i in range(count):
        n = 1 + (i * 7) % 40
        out.append(("short%d" % i, pos, n))
        pos += n + (i % 3)
    assert pos <= ARENA
    return out
