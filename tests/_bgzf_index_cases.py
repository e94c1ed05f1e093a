"""Files and expectations shared by the BGZF index and range-read tests.  Plain Python, no GPU.

The expected index of a blob is tests/_bgzf.py's walk plus the ISIZE fields read with struct; nothing here comes from the
library under test.
"""
import ctypes as C
import struct

import numpy as np

import _bgzf
import _bgzip_expect

RAGGED = (1, 15, 16, 17, 0, 4096, 65280, 33)
RAGGED_LEVELS = [0, 1, 6, 9, 0, 1, 6, 9]
WRITER_SIZES = (0, 1, 65281, 2 * 65280 + 1)
GZIP_KINDS = ("bsize_plus", "bsize_minus", "pad_between", "trailing_zeros", "plain_middle", "cut_trailer", "garbage")
OK_KINDS = ("crc_flip", "body_bit", "isize_wrong")


def expected(blob):
    """(coff, uoff) of a BGZF file: members + 1 entries each."""
    ms = _bgzf.walk(blob)
    coff = [p for p, _, _ in ms] + [len(blob)]
    uoff = [0]
    for p, s, _ in ms:
        uoff.append(uoff[-1] + struct.unpack_from("<I", blob, p + s - 4)[0])
    return np.array(coff, dtype=np.uint64), np.array(uoff, dtype=np.uint64)


def text(n, seed=7):
    """n bytes that compress, without a GPU and without the library."""
    rng = np.random.default_rng(seed)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"member", b"index", b"range", b" ", b"\n", b"0123456789"]
    out = b"".join(words[i] for i in rng.integers(0, len(words), n // 3 + 8))
    return out[:n]


def ragged():
    a = text(sum(RAGGED))
    chunks, p = [], 0
    for n in RAGGED:
        chunks.append(a[p:p + n])
        p += n
    return _bgzf.bgzf(chunks, level=RAGGED_LEVELS), a


FAKE_AT = 18 + 5 + 40  # where the fake header of fake_header_file lies: behind the member's header, the stored block's five bytes and 40 payload bytes


def fake_header_file(exact):
    """A stored (level 0) member whose payload holds a complete qualifying 18-byte BGZF header at FAKE_AT, then a real data
    member and the marker.  exact: the fake header's size ends exactly where the next real member starts; else it leads
    into the middle of the next member."""
    filler = text(300, 9)
    payload_len = 40 + 18 + len(filler)
    first_size = 18 + 5 + payload_len + 8
    size = first_size - FAKE_AT if exact else first_size - FAKE_AT + 11
    fake = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", size - 1)
    payload = b"p" * 40 + fake + filler
    m0 = _bgzf.member(payload, _bgzf.raw_body(payload, 0))
    assert len(m0) == first_size and m0[FAKE_AT:FAKE_AT + 18] == fake
    rest = _bgzf.bgzf([text(5000, 10)])
    return m0 + rest, payload + text(5000, 10)


def bare_signature_file():
    """A stored member whose payload holds 1f 8b 08 04 followed by bytes that do not qualify (XLEN too long; no BC subfield)."""
    payload = b"q" * 7 + b"\x1f\x8b\x08\x04" + b"\xff" * 30 + b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00XY\x02\x00\x30\x00" + b"r" * 100
    return _bgzf.bgzf([payload, text(100, 11)], level=[0, 6]), payload + text(100, 11)


def files():
    """name -> (blob, uncompressed bytes): every valid file of the index tests."""
    out = {}
    out["marker_alone"] = (_bgzf.bgzf([]), b"")
    one = text(3000, 3)
    out["one_member_no_marker"] = (_bgzf.bgzf([one], eof=False), one)
    out["ragged"] = ragged()
    sub = [text(1000, 4), text(16, 5), text(1984, 6)]
    out["other_subfields"] = (_bgzf.bgzf(sub, extra_before=b"XY\x03\x00abc", extra_after=b"ZZ\x00\x00Q1\x05\x00hello"), b"".join(sub))
    for n in WRITER_SIZES:
        x = text(n, 20 + n % 7)
        out["writer_%d" % n] = (_bgzip_expect.expect(x), x)
    out["fake_header_nowhere"] = fake_header_file(False)
    out["fake_header_exact"] = fake_header_file(True)
    return out


def damage_chunks():
    a = text(3000 + 20000 + 17 + 1234, 12)
    cuts = (0, 3000, 23000, 23017, len(a))
    return [a[cuts[i]:cuts[i + 1]] for i in range(4)]


def c_index(fn, ptr, c, flags=0, cap=None):
    """One zes_bgzf_index* call with arrays of `cap` entries (None: ask for the count first and size them by it) ->
    (status, members, coff, uoff); the arrays are filled with a pattern beforehand."""
    m = C.c_uint64(0xDEAD)
    if cap is None:
        rc = fn(ptr, c, None, None, 0, C.byref(m), flags)
        if rc != -16:  # ZES_E_NOSPACE: the count query's answer on a valid file
            return rc, m.value, None, None
        cap = m.value + 1
    coff = np.full(max(cap, 1), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    uoff = coff.copy()
    rc = fn(ptr, c, coff.ctypes.data, uoff.ctypes.data, cap, C.byref(m), flags)
    return rc, m.value, coff[:cap], uoff[:cap]
