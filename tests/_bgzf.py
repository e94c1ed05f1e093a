"""BGZF files built by hand, and ways to damage them.  Plain Python, no GPU.

A BGZF file (bgzip / htslib) is valid gzip: a run of members of at most 64 KiB, each stating its own size in a 'B','C'
extra subfield (BSIZE = member size - 1), usually closed by an empty member, the end-of-file marker.
"""
import struct
import zlib

EOF_BODY = b"\x03\x00"


def raw_body(data, level=6, strategy=0):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


def member(data, body, extra_before=b"", extra_after=b"", bsize_delta=0):
    """One member around a raw DEFLATE body; the 18-byte header 1f 8b 08 04 00000000 00 ff XLEN 42 43 02 00 BSIZE when
    there are no other subfields."""
    xlen = len(extra_before) + 6 + len(extra_after)
    size = 12 + xlen + len(body) + 8
    assert size <= 65536, "a BGZF member holds at most 64 KiB (BSIZE is 16 bits): %d" % size
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra_before \
        + b"BC\x02\x00" + struct.pack("<H", (size - 1 + bsize_delta) & 0xFFFF) + extra_after
    return head + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def bgzf_members(chunks, level=6, strategy=0, extra_before=b"", extra_after=b"", eof=True, bodies=None):
    """The members of bgzf(...), one bytes object each.  level and strategy: one value, or one per chunk; bodies: raw
    DEFLATE bodies made elsewhere, one per chunk (None: zlib makes it)."""
    per = lambda v, i: v[i] if isinstance(v, (list, tuple)) else v
    out = []
    for i, data in enumerate(chunks):
        data = bytes(data)
        body = bodies[i] if bodies is not None and bodies[i] is not None else raw_body(data, per(level, i), per(strategy, i))
        out.append(member(data, bytes(body), extra_before, extra_after))
    if eof:
        out.append(member(b"", EOF_BODY, extra_before, extra_after))
    return out


def bgzf(chunks, level=6, strategy=0, extra_before=b"", extra_after=b"", eof=True, bodies=None):
    return b"".join(bgzf_members(chunks, level, strategy, extra_before, extra_after, eof, bodies))


def walk(blob):
    """(position, size, header length) of every member, following BSIZE as a BGZF reader does."""
    out, pos = [], 0
    while pos < len(blob):
        assert blob[pos:pos + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", blob, pos + 10)[0]
        p, end, size = pos + 12, pos + 12 + xlen, None
        while p < end:
            si, sl = blob[p:p + 2], struct.unpack_from("<H", blob, p + 2)[0]
            if si == b"BC" and sl == 2 and size is None:
                size = struct.unpack_from("<H", blob, p + 4)[0] + 1
            p += 4 + sl
        assert p == end and size is not None
        out.append((pos, size, 12 + xlen))
        pos += size
    assert pos == len(blob)
    return out


def plain_member(data, level=6):
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw_body(data, level) + struct.pack("<II", zlib.crc32(data), len(data))


# what CPython's gzip.decompress still reads (to the same bytes) / what it raises on
DECODABLE = ("bsize_plus", "bsize_minus", "pad_between", "trailing_zeros", "plain_middle")
RAISING = ("crc_flip", "isize_wrong", "body_bit", "cut_trailer", "garbage")


def damage(chunks, kind):
    """A file of `chunks` (at least three) plus the end-of-file marker, damaged in or around its middle member.
    Returns (blob, position of the damaged member's body or None)."""
    ms = bgzf_members(chunks)
    mid = len(chunks) // 2
    body_at = sum(len(m) for m in ms[:mid]) + 18
    flip = lambda m, at, bit: m[:at] + bytes([m[at] ^ bit]) + m[at + 1:]
    if kind in ("bsize_plus", "bsize_minus"):
        ms[mid] = member(bytes(chunks[mid]), raw_body(bytes(chunks[mid])), bsize_delta=1 if kind == "bsize_plus" else -1)
    elif kind == "pad_between":
        ms.insert(mid, b"\x00" * 5)
    elif kind == "trailing_zeros":
        ms.append(b"\x00" * 7)
    elif kind == "plain_middle":
        ms[mid] = plain_member(bytes(chunks[mid]))
    elif kind == "crc_flip":
        ms[mid] = flip(ms[mid], len(ms[mid]) - 7, 0x10)
    elif kind == "isize_wrong":
        ms[mid] = flip(ms[mid], len(ms[mid]) - 4, 0x01)
    elif kind == "body_bit":
        ms[mid] = ms[mid][:18] + bytes([ms[mid][18] | 0x06]) + ms[mid][19:]  # BTYPE 3: no inflate accepts it
    elif kind == "cut_trailer":
        ms[-1] = ms[-1][:-3]
    elif kind == "garbage":
        ms.append(b"\x01garbage")
    else:
        raise ValueError(kind)
    return b"".join(ms), (body_at if kind == "body_bit" else None)
