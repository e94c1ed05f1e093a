"""The gzip batch forms' tests (include/zes.h: "zes_gzip_batch*", "zes_gunzip_batch*"), in plain Python: the file the writer
must give, assembled with numpy from header, body and trailer — the body is the single-file form's own (z.gzip on the GPU,
the CPU oracle's raw stream elsewhere: the same bytes) or the stored form — and the case lists that the CPU and the GPU tests
walk: the writer's lengths, the reader's files for the batched route, and the files that the per-file route must judge, each
with the verdict CPython's gzip.decompress gives it."""
import functools
import gzip
import struct
import zlib

import numpy as np

import _bgzip_expect
import _oracle

BLK = 131072
PIECES, SERIAL = 4, 32  # ZES_F_PIECES, ZES_F_GZIP_SERIAL
OK, NOSPACE, E_GZIP, E_CHECKSUM, E_UNSUPPORTED, E_ARG, E_DEVICE = 0, -16, -20, -21, -23, -18, -17
HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
STORED_BLOCK = 65535
LENGTHS = (0, 1, 2, 17, 65535, 65536, 131072, 131073, 300000)
BOUNDS = {0: 23, 1: 24, 65535: 65558, 65536: 65564, 131070: 131098, 131071: 131104}  # 18 + n + 5 * max(1, ceil(n / 65535))


def throws(n):
    return n == 0 or n == 1 or n % BLK == 1


def bound(n):
    return 18 + n + 5 * max(1, -(-n // STORED_BLOCK))


def stored_body(data):
    """The stored form: blocks of 65535 bytes, BFINAL on the last; no bytes: 01 00 00 ff ff."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    nb = max(1, -(-a.size // STORED_BLOCK))
    parts = []
    for b in range(nb):
        chunk = a[b * STORED_BLOCK:(b + 1) * STORED_BLOCK]
        head = np.frombuffer(struct.pack("<BHH", 1 if b + 1 == nb else 0, chunk.size, chunk.size ^ 0xFFFF), dtype=np.uint8)
        parts += [head, chunk]
    return np.concatenate(parts)


def oracle_raw(data):
    return _oracle.deflate_raw(np.frombuffer(bytes(data), dtype=np.uint8))


def expect(data, raw=oracle_raw):
    """(file, kind) for one buffer: kind "stream", "longer" (stored because the stream is not shorter), "refused" (stored because
    the encoder refuses the length).  raw(data) -> the single-file form's body."""
    data = bytes(data)
    st = stored_body(data)
    kind = "refused"
    body = st
    if not throws(len(data)):
        s = np.asarray(raw(data), dtype=np.uint8)
        kind, body = ("stream", s) if s.size < st.size else ("longer", st)
    trailer = np.frombuffer(struct.pack("<II", zlib.crc32(data), len(data)), dtype=np.uint8)
    return np.concatenate([np.frombuffer(HEADER, dtype=np.uint8), body, trailer]).tobytes(), kind


@functools.lru_cache(maxsize=None)
def _writer_cases(z):
    out = []
    for n in LENGTHS:
        out.append(("text %d" % n, z.gen("itext", 700 + n % 89, n).tobytes()))
    for n in LENGTHS:
        out.append(("random %d" % n, z.gen("xorshift", 800 + n % 89, n).tobytes()))
    return tuple(out)


def writer_cases(z):
    """[(name, data)]: the writer's case list, text and random bytes of every length of LENGTHS."""
    return list(_writer_cases(z))


def nine(z):
    """Nine buffers for ZES_F_PIECES: groups of four meet twice and the last group holds one."""
    c = dict(writer_cases(z))
    return [(k, c[k]) for k in ("text 17", "random 65536", "text 1", "text 131072", "random 2", "text 131073", "text 65535", "text 0", "text 300000")]


# ---- the reader's files ----
def header(extra=None, name=None, comment=None, fhcrc=None, flg=0, cm=8, magic=b"\x1f\x8b"):
    """A member's header.  extra: the extra field's bytes; name, comment: without their NUL; fhcrc: None, "right" or "wrong"."""
    flg |= (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if fhcrc else 0)
    h = magic + bytes([cm, flg, 0, 0, 0, 0, 0, 0xFF])
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if fhcrc:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) ^ (0 if fhcrc == "right" else 0x0100))
    return h


def raw6(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def member(data, head=HEADER, body=None, crc=None, isize=None):
    body = raw6(data) if body is None else body
    return head + body + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def ref_gzip(data):
    """z.gzip(data), from the CPU oracle."""
    return member(data, body=oracle_raw(data).tobytes())


SUB = b"XY\x03\x00abc"  # an extra subfield that is not 'B','C'


@functools.lru_cache(maxsize=None)
def _texts(z):
    g = lambda seed, n: z.gen("itext", seed, n).tobytes()
    return {"a": g(901, 40003), "b": g(902, 65536), "c": g(903, 150001), "d": g(904, 4096), "e": g(905, 1000)}


def good_files(z):
    """[(name, file, plain)]: single members that the batched route must finish.  CPython's streams take the segment-parallel
    tier and the oracle's (z.gzip's bytes) the block-parallel one; the outputs' sizes are and are not multiples of 16."""
    t = _texts(z)
    out = [("gzip.compress level %d" % lv, gzip.compress(t[k], lv, mtime=0), t[k]) for lv, k in ((1, "a"), (6, "b"), (9, "d"))]
    out.append(("z.gzip, two blocks", ref_gzip(t["c"]), t["c"]))
    out.append(("z.gzip, 4096 bytes", ref_gzip(t["d"]), t["d"]))
    out.append(("FEXTRA", member(t["e"], header(extra=SUB)), t["e"]))
    out.append(("FNAME", member(t["e"], header(name=b"shard-0001.log")), t["e"]))
    out.append(("FCOMMENT", member(t["d"], header(comment=b"made by hand")), t["d"]))
    out.append(("FEXTRA, FNAME and FCOMMENT", member(t["a"], header(extra=SUB + SUB, name=b"n", comment=b"")), t["a"]))
    out.append(("an empty output", gzip.compress(b"", 6, mtime=0), b""))
    return out


def serial_files(z):
    """[(name, file, verdict, cap_delta)]: files that only the per-file route can judge.  verdict: what CPython 3's
    gzip.decompress gives, the bytes or None for an exception (it skips FHCRC and the reserved FLG bits, which zes_gunzip
    checks, and answers b"" for no input; the tests compare the library with its own single-file form).  cap_delta: the
    output's capacity relative to its size (device form)."""
    t = _texts(z)
    a, e = t["a"], t["e"]
    good = gzip.compress(a, 6, mtime=0)
    small = member(e)
    named = member(e, header(name=b"some-name"))
    flipped = bytearray(good)
    flipped[len(good) // 2] ^= 0x10
    forty = member(b"tiny", header(extra=b"Z" * (40 - 12 - len(raw6(b"tiny")) - 8)))  # (an extra field pads it to 40 bytes)
    assert len(forty) == 40
    bg = bytes(z.gen("itext", 906, 2 * _bgzip_expect.CHUNK + 777))
    out = [
        ("two members", small + member(t["d"]), e + t["d"], 0),
        ("a BGZF file of 3 members and the marker", _bgzip_expect.expect(bg), bg, 0),
        ("trailing zero bytes", small + bytes(5), e, 0),
        ("FHCRC right", member(e, header(name=b"x", fhcrc="right")), e, 0),
        ("FHCRC wrong", member(e, header(name=b"x", fhcrc="wrong")), e, 0),
        ("an FNAME of 300 bytes", member(e, header(name=b"n" * 300)), e, 0),
        ("bad magic", member(e, header(magic=b"\x1f\x8c")), None, 0),
        ("CM 9", member(e, header(cm=9)), None, 0),
        ("a reserved FLG bit", member(e, header(flg=0x20)), e, 0),
        ("no bytes", b"", b"", 0),
        ("10 bytes", small[:10], None, 0),
        ("17 bytes", small[:17], None, 0),
        ("cut inside the header", named[:14], None, 0),
        ("cut inside the body", good[:len(good) // 2], None, 0),
        ("cut inside the trailer", good[:-3], None, 0),
        ("one flipped body bit", bytes(flipped), None, 0),
        ("a wrong CRC", member(e, crc=zlib.crc32(e) ^ 1), None, 0),
        ("ISIZE one less", member(e, isize=len(e) - 1), None, 0),
        ("ISIZE one more", member(e, isize=len(e) + 1), None, 0),
        ("ISIZE 0xFFFFFFF0", member(e, isize=0xFFFFFFF0), None, 0),
        ("40 bytes claiming 0xFFFFFFF0", forty[:-4] + struct.pack("<I", 0xFFFFFFF0), None, 0),
        ("out_cap one short", good, a, -1),
    ]
    return out


def forty_good(z):
    """A good file of 40 bytes (the yardstick of the lying-ISIZE test) and its plain bytes."""
    f = next(x for x in serial_files(z) if x[0].startswith("40 bytes"))[1]
    return f[:-4] + struct.pack("<I", 4), b"tiny"


def py_verdict(blob):
    try:
        return gzip.decompress(blob)
    except (OSError, EOFError, zlib.error):
        return None
