"""PNG files for the reader's tests, in pure Python and numpy: a writer that takes raw scanlines, a filter type per row, an
IDAT split plan and the zlib stream's maker; the forward filters; an independent unfilter (the oracle: plain byte loops
after the PNG specification, 9.2 to 9.4, sharing nothing with the forward side but the Paeth predictor's definition); the
file rule of include/zes.h restated; and the two case tables (geometry(), damage()) that the CPU and the GPU tests walk."""
import functools
import struct
import zlib

import numpy as np

ZES_E_NOSPACE, ZES_E_ARG, ZES_E_DEVICE, ZES_E_CHECKSUM, ZES_E_UNSUPPORTED, ZES_E_PNG = -16, -18, -17, -21, -23, -24
INFLATE_STATUSES = (-1, -2, -3, -4, -5)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
PAIRS = [(c, d) for c in sorted(DEPTHS) for d in DEPTHS[c]]
WIDTHS = (1, 2, 3, 5, 17, 63, 64, 65, 300)
HEIGHTS = (1, 2, 63, 64, 65, 128, 129, 200)
INFO_FIELDS = ("width", "height", "depth", "colour", "interlace", "channels", "bpp", "rowbytes", "out_size", "idat_count", "plte_len", "idat_bytes",
               "plte_pos", "trns_pos", "trns_len", "pad2")


def shape(width, height, colour, depth):
    """(bpp, rowbytes, out_size) as include/zes.h defines them."""
    bits = CHANNELS[colour] * depth
    rowbytes = (width * bits + 7) // 8
    return max(1, bits // 8), rowbytes, height * rowbytes


# ---------------------------------------------------------------------------------------------------------------------
# filters
# ---------------------------------------------------------------------------------------------------------------------
def _paeth_np(a, b, c):
    a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(raw, height, rowbytes, bpp, filters):
    """The filtered scanlines (a filter byte and rowbytes bytes a row) of `raw`, row r filtered by type filters[r]."""
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(height, rowbytes)
    out = np.zeros((height, 1 + rowbytes), dtype=np.uint8)
    zero = np.zeros(rowbytes, dtype=np.uint8)
    for r in range(height):
        x, b = rows[r], rows[r - 1] if r else zero
        a = np.concatenate([np.zeros(bpp, dtype=np.uint8), x[:-bpp]]) if rowbytes > bpp else np.zeros(rowbytes, dtype=np.uint8)
        c = np.concatenate([np.zeros(bpp, dtype=np.uint8), b[:-bpp]]) if rowbytes > bpp else np.zeros(rowbytes, dtype=np.uint8)
        a, c = a[:rowbytes], c[:rowbytes]
        ft = filters[r]
        pred = {0: zero.astype(np.int32), 1: a.astype(np.int32), 2: b.astype(np.int32), 3: (a.astype(np.int32) + b.astype(np.int32)) >> 1}.get(ft)
        if pred is None:
            assert ft == 4, ft
            pred = _paeth_np(a, b, c)
        out[r, 0] = ft
        out[r, 1:] = ((x.astype(np.int32) - pred) & 255).astype(np.uint8)
    return out.tobytes()


def unfilter(filtered, height, rowbytes, bpp):
    """The oracle: reconstruct byte by byte (PNG specification, 9.2).  None when a filter byte is above 4."""
    f = bytes(filtered)
    assert len(f) == height * (1 + rowbytes)
    out = bytearray(height * rowbytes)
    prev = bytes(rowbytes)
    for r in range(height):
        base = r * (1 + rowbytes)
        ft, line = f[base], f[base + 1:base + 1 + rowbytes]
        cur = bytearray(rowbytes)
        if ft > 4:
            return None
        for i in range(rowbytes):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if ft == 0:
                p = 0
            elif ft == 1:
                p = a
            elif ft == 2:
                p = b
            elif ft == 3:
                p = (a + b) // 2
            else:
                est = a + b - c
                pa, pb, pc = abs(est - a), abs(est - b), abs(est - c)
                p = a if pa <= pb and pa <= pc else b if pb <= pc else c
            cur[i] = (line[i] + p) & 255
        out[r * rowbytes:(r + 1) * rowbytes] = cur
        prev = bytes(cur)
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------------
def chunk(ctype, data=b"", crc=None):
    body = ctype + bytes(data)
    return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) if crc is None else crc)


def ihdr(width, height, colour, depth, interlace=0, compression=0, filt=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, compression, filt, interlace))


def fixed_stream(data):
    """A zlib stream of fixed-Huffman blocks (Z_FIXED)."""
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    return co.compress(bytes(data)) + co.flush()


def split(stream, plan):
    """The stream cut into IDAT payloads: plan is a list of lengths; the rest goes into a last chunk (None: one chunk)."""
    if plan is None:
        return [stream]
    parts, at = [], 0
    for n in plan:
        parts.append(stream[at:at + n])
        at += n
    parts.append(stream[at:])
    assert b"".join(parts) == stream
    return parts


def write(width, height, colour, depth, raw, filters, plan=None, stream=6, before=(), between=(), after=(), interlace=0, palette=True):
    """A PNG file.  raw: the height * rowbytes scanline bytes; filters: a type per row; plan: see split(); stream: a zlib level,
    or a callable that makes the zlib stream of the filtered bytes; before / after: whole chunks (bytes) in front of the first
    IDAT and behind the last; between: chunks put behind the first IDAT; palette: colour type 3 gets a PLTE."""
    bpp, rowbytes, size = shape(width, height, colour, depth)
    assert len(raw) == size and len(filters) == height
    filtered = filter_rows(raw, height, rowbytes, bpp, filters)
    zs = stream(filtered) if callable(stream) else zlib.compress(filtered, stream)
    out = [SIGNATURE, ihdr(width, height, colour, depth, interlace)]
    if colour == 3 and palette:
        out.append(chunk(b"PLTE", bytes((7 * k) & 255 for k in range(3 << depth))))
    out += list(before)
    for k, part in enumerate(split(bytes(zs), plan)):
        out.append(chunk(b"IDAT", part))
        if k == 0:
            out += list(between)
    out += list(after)
    out.append(chunk(b"IEND"))
    return b"".join(out)


def chunks_of(b):
    """[(position, type, data position, length)] of a sound file."""
    out, pos = [], 8
    while pos < len(b):
        n = struct.unpack(">I", b[pos:pos + 4])[0]
        out.append((pos, b[pos + 4:pos + 8], pos + 8, n))
        pos += 12 + n
    return out


def flip_crc(b, ctype, which=0):
    """The file with one bit of the CRC field of the which-th chunk of that type flipped."""
    pos, _, data, n = [c for c in chunks_of(b) if c[1] == ctype][which]
    at = data + n
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


# ---------------------------------------------------------------------------------------------------------------------
# the file rule of include/zes.h, restated
# ---------------------------------------------------------------------------------------------------------------------
def info_rule(b):
    """(status, info): the verdict of the file rule and, for ZES_OK, zes_png_info's fields as a dict."""
    b = bytes(b)
    c = len(b)
    if c < 8 or b[:8] != SIGNATURE:
        return ZES_E_PNG, None
    pos, k = 8, 0
    h = dict(idat_count=0, idat_bytes=0, plte_pos=0, plte_len=0, trns_pos=0, trns_len=0, pad2=0)
    idat = closed = plte = trns = False
    for _ in range(c // 12):
        if c - pos < 12:
            return ZES_E_PNG, None
        n, t = struct.unpack(">I", b[pos:pos + 4])[0], b[pos + 4:pos + 8]
        if n > 0x7fffffff or not all(65 <= x <= 90 or 97 <= x <= 122 for x in t) or n > c - pos - 12:
            return ZES_E_PNG, None
        d = pos + 8
        k += 1
        if k == 1:
            if t != b"IHDR" or n != 13:
                return ZES_E_PNG, None
            w, hh, depth, colour, comp, filt, inter = struct.unpack(">IIBBBBB", b[d:d + 13])
            if not (1 <= w <= 0x7fffffff and 1 <= hh <= 0x7fffffff) or colour not in DEPTHS or depth not in DEPTHS[colour] or comp or filt or inter > 1:
                return ZES_E_PNG, None
            h.update(width=w, height=hh, depth=depth, colour=colour, interlace=inter)
        elif t == b"IHDR":
            return ZES_E_PNG, None
        elif t == b"IDAT":
            if closed or (h["colour"] == 3 and not plte):
                return ZES_E_PNG, None
            idat = True
            h["idat_count"] += 1
            h["idat_bytes"] += n
        else:
            closed = idat
            if t == b"PLTE":
                if plte or idat or n % 3 or not 3 <= n <= 768:
                    return ZES_E_PNG, None
                plte = True
                h.update(plte_pos=d, plte_len=n)
            elif t == b"IEND":
                if n or pos + 12 != c or not idat:
                    return ZES_E_PNG, None
                bpp, rowbytes, size = shape(h["width"], h["height"], h["colour"], h["depth"])
                if h["height"] * (1 + rowbytes) > 0xFFFFFFFF:
                    return ZES_E_UNSUPPORTED, None
                h.update(channels=CHANNELS[h["colour"]], bpp=bpp, rowbytes=rowbytes, out_size=size)
                return 0, h
            elif 65 <= t[0] <= 90:
                return ZES_E_UNSUPPORTED, None
            elif t == b"tRNS" and not idat and not trns:
                trns = True
                h.update(trns_pos=d, trns_len=n)
        pos += 12 + n
    return ZES_E_PNG, None


def info_dict(rec):
    """A PNG_INFO record of the package as info_rule's dict."""
    return {f: int(rec[f]) for f in INFO_FIELDS}


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
def _cycle():
    """A cyclic sequence over the five filter types in which every ordered pair (a, b), a == b included, occurs once: an
    Euler circuit of the complete directed graph with loops (Hierholzer)."""
    left = {a: list(range(5)) for a in range(5)}
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop())
        else:
            out.append(stack.pop())
    seq = out[::-1][:-1]
    assert len(seq) == 25 and {(seq[i], seq[(i + 1) % 25]) for i in range(25)} == {(a, b) for a in range(5) for b in range(5)}
    return seq


CYCLE = _cycle()


def pattern(height, k):
    """Filter types for an image's rows: the cycle, started at its k-th place."""
    return [CYCLE[(r + k) % 25] for r in range(height)]


def pixels(size, seed):
    return np.random.RandomState(seed).randint(0, 256, size=size, dtype=np.uint8).tobytes()


class Case:
    def __init__(self, name, blob, want, status=0, info_status=None, short=False):
        self.name, self.blob, self.want = name, bytes(blob), want
        self.status = status            # what the decode calls answer (a tuple: any of these)
        self.info_status = status if info_status is None else info_status  # what the info call answers
        self.short = short              # the device form gets a capacity one byte short: ZES_E_NOSPACE


# (colour, depth, width, height): every pair, width and height, every bpp and every rowbytes residue mod 4
_GEOMETRY = [
    (0, 1, 1, 1), (0, 1, 17, 65), (0, 1, 300, 2), (0, 2, 3, 64), (0, 2, 65, 129), (0, 4, 5, 63), (0, 4, 63, 128), (0, 8, 1, 200), (0, 8, 2, 65),
    (0, 8, 64, 64), (0, 8, 300, 129), (0, 16, 1, 63), (0, 16, 17, 128), (0, 16, 65, 2),
    (2, 8, 1, 1), (2, 8, 2, 129), (2, 8, 3, 63), (2, 8, 5, 200), (2, 8, 17, 64), (2, 8, 63, 65), (2, 8, 64, 128), (2, 8, 65, 1), (2, 16, 1, 65),
    (2, 16, 3, 128), (2, 16, 64, 2), (2, 16, 17, 129),
    (3, 1, 63, 63), (3, 2, 17, 2), (3, 4, 65, 64), (3, 8, 5, 129), (3, 8, 300, 65),
    (4, 8, 1, 128), (4, 8, 63, 200), (4, 8, 64, 1), (4, 16, 2, 64), (4, 16, 5, 65),
    (6, 8, 1, 63), (6, 8, 3, 129), (6, 8, 65, 128), (6, 8, 300, 64), (6, 16, 1, 2), (6, 16, 17, 200), (6, 16, 63, 1),
]


@functools.lru_cache(maxsize=None)
def geometry():
    """The good table: about 40 images, each with seeded random pixels and the cycle's filter pattern."""
    out = []
    for k, (colour, depth, w, h) in enumerate(_GEOMETRY):
        raw = pixels(shape(w, h, colour, depth)[2], 1000 + k)
        out.append(Case("c%d d%d %dx%d" % (colour, depth, w, h), write(w, h, colour, depth, raw, pattern(h, k)), raw))
    return out


def geometry_facts():
    """What the table is there for (tests/test_png_cpu.py asserts it)."""
    g = _GEOMETRY
    sh = [shape(w, h, c, d) for c, d, w, h in g]
    firsts = {pattern(h, k)[0] for k, (_, _, _, h) in enumerate(g)}
    pairs = set()
    for k, (_, _, _, h) in enumerate(g):
        p = pattern(h, k)
        pairs |= set(zip(p, p[1:]))
    return dict(pairs={(c, d) for c, d, _, _ in g}, widths={w for _, _, w, _ in g}, heights={h for _, _, _, h in g}, bpp={s[0] for s in sh},
                residues={s[1] % 4 for s in sh}, row0=firsts, ordered=pairs, count=len(g))


BASE = (2, 8, 17, 70)  # the damage table's image: RGB, two bands


@functools.lru_cache(maxsize=None)
def damage():
    """Every kind of damage with the status the decode calls must give it (and the info call, where that differs)."""
    colour, depth, w, h = BASE
    bpp, rowbytes, size = shape(w, h, colour, depth)
    raw = pixels(size, 77)
    filt = pattern(h, 3)
    text = chunk(b"tEXt", b"Comment\0made by tests/_png.py")
    good = write(w, h, colour, depth, raw, filt, before=[text])
    filtered = filter_rows(raw, h, rowbytes, bpp, filt)
    row = filtered[:1 + rowbytes]

    def with_stream(zs, **kw):
        return write(w, h, colour, depth, raw, filt, stream=lambda _f: zs, **kw)

    zgood = zlib.compress(filtered, 6)
    bad5 = bytearray(filtered)
    bad5[66 * (1 + rowbytes)] = 5
    iend = chunks_of(good)[-1][0]
    pal_raw = pixels(shape(w, h, 3, 8)[2], 78)
    OK, CK, UN, PN = 0, ZES_E_CHECKSUM, ZES_E_UNSUPPORTED, ZES_E_PNG
    return [
        Case("bad signature", b"\x88" + good[1:], raw, PN),
        Case("no IEND", good[:iend], raw, PN),
        Case("bytes behind IEND", good + b"\0", raw, PN),
        Case("split IDAT run", write(w, h, colour, depth, raw, filt, plan=[20], between=[text]), raw, PN),
        Case("colour type 3 without PLTE", write(w, h, 3, 8, pal_raw, pattern(h, 1), palette=False), pal_raw, PN),
        Case("unknown critical chunk", write(w, h, colour, depth, raw, filt, before=[chunk(b"FRAc", b"abc")]), raw, UN),
        Case("interlaced", write(w, h, colour, depth, raw, filt, interlace=1), raw, UN, info_status=OK),
        Case("flipped CRC of IHDR", flip_crc(good, b"IHDR"), raw, CK, info_status=OK),
        Case("flipped CRC of an IDAT", flip_crc(write(w, h, colour, depth, raw, filt, plan=[50, 50]), b"IDAT", 1), raw, CK, info_status=OK),
        Case("flipped CRC of an ancillary chunk", flip_crc(good, b"tEXt"), raw, CK, info_status=OK),
        Case("flipped Adler-32", with_stream(zgood[:-1] + bytes([zgood[-1] ^ 1])), raw, CK, info_status=OK),
        Case("stream cut short", with_stream(zgood[:-12]), raw, INFLATE_STATUSES + (CK,), info_status=OK),
        Case("one row too many", with_stream(zlib.compress(filtered + row, 6)), raw, PN, info_status=OK),
        Case("one row too few", with_stream(zlib.compress(filtered[:-(1 + rowbytes)], 6)), raw, PN, info_status=OK),
        Case("filter byte 5", with_stream(zlib.compress(bytes(bad5), 6)), raw, PN, info_status=OK),
        Case("out_cap one byte short", good, raw, OK, short=True),
    ]


def neighbours():
    """Two good images to stand on either side of a damaged one."""
    g = geometry()
    return g[9], g[19]


def rule_only():
    """Further files that only the rule judges (no GPU needed to know their status): for the info call and walk parity."""
    colour, depth, w, h = 0, 8, 4, 3
    raw = pixels(12, 5)
    f = [0, 1, 2]
    good = write(w, h, colour, depth, raw, f)
    idat = [c for c in chunks_of(good) if c[1] == b"IDAT"][0]
    body = good[idat[0]:idat[2] + idat[3] + 4]
    head = lambda *a, **k: SIGNATURE + ihdr(*a, **k)
    tail = body + chunk(b"IEND")
    PN, UN = ZES_E_PNG, ZES_E_UNSUPPORTED
    trns = chunk(b"tRNS", b"\0\1")
    plte = chunk(b"PLTE", bytes(range(9)))
    return [
        Case("no bytes", b"", None, PN), Case("signature alone", SIGNATURE, None, PN), Case("seven bytes", SIGNATURE[:7], None, PN),
        Case("first chunk is not IHDR", SIGNATURE + tail, None, PN),
        Case("IHDR of 12 bytes", SIGNATURE + chunk(b"IHDR", b"\0" * 12) + tail, None, PN),
        Case("width 0", head(0, 3, 0, 8) + tail, None, PN), Case("height 2^31", head(4, 1 << 31, 0, 8) + tail, None, PN),
        Case("depth 3", head(4, 3, 0, 3) + tail, None, PN), Case("colour 2 depth 4", head(4, 3, 2, 4) + tail, None, PN),
        Case("colour 5", head(4, 3, 5, 8) + tail, None, PN), Case("compression 1", head(4, 3, 0, 8, compression=1) + tail, None, PN),
        Case("filter method 1", head(4, 3, 0, 8, filt=1) + tail, None, PN), Case("interlace 2", head(4, 3, 0, 8, interlace=2) + tail, None, PN),
        Case("second IHDR", head(4, 3, 0, 8) + ihdr(4, 3, 0, 8) + tail, None, PN),
        Case("no IDAT", head(4, 3, 0, 8) + chunk(b"IEND"), None, PN),
        Case("two PLTE", head(4, 3, 2, 8) + plte + plte + tail, None, PN),
        Case("PLTE behind IDAT", head(4, 3, 2, 8) + body + plte + chunk(b"IEND"), None, PN),
        Case("PLTE of 4 bytes", head(4, 3, 2, 8) + chunk(b"PLTE", b"abcd") + tail, None, PN),
        Case("PLTE of 771 bytes", head(4, 3, 2, 8) + chunk(b"PLTE", bytes(771)) + tail, None, PN),
        Case("IEND with data", head(4, 3, 0, 8) + body + chunk(b"IEND", b"x"), None, PN),
        Case("a type with a digit", head(4, 3, 0, 8) + chunk(b"tEX1", b"x") + tail, None, PN),
        Case("length beyond the file", head(4, 3, 0, 8) + struct.pack(">I", 1000) + b"IDATxx", None, PN),
        Case("length 2^31", head(4, 3, 0, 8) + struct.pack(">I", 1 << 31) + b"IDAT" + bytes(20), None, PN),
        Case("chunk cut inside its CRC", good[:-14], None, PN),
        Case("filtered size above 2^32 - 1", head(65536, 65536, 6, 16) + tail, None, UN),
        Case("critical chunk behind IDAT", head(4, 3, 0, 8) + body + chunk(b"ZZZz") + chunk(b"IEND"), None, UN),
        Case("tRNS noted, second one ignored", head(4, 3, 0, 8) + trns + chunk(b"tRNS", b"\0\2\3") + tail, raw, 0),
        Case("tRNS behind IDAT not noted", head(4, 3, 0, 8) + body + trns + chunk(b"IEND"), raw, 0),
        Case("PLTE in a truecolour file", head(4, 3, 2, 8) + plte + tail, None, 0),
        Case("many small chunks", write(w, h, colour, depth, raw, f, before=[chunk(b"tEXt", b"k\0v")] * 60), raw, 0),
    ]


def everything():
    """Both tables and the rule-only files: every file the info call and the walk are compared on."""
    return geometry() + damage() + rule_only()
