"""TIFF files built in memory for the TIFF reader's tests (tests/test_tiff_cpu.py, tests/test_gpu_tiff.py, tests/_tiff_poison.py):

  write()      a TIFF writer: II or MM byte order, strips or tiles, Compression 1, 8 or 32946, Predictor 1 or 2, 8, 16 or 32
               bits, 1 to 4 samples, several directories, segments at odd positions on request; the streams come from CPython's
               zlib or from a callable per segment (the CPU oracle's deflate, a damaged stream)
  rule()       the file rule of include/zes.h ("zes_tiff_*") stated once more, with the line that decided
  decode()     an independent reader on top of it (CPython's zlib, numpy): what every decode call must give
  cases()      the case table;  index_damage()  files with the status each must get and the rule's line it reaches;
  segment_damage()  one tile of twelve broken each way

Nothing here calls the library under test."""
import struct
import zlib

import numpy as np

OK, E_NOSPACE, E_DEVICE, E_ARG, E_CHECKSUM, E_UNSUPPORTED, E_TIFF = 0, -16, -17, -18, -21, -23, -25
FIELDS = ("width", "height", "seg_w", "seg_h", "across", "down", "bits", "spp", "compression", "predictor", "photometric", "sample_format",
          "extra_samples", "big_endian", "tiled", "out_size")
USED = (256, 257, 258, 259, 262, 266, 273, 277, 278, 279, 284, 317, 322, 323, 324, 325, 338, 339)

# the lines of the file rule, in the order in which they decide
LINES = ("header: short or magic", "header: BigTIFF", "header: version", "chain: offset", "chain: extent", "chain: hops", "chain: dir >= dirs",
         "entries: type", "entries: count", "entries: value offset", "geometry: width or length absent", "geometry: width or length 0",
         "geometry: both kinds or neither", "geometry: partner", "geometry: tile dimensions", "geometry: RowsPerStrip 0", "geometry: array count",
         "geometry: segment extent", "kinds: samples 0 or BitsPerSample count", "kinds: unequal depths", "kinds: depth", "kinds: samples > 4",
         "kinds: planes", "kinds: FillOrder", "kinds: Compression", "kinds: Predictor 3", "kinds: Predictor 2 uncompressed", "kinds: segment size",
         "kinds: segment count", "kinds: Predictor")
# a line no file below 4 GiB reaches: more than 2^31 - 1 segments need arrays of as many values inside the file
UNREACHABLE = ("kinds: segment count",)


# ---------------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------------
def _sample_dtype(bits, order, fmt=1):
    kind = "f" if (fmt == 3 and bits == 32) else "i" if fmt == 2 else "u"
    return np.dtype(("<" if order == "II" else ">") + kind + str(bits // 8))


def page(pixels, layout=("tiles", 16, 16), compression=8, predictor=1, sample_format=1, compress=None, seg_len=None, override=None, append=()):
    """One directory for write().  pixels: (h, w, spp) of uint8 / uint16 / uint32 (or the signed / float32 kinds with
    sample_format 2 / 3).  layout: ("tiles", tw, tl) or ("strips", rows).  compress(k, raw) -> the stream of segment k (default:
    zlib level 6).  seg_len(k, n) -> the byte count the directory states for segment k.  override: tag -> (type, values) or
    None (the tag left out).  append: (tag, type, values) entries behind the sorted ones."""
    return dict(pixels=np.ascontiguousarray(pixels), layout=layout, compression=compression, predictor=predictor, sample_format=sample_format,
                compress=compress, seg_len=seg_len, override=override or {}, append=tuple(append))


def segments_of(pg, order):
    """The decoded bytes of every segment of a page as the file holds them (byte order, predictor applied), row-major."""
    px = pg["pixels"]
    h, w, spp = px.shape
    bits = px.dtype.itemsize * 8
    u = px.view(np.dtype("u%d" % px.dtype.itemsize)) if px.dtype.kind != "u" else px
    if pg["layout"][0] == "tiles":
        _, tw, tl = pg["layout"]
    else:
        tw, tl = w, min(pg["layout"][1], h)
    out = []
    for y0 in range(0, h, tl):
        for x0 in range(0, w, tw):
            rows = tl if pg["layout"][0] == "tiles" else min(tl, h - y0)
            blk = np.zeros((rows, tw, spp), dtype=u.dtype)
            part = u[y0:y0 + rows, x0:x0 + tw]
            blk[:part.shape[0], :part.shape[1]] = part
            if pg["predictor"] == 2:
                blk[:, 1:] = blk[:, 1:] - blk[:, :-1]  # (modulo 2^bits: unsigned arithmetic)
            out.append(blk.astype(_sample_dtype(bits, order)).tobytes())
    return out


def write(pages, order="II", odd=False, first=None):
    """The file of `pages` (page() records), directories chained in order.  odd: every segment starts at an odd position.
    first: the header's first-directory offset instead of the real one."""
    e = "<" if order == "II" else ">"
    body = bytearray(b"II*\x00" if order == "II" else b"MM\x00*") + bytearray(4)
    links = [4]  # where the offset of the next directory goes
    for pg in pages:
        px = pg["pixels"]
        h, w, spp = px.shape
        bits = px.dtype.itemsize * 8
        offs, lens = [], []
        for k, raw in enumerate(segments_of(pg, order)):
            data = raw if pg["compression"] == 1 else (pg["compress"] or (lambda k, raw: zlib.compress(raw, 6)))(k, raw)
            if (len(body) & 1) != (1 if odd else 0):
                body += b"\x00"
            offs.append(len(body))
            lens.append(len(data) if pg["seg_len"] is None else pg["seg_len"](k, len(data)))
            body += data
        tags = {256: (4, [w]), 257: (4, [h]), 258: (3, [bits] * spp), 259: (3, [pg["compression"]]), 262: (3, [2 if spp >= 3 else 1]),
                277: (3, [spp]), 284: (3, [1]), 339: (3, [pg["sample_format"]] * spp)}
        if spp in (2, 4):
            tags[338] = (3, [2])
        if pg["predictor"] != 1:
            tags[317] = (3, [pg["predictor"]])
        if pg["layout"][0] == "tiles":
            tags.update({322: (3, [pg["layout"][1]]), 323: (3, [pg["layout"][2]]), 324: (4, offs), 325: (4, lens)})
        else:
            tags.update({278: (3, [pg["layout"][1]]), 273: (4, offs), 279: (4, lens)})
        for t, v in pg["override"].items():
            if v is None:
                tags.pop(t, None)
            else:
                tags[t] = v
        entries = [(t,) + tags[t] for t in sorted(tags)] + list(pg["append"])
        fixed = []
        for t, typ, vals in entries:
            fmt = {3: "H", 4: "I", 1: "B", 2: "B"}.get(typ, "I")
            if isinstance(vals, tuple) and vals and vals[0] == "at":  # ("at", count, offset): a value offset stated outright
                fixed.append((t, typ, vals[1], struct.pack(e + "I", vals[2])))
                continue
            blob = struct.pack(e + fmt * len(vals), *vals)
            if len(blob) <= 4:
                fixed.append((t, typ, len(vals), blob.ljust(4, b"\x00")))
            else:
                if len(body) & 1:
                    body += b"\x00"
                fixed.append((t, typ, len(vals), struct.pack(e + "I", len(body))))
                body += blob
        if len(body) & 1:
            body += b"\x00"
        at = len(body)
        struct.pack_into(e + "I", body, links[-1], at)
        body += struct.pack(e + "H", len(fixed))
        for t, typ, cnt, val in fixed:
            body += struct.pack(e + "HHI", t, typ, cnt) + val
        links.append(len(body))
        body += bytes(4)
    if first is not None:
        struct.pack_into(e + "I", body, 4, first)
    return bytes(body)


# ---------------------------------------------------------------------------------------------------------------------
# the rule, stated once more
# ---------------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, status, line, dirs=0):
        super().__init__("%d: %s" % (status, line))
        assert line in LINES, line
        self.status, self.line, self.dirs = status, line, dirs


def rule(data, dir=0):
    """(record, seg_off, seg_len, dirs) of directory `dir`, or Refused with the status and the deciding line."""
    data = bytes(data)
    c = len(data)
    if c < 8 or data[:2] not in (b"II", b"MM"):
        raise Refused(E_TIFF, "header: short or magic")
    e = "<" if data[:2] == b"II" else ">"
    u16 = lambda p: struct.unpack_from(e + "H", data, p)[0]
    u32 = lambda p: struct.unpack_from(e + "I", data, p)[0]
    if u16(2) == 43:
        raise Refused(E_UNSUPPORTED, "header: BigTIFF")
    if u16(2) != 42:
        raise Refused(E_TIFF, "header: version")
    chain, o = [], u32(4)
    while o:
        if len(chain) >= 65536:
            raise Refused(E_TIFF, "chain: hops")
        if o < 8 or o + 2 > c:
            raise Refused(E_TIFF, "chain: offset")
        n = u16(o)
        if o + 2 + 12 * n + 4 > c:
            raise Refused(E_TIFF, "chain: extent")
        chain.append((o, n))
        o = u32(o + 2 + 12 * n)
    dirs = len(chain)
    if dir >= dirs:
        raise Refused(E_ARG, "chain: dir >= dirs", dirs)
    try:
        return _directory(data, c, chain[dir], u16, u32) + (dirs,)
    except Refused as r:
        r.dirs = dirs
        raise


def _directory(data, c, where, u16, u32):
    at, n = where
    tags = {}
    for i in range(n):
        p = at + 2 + 12 * i
        t = u16(p)
        if t not in USED or t in tags:
            continue
        typ, cnt = u16(p + 2), u32(p + 4)
        if typ not in (3, 4):
            raise Refused(E_TIFF, "entries: type")
        if cnt == 0:
            raise Refused(E_TIFF, "entries: count")
        size = 2 if typ == 3 else 4
        pos = p + 8
        if cnt * size > 4:
            pos = u32(p + 8)
            if pos + cnt * size > c:
                raise Refused(E_TIFF, "entries: value offset")
        tags[t] = (typ, cnt, pos)

    def values(t, k=None):
        typ, cnt, pos = tags[t]
        k = cnt if k is None else k
        return [u16(pos + 2 * i) if typ == 3 else u32(pos + 4 * i) for i in range(k)]

    first = lambda t, absent: values(t, 1)[0] if t in tags else absent
    if 256 not in tags or 257 not in tags:
        raise Refused(E_TIFF, "geometry: width or length absent")
    W, H = first(256, 0), first(257, 0)
    if not W or not H:
        raise Refused(E_TIFF, "geometry: width or length 0")
    strips, tiles = any(t in tags for t in (273, 279)), any(t in tags for t in (322, 323, 324, 325))
    if strips == tiles:
        raise Refused(E_TIFF, "geometry: both kinds or neither")
    if not all(t in tags for t in ((273, 279) if strips else (322, 323, 324, 325))):
        raise Refused(E_TIFF, "geometry: partner")
    if tiles:
        sw, sh = first(322, 0), first(323, 0)
        if not sw or not sh or sw % 16 or sh % 16:
            raise Refused(E_TIFF, "geometry: tile dimensions")
    else:
        sw, sh = W, first(278, H)
        if not sh:
            raise Refused(E_TIFF, "geometry: RowsPerStrip 0")
        sh = min(sh, H)
    across, down = -(-W // sw), -(-H // sh)
    t_off, t_len = (324, 325) if tiles else (273, 279)
    if tags[t_off][1] != across * down or tags[t_len][1] != across * down:
        raise Refused(E_TIFF, "geometry: array count")
    off, ln = values(t_off), values(t_len)
    if any(o + l > c for o, l in zip(off, ln)):
        raise Refused(E_TIFF, "geometry: segment extent")
    spp, comp, pred, planar, fill = first(277, 1), first(259, 1), first(317, 1), first(284, 1), first(266, 1)
    if not spp or (tags[258][1] if 258 in tags else 1) != spp:
        raise Refused(E_TIFF, "kinds: samples 0 or BitsPerSample count")
    bits = values(258) if 258 in tags else [1]
    if any(b != bits[0] for b in bits):
        raise Refused(E_UNSUPPORTED, "kinds: unequal depths")
    if bits[0] not in (8, 16, 32):
        raise Refused(E_UNSUPPORTED, "kinds: depth")
    if spp > 4:
        raise Refused(E_UNSUPPORTED, "kinds: samples > 4")
    if planar != 1 and spp > 1:
        raise Refused(E_UNSUPPORTED, "kinds: planes")
    if fill != 1:
        raise Refused(E_UNSUPPORTED, "kinds: FillOrder")
    if comp not in (1, 8, 32946):
        raise Refused(E_UNSUPPORTED, "kinds: Compression")
    if pred == 3:
        raise Refused(E_UNSUPPORTED, "kinds: Predictor 3")
    if pred == 2 and comp == 1:
        raise Refused(E_UNSUPPORTED, "kinds: Predictor 2 uncompressed")
    if sw * sh * spp * (bits[0] // 8) > 0xFFFFFFFF:
        raise Refused(E_UNSUPPORTED, "kinds: segment size")
    if across * down > 0x7FFFFFFF:
        raise Refused(E_UNSUPPORTED, "kinds: segment count")
    if pred not in (1, 2):
        raise Refused(E_TIFF, "kinds: Predictor")
    rec = dict(width=W, height=H, seg_w=sw, seg_h=sh, across=across, down=down, bits=bits[0], spp=spp, compression=comp, predictor=pred,
               photometric=first(262, 0), sample_format=first(339, 1), extra_samples=first(338, 0), big_endian=int(u16(2) == 42 and data[:2] == b"MM"),
               tiled=int(tiles), out_size=W * H * spp * (bits[0] // 8))
    return rec, off, ln


# ---------------------------------------------------------------------------------------------------------------------
# an independent reader
# ---------------------------------------------------------------------------------------------------------------------
def out_dtype(rec):
    kind = "f" if (rec["sample_format"] == 3 and rec["bits"] == 32) else "i" if rec["sample_format"] == 2 else "u"
    return np.dtype("<" + kind + str(rec["bits"] // 8))


def touched(rec, rect):
    x, y, w, h = rect
    return [sy * rec["across"] + sx for sy in range(y // rec["seg_h"], (y + h - 1) // rec["seg_h"] + 1)
            for sx in range(x // rec["seg_w"], (x + w - 1) // rec["seg_w"] + 1)]


def decode(data, dir=0, rect=None, skip=()):
    """The pixels of the rectangle (x, y, w, h) as (h, w, spp), little-endian samples.  skip: segments left undecoded (zeros)."""
    data = bytes(data)
    rec, off, ln, _ = rule(data, dir)
    W, H, sw, sh, spp, bps = rec["width"], rec["height"], rec["seg_w"], rec["seg_h"], rec["spp"], rec["bits"] // 8
    img = np.zeros((H, W, spp), dtype="u%d" % bps)
    rect = rect or (0, 0, W, H)
    for k in touched(rec, rect):
        if k in skip:
            continue
        sy, sx = divmod(k, rec["across"])
        rows = sh if rec["tiled"] else min(sh, H - sy * sh)
        E = rows * sw * spp * bps
        raw = data[off[k]:off[k] + ln[k]]
        raw = raw[:E] if rec["compression"] == 1 else zlib.decompress(raw)
        assert len(raw) == E, (k, len(raw), E)
        blk = np.frombuffer(raw, dtype=(">" if rec["big_endian"] else "<") + "u%d" % bps).reshape(rows, sw, spp).astype("u%d" % bps)
        if rec["predictor"] == 2:
            blk = np.cumsum(blk, axis=1, dtype=blk.dtype)
        y0, x0 = sy * sh, sx * sw
        part = blk[:min(rows, H - y0), :min(sw, W - x0)]
        img[y0:y0 + part.shape[0], x0:x0 + part.shape[1]] = part
    x, y, w, h = rect
    return np.ascontiguousarray(img[y:y + h, x:x + w]).view(out_dtype(rec))


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = (("tiles", 16, 16), ("tiles", 32, 16), ("strips", 5), ("strips", 23))
CODINGS = ((1, 1), (8, 1), (8, 2), (32946, 1), (32946, 2))  # (Compression, Predictor) without the refused pair


def pixels(w, h, spp, bits, seed):
    rng = np.random.default_rng(seed)
    # smooth in places, so that the streams have matches, and full-range in others, so that the predictor's sums wrap
    a = rng.integers(0, 1 << bits, size=(h, w, spp), dtype=np.uint64)
    a[:, : w // 2] = (np.arange(w // 2)[None, :, None] * 3 + np.arange(h)[:, None, None]) & ((1 << bits) - 1)
    return a.astype("u%d" % (bits // 8))


def grid(layouts=LAYOUTS, depths=(8, 16, 32), samples=(1, 3, 4), orders=("II", "MM"), codings=CODINGS, w=37, h=23):
    """(name, keyword arguments of make()) for every combination."""
    for lay in layouts:
        for bits in depths:
            for spp in samples:
                for order in orders:
                    for comp, pred in codings:
                        name = "%s %s %d bits x %d %s c%d p%d" % (lay[0], "x".join(map(str, lay[1:])), bits, spp, order, comp, pred)
                        yield name, dict(w=w, h=h, spp=spp, bits=bits, layout=lay, order=order, compression=comp, predictor=pred)


def make(w, h, spp, bits, layout, order, compression, predictor, odd=True, compress=None, seed=None, seg_len=None):
    """(file, pixels) of one case; the pixels are a function of the shape and kind alone."""
    px = pixels(w, h, spp, bits, seed if seed is not None else w * 1000 + h * 10 + spp + bits)
    return write([page(px, layout, compression, predictor, compress=compress, seg_len=seg_len)], order, odd), px


def extra_cases():
    """The shapes beyond the grid: a row longer than a wave's lanes times one pixel, whose sums wrap modulo 2^16 (and one longer
    than a wave's runs, so that the sums cross the chunks of a row); a width of 1; exactly one tile; signed and float samples."""
    yield "300 x 3 strips of 16 bits x 3", dict(w=300, h=3, spp=3, bits=16, layout=("strips", 3), order="MM", compression=8, predictor=2)
    yield "700 x 2 strips of 8 bits x 4", dict(w=700, h=2, spp=4, bits=8, layout=("strips", 1), order="II", compression=8, predictor=2)
    yield "1100 x 2 strips of 8 bits x 3", dict(w=1100, h=2, spp=3, bits=8, layout=("strips", 2), order="II", compression=32946, predictor=2)
    yield "272 x 17 tiles of 272 x 16, 32 bits x 4", dict(w=272, h=17, spp=4, bits=32, layout=("tiles", 272, 16), order="MM", compression=8, predictor=2)
    yield "width 1", dict(w=1, h=9, spp=3, bits=8, layout=("strips", 4), order="II", compression=8, predictor=2)
    yield "width 1, tiled", dict(w=1, h=9, spp=1, bits=16, layout=("tiles", 16, 16), order="MM", compression=8, predictor=2)
    yield "one tile", dict(w=16, h=16, spp=4, bits=8, layout=("tiles", 16, 16), order="II", compression=8, predictor=2)
    yield "one tile, uncompressed", dict(w=16, h=16, spp=1, bits=8, layout=("tiles", 16, 16), order="II", compression=1, predictor=1)


def two_directories():
    """A file of two directories of different kinds, and the pixels of both."""
    a, b = pixels(37, 23, 3, 8, 5), pixels(20, 31, 1, 16, 6)
    return write([page(a, ("tiles", 16, 16), 8, 2), page(b, ("strips", 7), 32946, 2)], "MM", True), (a, b)


def rectangles(rec):
    """The rectangles of the tiled cases, by name."""
    W, H = rec["width"], rec["height"]
    return {"whole": (0, 0, W, H), "one pixel": (W - 2, H - 3, 1, 1), "inside one tile, off its column 0": (19, 3, 9, 7),
            "straddling four tiles": (27, 9, 8, 11), "last row": (0, H - 1, W, 1), "last column": (W - 1, 0, 1, H)}


# ---------------------------------------------------------------------------------------------------------------------
# damage
# ---------------------------------------------------------------------------------------------------------------------
def index_damage():
    """[(name, file, dir, status, line)]: files the rule refuses, one for every reachable line at least."""
    px = pixels(37, 23, 1, 8, 1)
    rgb = pixels(37, 23, 3, 8, 2)
    T, S = ("tiles", 16, 16), ("strips", 5)
    good = write([page(px, T)], "II")

    def patched(at, blob, base=good):
        b = bytearray(base)
        b[at:at + len(blob)] = blob
        return bytes(b)

    one = lambda **kw: write([page(kw.pop("px", px), kw.pop("layout", T), **kw)], "II")
    first_dir = struct.unpack_from("<I", good, 4)[0]
    n_first = struct.unpack_from("<H", good, first_dir)[0]
    loop = patched(first_dir + 2 + 12 * n_first, struct.pack("<I", first_dir))  # a directory that names itself as the next
    out = [
        ("seven bytes", good[:7], 0, E_TIFF, "header: short or magic"),
        ("no bytes", b"", 0, E_TIFF, "header: short or magic"),
        ("PNG magic", b"\x89PNG\r\n\x1a\n" + good[8:], 0, E_TIFF, "header: short or magic"),
        ("BigTIFF", patched(2, b"\x2b\x00"), 0, E_UNSUPPORTED, "header: BigTIFF"),
        ("version 41", patched(2, b"\x29\x00"), 0, E_TIFF, "header: version"),
        ("II with the MM version bytes", patched(2, b"\x00\x2a"), 0, E_TIFF, "header: version"),
        ("first directory at 4", patched(4, struct.pack("<I", 4)), 0, E_TIFF, "chain: offset"),
        ("first directory behind the file", patched(4, struct.pack("<I", len(good) - 1)), 0, E_TIFF, "chain: offset"),
        ("directory cut short", good[:-3], 0, E_TIFF, "chain: extent"),
        ("a chain that loops", loop, 0, E_TIFF, "chain: hops"),
        ("dir 1 of one", good, 1, E_ARG, "chain: dir >= dirs"),
        ("no directory at all", patched(4, bytes(4)), 0, E_ARG, "chain: dir >= dirs"),
        ("ImageWidth as RATIONAL", one(override={256: (5, ("at", 1, 8))}), 0, E_TIFF, "entries: type"),
        ("Compression as BYTE", one(override={259: (1, [8])}), 0, E_TIFF, "entries: type"),
        ("ImageLength with count 0", one(override={257: (4, ("at", 0, 0))}), 0, E_TIFF, "entries: count"),
        ("TileOffsets behind the file", one(override={324: (4, ("at", 6, 0x7FFFFFF0))}), 0, E_TIFF, "entries: value offset"),
        ("no ImageWidth", one(override={256: None}), 0, E_TIFF, "geometry: width or length absent"),
        ("ImageLength 0", one(override={257: (4, [0])}), 0, E_TIFF, "geometry: width or length 0"),
        ("strips and tiles", one(override={278: (3, [5])}, append=[(273, 4, [8]), (279, 4, [1])]), 0, E_TIFF, "geometry: both kinds or neither"),
        ("neither strips nor tiles", one(override={322: None, 323: None, 324: None, 325: None}), 0, E_TIFF, "geometry: both kinds or neither"),
        ("no TileByteCounts", one(override={325: None}), 0, E_TIFF, "geometry: partner"),
        ("no StripOffsets", one(layout=S, override={273: None}), 0, E_TIFF, "geometry: partner"),
        ("TileWidth 24", one(override={322: (3, [24])}), 0, E_TIFF, "geometry: tile dimensions"),
        ("TileLength 0", one(override={323: (3, [0])}), 0, E_TIFF, "geometry: tile dimensions"),
        ("RowsPerStrip 0", one(layout=S, override={278: (3, [0])}), 0, E_TIFF, "geometry: RowsPerStrip 0"),
        ("five TileOffsets for six tiles", one(override={324: (4, [8] * 5)}), 0, E_TIFF, "geometry: array count"),
        ("seven StripByteCounts for five strips", one(layout=S, override={279: (4, [1] * 7)}), 0, E_TIFF, "geometry: array count"),
        ("a tile that ends behind the file", one(seg_len=lambda k, n: n + (1 << 20) if k == 4 else n), 0, E_TIFF, "geometry: segment extent"),
        ("SamplesPerPixel 0", one(override={277: (3, [0])}), 0, E_TIFF, "kinds: samples 0 or BitsPerSample count"),
        ("one BitsPerSample for three samples", one(px=rgb, override={258: (3, [8])}), 0, E_TIFF, "kinds: samples 0 or BitsPerSample count"),
        ("no BitsPerSample, three samples", one(px=rgb, override={258: None}), 0, E_TIFF, "kinds: samples 0 or BitsPerSample count"),
        ("depths 8, 8, 16", one(px=rgb, override={258: (3, [8, 8, 16])}), 0, E_UNSUPPORTED, "kinds: unequal depths"),
        ("no BitsPerSample: bilevel", one(override={258: None}), 0, E_UNSUPPORTED, "kinds: depth"),
        ("4 bits", one(override={258: (3, [4])}), 0, E_UNSUPPORTED, "kinds: depth"),
        ("64 bits", one(override={258: (3, [64])}), 0, E_UNSUPPORTED, "kinds: depth"),
        ("five samples", one(override={277: (3, [5]), 258: (3, [8] * 5)}), 0, E_UNSUPPORTED, "kinds: samples > 4"),
        ("separate planes", one(px=rgb, override={284: (3, [2])}), 0, E_UNSUPPORTED, "kinds: planes"),
        ("FillOrder 2", one(append=[(266, 3, [2])]), 0, E_UNSUPPORTED, "kinds: FillOrder"),
        ("LZW", one(override={259: (3, [5])}), 0, E_UNSUPPORTED, "kinds: Compression"),
        ("PackBits", one(override={259: (3, [32773])}), 0, E_UNSUPPORTED, "kinds: Compression"),
        ("Predictor 3", one(override={317: (3, [3])}), 0, E_UNSUPPORTED, "kinds: Predictor 3"),
        ("Predictor 2 uncompressed", one(compression=1, override={317: (3, [2])}), 0, E_UNSUPPORTED, "kinds: Predictor 2 uncompressed"),
        ("a tile of 2^32 bytes", one(override={256: (4, [1]), 257: (4, [1]), 322: (4, [65536]), 323: (4, [65536]), 324: (4, [8]), 325: (4, [0])}), 0,
         E_UNSUPPORTED, "kinds: segment size"),
        ("a tile whose size does not fit 64 bits", one(override={256: (4, [1]), 257: (4, [1]), 322: (4, [0xFFFFFFF0]), 323: (4, [0xFFFFFFF0]), 324: (4, [8]),
                                                                  325: (4, [0]), 277: (3, [4]), 258: (3, [32] * 4)}), 0, E_UNSUPPORTED, "kinds: segment size"),
        ("Predictor 7", one(override={317: (3, [7])}), 0, E_TIFF, "kinds: Predictor"),
    ]
    return out


def index_quirks():
    """[(name, file, pixels)]: files the rule accepts although they look odd — unsorted entries, a tag twice (the first
    counts), SHORT arrays, inline arrays, absent tags whose defaults hold, RowsPerStrip beyond the height."""
    px = pixels(37, 23, 1, 8, 1)
    small = pixels(16, 16, 1, 8, 3)
    T, S = ("tiles", 16, 16), ("strips", 5)
    return [
        ("ImageWidth twice", write([page(px, T, append=[(256, 4, [9999])])], "II"), px),
        ("Predictor behind the sorted tags", write([page(px, T, 8, 2, override={317: None}, append=[(317, 3, [2])])], "MM"), px),
        ("no RowsPerStrip", write([page(px, ("strips", 23), override={278: None})], "II"), px),
        ("RowsPerStrip 0xFFFFFFFF", write([page(px, ("strips", 23), override={278: (4, [0xFFFFFFFF])})], "MM"), px),
        ("no Compression, Planar, SampleFormat, Photometric", write([page(px, S, 1, 1, override={259: None, 284: None, 339: None, 262: None})], "II"), px),
        ("one tile: inline arrays", write([page(small, T)], "II"), small),
        ("ImageWidth as SHORT", write([page(px, T, override={256: (3, [37]), 257: (3, [23])})], "MM"), px),
    ]


def stream_verdict(stream, E, oracle):
    """What step 4 of include/zes.h says about a stream that must give E bytes, from the CPU oracle and CPython's Adler-32."""
    try:
        out = oracle.inflate(np.frombuffer(bytes(stream), dtype=np.uint8))
    except oracle.OracleError as e:
        return e.code
    if out.size != E:
        return E_TIFF
    return OK if len(stream) >= 6 and zlib.adler32(out.tobytes()) == int.from_bytes(stream[-4:], "big") else E_CHECKSUM


def segment_damage(oracle):
    """[(name, file, pixels, the broken tile, its status)]: a 64 x 48 image of twelve 16 x 16 tiles with tile 7 broken."""
    px = pixels(64, 48, 3, 8, 9)
    T, bad, E = ("tiles", 16, 16), 7, 16 * 16 * 3
    raws = segments_of(page(px, T, 8, 2), "II")
    good = zlib.compress(raws[bad], 6)

    def flipped():
        b = bytearray(good)
        b[len(b) // 2] ^= 0x10
        return bytes(b)

    broken = {
        "cut short": good[: len(good) // 2],
        "a flipped stream bit": flipped(),
        "a wrong Adler-32": good[:-1] + bytes([good[-1] ^ 1]),
        "no Adler-32": good[:-4],
        "one row too long": zlib.compress(raws[bad] + bytes(16 * 3), 6),
        "one byte short": zlib.compress(raws[bad][:-1], 6),
        "an empty segment": b"",
    }
    out = []
    for name, s in broken.items():
        want = stream_verdict(s, E, oracle) if s else -1
        f = write([page(px, T, 8, 2, compress=lambda k, raw, s=s: s if k == bad else zlib.compress(raw, 6))], "II", True)
        out.append((name, f, px, bad, want))
    f = write([page(px, T, 1, 1, seg_len=lambda k, n: n - 1 if k == bad else n)], "MM", True)
    out.append(("an uncompressed segment too short", f, px, bad, E_TIFF))
    return out
