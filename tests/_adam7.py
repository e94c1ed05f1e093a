"""Adam7-interlaced PNG files for the reader's tests, in pure Python and numpy, on top of tests/_png.py: the seven passes
cut out of raw scanlines at bit level, each filtered as an image of its own by _png.filter_rows with a filter type per (pass,
row), the stream and the chunks made as _png.write makes them; the pass geometry and the interlaced filtered size Fi of
include/zes.h restated; an independent per-pixel deinterlace (the oracle of the writer); and the case lists that the CPU and
the GPU tests share."""
import functools
import zlib

import numpy as np

import _png

ZES_F_PIECES, ZES_F_PNG_INTERLACED = 4, 128
# (x0, y0, dx, dy) of pass 1..7 (PNG specification, 8.2)
PASSES = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def pass_dims(width, height):
    """[(pw, ph)] of the seven passes; (0, 0) for a pass without pixels."""
    out = []
    for x0, y0, dx, dy in PASSES:
        pw = -(-(width - x0) // dx) if width > x0 else 0
        ph = -(-(height - y0) // dy) if height > y0 else 0
        out.append((pw, ph) if pw and ph else (0, 0))
    return out


def pass_rowbytes(pw, colour, depth):
    return (pw * _png.CHANNELS[colour] * depth + 7) // 8


def fi(width, height, colour, depth):
    """The interlaced filtered size of include/zes.h: a filter byte and the row bytes for every row of every pass with pixels."""
    return sum(ph * (1 + pass_rowbytes(pw, colour, depth)) for pw, ph in pass_dims(width, height))


def clean(raw, width, height, colour, depth):
    """raw with the pad bits behind the last pixel of every row (depths below 8) set to zero."""
    bits = _png.CHANNELS[colour] * depth
    _, rowbytes, _ = _png.shape(width, height, colour, depth)
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(height, rowbytes).copy()
    used = (width * bits - 1) % 8 + 1
    rows[:, -1] &= (0xFF << (8 - used)) & 0xFF
    return rows.tobytes()


def pixels(width, height, colour, depth, seed):
    """Seeded random scanlines with zero pad bits: what a reader must give back."""
    return clean(_png.pixels(_png.shape(width, height, colour, depth)[2], seed), width, height, colour, depth)


def split_passes(raw, width, height, colour, depth, pad_ones=False):
    """The seven passes' packed rows as bytes (b"" for a pass without pixels); pad_ones: the pad bits of a pass row are ones."""
    bits = _png.CHANNELS[colour] * depth
    _, rowbytes, _ = _png.shape(width, height, colour, depth)
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(height, rowbytes)
    px = np.unpackbits(rows, axis=1)[:, :width * bits].reshape(height, width, bits)
    out = []
    for (x0, y0, dx, dy), (pw, ph) in zip(PASSES, pass_dims(width, height)):
        if not pw:
            out.append(b"")
            continue
        sub = px[y0::dy, x0::dx, :].reshape(ph, pw * bits)
        prb = pass_rowbytes(pw, colour, depth)
        full = np.full((ph, prb * 8), 1 if pad_ones else 0, dtype=np.uint8)
        full[:, :pw * bits] = sub
        out.append(np.packbits(full, axis=1).tobytes())
    return out


def pattern(width, height, k):
    """A filter type per (pass, row): _png.pattern per pass, pass p started at the cycle's place k + p."""
    return [_png.pattern(ph, k + p) for p, (_, ph) in enumerate(pass_dims(width, height))]


def constant(width, height, ft):
    return [[ft] * ph for _, ph in pass_dims(width, height)]


def filtered(raw, width, height, colour, depth, filters, pad_ones=False):
    """The bytes the zlib stream of an interlaced file holds: the passes back to back, filters[p][r] the type of row r of pass p + 1."""
    bpp = _png.shape(width, height, colour, depth)[0]
    out = []
    for p, ((pw, ph), rows) in enumerate(zip(pass_dims(width, height), split_passes(raw, width, height, colour, depth, pad_ones))):
        if pw:
            assert len(filters[p]) == ph
            out.append(_png.filter_rows(rows, ph, pass_rowbytes(pw, colour, depth), bpp, filters[p]))
    return b"".join(out)


def wrap(width, height, colour, depth, body, plan=None, stream=6, before=(), between=(), after=(), interlace=1, palette=True):
    """The file around the filtered bytes `body`: _png.write's chunks with interlace method 1 in the header."""
    zs = stream(body) if callable(stream) else zlib.compress(body, stream)
    out = [_png.SIGNATURE, _png.ihdr(width, height, colour, depth, interlace)]
    if colour == 3 and palette:
        out.append(_png.chunk(b"PLTE", bytes((7 * k) & 255 for k in range(3 << depth))))
    out += list(before)
    for k, part in enumerate(_png.split(bytes(zs), plan)):
        out.append(_png.chunk(b"IDAT", part))
        if k == 0:
            out += list(between)
    out += list(after)
    out.append(_png.chunk(b"IEND"))
    return b"".join(out)


def write(width, height, colour, depth, raw, filters, pad_ones=False, **kw):
    """An interlaced PNG file of the scanlines `raw`; plan, stream and the chunk options as in _png.write."""
    assert len(raw) == _png.shape(width, height, colour, depth)[2]
    return wrap(width, height, colour, depth, filtered(raw, width, height, colour, depth, filters, pad_ones), **kw)


def minsum(raw, width, height, colour, depth):
    """The usual encoder's choice: for every pass row the type with the smallest sum of absolute filtered values."""
    bpp = _png.shape(width, height, colour, depth)[0]
    out = []
    for (pw, ph), rows in zip(pass_dims(width, height), split_passes(raw, width, height, colour, depth)):
        if not pw:
            out.append([])
            continue
        prb = pass_rowbytes(pw, colour, depth)
        x = np.frombuffer(rows, dtype=np.uint8).reshape(ph, prb).astype(np.int32)
        a = np.zeros_like(x)
        a[:, bpp:] = x[:, :-bpp] if prb > bpp else 0
        b = np.zeros_like(x)
        b[1:] = x[:-1]
        c = np.zeros_like(x)
        c[:, bpp:] = b[:, :-bpp] if prb > bpp else 0
        preds = [np.zeros_like(x), a, b, (a + b) >> 1, _png._paeth_np(a, b, c)]
        cost = [np.abs(((x - p) & 255).astype(np.uint8).view(np.int8).astype(np.int32)).sum(axis=1) for p in preds]
        out.append([int(t) for t in np.argmin(np.stack(cost), axis=0)])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the oracle of the writer: unfilter every pass with _png.unfilter, then put every pixel in its place, one by one
# ---------------------------------------------------------------------------------------------------------------------
def deinterlace(body, width, height, colour, depth):
    """The scanlines that the interlaced filtered bytes `body` stand for (None: a filter byte above 4, or a wrong length)."""
    bits = _png.CHANNELS[colour] * depth
    bpp, rowbytes, size = _png.shape(width, height, colour, depth)
    if len(body) != fi(width, height, colour, depth):
        return None
    out = bytearray(size)
    at = 0
    for (x0, y0, dx, dy), (pw, ph) in zip(PASSES, pass_dims(width, height)):
        if not pw:
            continue
        prb = pass_rowbytes(pw, colour, depth)
        rows = _png.unfilter(body[at:at + ph * (1 + prb)], ph, prb, bpp)
        at += ph * (1 + prb)
        if rows is None:
            return None
        for m in range(ph):
            for k in range(pw):
                x, y = x0 + k * dx, y0 + m * dy
                for b in range(bits):
                    sbit, dbit = k * bits + b, x * bits + b
                    if rows[m * prb + sbit // 8] >> (7 - sbit % 8) & 1:
                        out[y * rowbytes + dbit // 8] |= 0x80 >> dbit % 8
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------------------------------
def case(name, colour, depth, w, h, filters, seed, pad_ones=False, **kw):
    raw = pixels(w, h, colour, depth, seed)
    return _png.Case(name, write(w, h, colour, depth, raw, filters, pad_ones=pad_ones, **kw), raw)


def plain_of(c):
    """The same pixels as the interlaced case c in a non-interlaced file by _png.write."""
    rec = _png.info_rule(c.blob)[1]
    w, h, colour, depth = rec["width"], rec["height"], rec["colour"], rec["depth"]
    return _png.Case("plain " + c.name, _png.write(w, h, colour, depth, c.want, _png.pattern(h, 2)), c.want)


@functools.lru_cache(maxsize=None)
def small_grid():
    """Every width and height in 1..9 — every combination of passes without pixels — for RGBA8 and 1-bit grey."""
    out = []
    for colour, depth in ((6, 8), (0, 1)):
        for w in range(1, 10):
            for h in range(1, 10):
                out.append(case("c%d d%d %dx%d" % (colour, depth, w, h), colour, depth, w, h, pattern(w, h, w + 3 * h), 9 * w + h, pad_ones=depth < 8))
    return out


@functools.lru_cache(maxsize=None)
def pairs():
    """Every (colour, depth) pair at 13 x 11 and 37 x 19, the cycle's filters per pass, the pass rows' pad bits ones."""
    out = []
    for k, (colour, depth) in enumerate(_png.PAIRS):
        for w, h in ((13, 11), (37, 19)):
            out.append(case("c%d d%d %dx%d" % (colour, depth, w, h), colour, depth, w, h, pattern(w, h, k + w), 500 + 2 * k + w, pad_ones=depth < 8))
    return out


@functools.lru_cache(maxsize=None)
def seams():
    """5 x 131 has 65 rows in pass 7, 3 x 513 has 65 rows in pass 1: a second band of k_png_unfilter inside a pass.  Chains of
    one filter type 2, 3, 4 across that seam, and a restart row (None, Sub) on and beside pass row 64."""
    out = []
    for w, h, p in ((5, 131, 6), (3, 513, 0)):
        for colour, depth in ((2, 8), (0, 2)):
            for ft in (2, 3, 4):
                out.append(case("%dx%d c%d type %d" % (w, h, colour, ft), colour, depth, w, h, constant(w, h, ft), 700 + len(out), pad_ones=depth < 8))
            for row in (63, 64):
                for ft in (0, 1):
                    f = constant(w, h, 4)
                    f[p][row] = ft
                    out.append(case("%dx%d c%d restart %d at %d" % (w, h, colour, ft, row), colour, depth, w, h, f, 720 + len(out), pad_ones=depth < 8))
    return out


@functools.lru_cache(maxsize=None)
def tiled():
    """Images of more than one tile of k_png_deinterlace (about 32 KiB of output rows a tile): 1100 x 70 RGBA16 has rows of
    8800 bytes, 3 a tile, more 16-byte units a row than a workgroup has threads; 300 x 200 RGB has 36 rows a tile and a short
    last tile; 1000 x 601 at 1 bit has 262 rows a tile."""
    return [case("c6 d16 1100x70", 6, 16, 1100, 70, pattern(1100, 70, 2), 800),
            case("c2 d8 300x200", 2, 8, 300, 200, pattern(300, 200, 5), 801),
            case("c0 d1 1000x601", 0, 1, 1000, 601, pattern(1000, 601, 9), 802, pad_ones=True)]


def damaged():
    """[(case, status)]: interlaced files that must fail, each for one reason."""
    colour, depth, w, h = 2, 8, 13, 11
    raw = pixels(w, h, colour, depth, 900)
    f = pattern(w, h, 4)
    body = filtered(raw, w, h, colour, depth, f)
    dims = pass_dims(w, h)
    at3 = sum(ph * (1 + pass_rowbytes(pw, colour, depth)) for pw, ph in dims[:2])  # the first filter byte of pass 3
    bad5 = bytearray(body)
    assert bad5[at3] <= 4
    bad5[at3] = 5
    bpp, rowbytes, _ = _png.shape(w, h, colour, depth)
    plain = _png.filter_rows(raw, h, rowbytes, bpp, _png.pattern(h, 1))
    assert len(plain) != len(body)
    mk = lambda name, b: _png.Case(name, wrap(w, h, colour, depth, bytes(b)), raw, _png.ZES_E_PNG)
    good = wrap(w, h, colour, depth, body, plan=[30, 30])
    return [
        mk("filter byte 5 in pass 3", bad5),
        mk("stream one byte short of Fi", body[:-1]),
        mk("the plain F bytes under an interlace-1 header", plain),
        _png.Case("flipped CRC of an IDAT", _png.flip_crc(good, b"IDAT", 1), raw, _png.ZES_E_CHECKSUM),
    ]
