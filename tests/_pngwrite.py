"""The PNG writer's expected bytes, built independently of the library: the filter rule of include/zes.h ("zes_pngwrite*") in
numpy on top of _png.filter_rows, the CPU oracle's zlib stream of the filtered bytes (or the stored form, restated here), and
_png.chunk for the chunks; the images the CPU and the GPU tests share; and the callers of both forms."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np

import _png

PIECES = 4  # ZES_F_PIECES
IDAT, BLOCK, BLK = 65536, 65535, 131072
GROUP, GROUP_SLOTS, GROUP_PIECES, GROUP_SLOTS_PIECES = 1024, 256 << 20, 4, 1 << 20


class Img:
    def __init__(self, name, width, height, colour, depth, filt, raw, plte=b"", trns=b""):
        self.name, self.width, self.height, self.colour, self.depth, self.filter = name, width, height, colour, depth, filt
        self.raw, self.plte, self.trns = bytes(raw), bytes(plte), bytes(trns)
        self.bpp, self.rowbytes, size = _png.shape(width, height, colour, depth)
        assert len(self.raw) == size, (name, len(self.raw), size)

    @property
    def F(self):
        return self.height * (1 + self.rowbytes)

    def record(self):
        return (self.width, self.height, self.depth, self.colour, self.filter, 0, len(self.plte), len(self.trns))

    def rows(self):
        return np.frombuffer(self.raw, dtype=np.uint8).reshape(self.height, self.rowbytes)


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def costs(im):
    """[5][height]: the sum of min(x, 256 - x) over row r's bytes filtered by type t."""
    out = []
    for t in range(5):
        f = np.frombuffer(_png.filter_rows(im.raw, im.height, im.rowbytes, im.bpp, [t] * im.height), dtype=np.uint8).reshape(im.height, 1 + im.rowbytes)
        x = f[:, 1:].astype(np.int64)
        out.append(np.minimum(x, 256 - x).sum(axis=1))
    return np.array(out)


def choose(im):
    """The filter type of every row."""
    if im.filter <= 4:
        return [im.filter] * im.height
    if im.colour == 3 or im.depth < 8:
        return [0] * im.height
    c = costs(im)
    return [int(np.argmin(c[:2, r] if im.filter == 5 and r % 64 == 0 else c[:, r])) for r in range(im.height)]  # (argmin: the first of equals)


def filtered(im):
    return _png.filter_rows(im.raw, im.height, im.rowbytes, im.bpp, choose(im))


def stored(f):
    out = [b"\x78\x01"]
    for at in range(0, len(f), BLOCK):
        part = f[at:at + BLOCK]
        out.append(struct.pack("<BHH", 1 if at + BLOCK >= len(f) else 0, len(part), len(part) ^ 0xFFFF) + part)
    out.append(struct.pack(">I", zlib.adler32(f)))
    return b"".join(out)


def stored_len(F):
    return 2 + 5 * ((F + BLOCK - 1) // BLOCK) + F + 4


def stream(f, oracle):
    """(the zlib stream of the filtered bytes f, "stream" | "stored" | "refused")."""
    if len(f) % BLK == 1:
        return stored(f), "refused"
    zs = oracle.deflate(np.frombuffer(f, dtype=np.uint8)).tobytes()
    return (zs, "stream") if len(zs) < stored_len(len(f)) else (stored(f), "stored")


def file_of(im, zs):
    out = [_png.SIGNATURE, _png.ihdr(im.width, im.height, im.colour, im.depth)]
    if im.plte:
        out.append(_png.chunk(b"PLTE", im.plte))
    if im.trns:
        out.append(_png.chunk(b"tRNS", im.trns))
    out += [_png.chunk(b"IDAT", zs[at:at + IDAT]) for at in range(0, len(zs), IDAT)]
    out.append(_png.chunk(b"IEND"))
    return b"".join(out)


_EXPECT = {}


def expect(im, oracle):
    """(file, route) for an image, made once."""
    key = (im.name, im.filter)
    if key not in _EXPECT:
        zs, route = stream(filtered(im), oracle)
        _EXPECT[key] = (file_of(im, zs), route)
    return _EXPECT[key]


def bound(im):
    zl = stored_len(im.F)
    return 8 + 25 + (12 + len(im.plte) if im.plte else 0) + (12 + len(im.trns) if im.trns else 0) + zl + 12 * ((zl + IDAT - 1) // IDAT) + 12


def idats(blob):
    return [n for _, t, _, n in _png.chunks_of(blob) if t == b"IDAT"]


def groups(ims, flags=0):
    """How many images each group of a call takes (include/zes.h): the count's limit, and the encoder slots' bytes."""
    most, room = (GROUP_PIECES, GROUP_SLOTS_PIECES) if flags & PIECES else (GROUP, GROUP_SLOTS)
    slot = lambda F: 0 if F % BLK == 1 else ((max(BLK, 2 * F) if F >= BLK // 2 else BLK) + 6 + 15) // 16 * 16
    out, cnt, used = [], 0, 0
    for im in ims:
        if cnt and (cnt == most or used + slot(im.F) > room):
            out.append(cnt)
            cnt, used = 0, 0
        cnt, used = cnt + 1, used + slot(im.F)
    return out + ([cnt] if cnt else [])


# ---------------------------------------------------------------------------------------------------------------------
# the images
# ---------------------------------------------------------------------------------------------------------------------
def palette(depth):
    return bytes((7 * k) & 255 for k in range(3 << depth))


@functools.lru_cache(maxsize=None)
def geometry():
    """Every (colour, depth) pair, every width and height of the issue's lists (heights 128 and 200 of the reader's table
    become 129 and 65), filter values 0..6 in turn; palette images with their PLTE, some images with a tRNS."""
    out = []
    for k, (colour, depth, w, h) in enumerate(_png._GEOMETRY):
        h = {128: 129, 200: 65}.get(h, h)
        raw = _png.pixels(_png.shape(w, h, colour, depth)[2], 2000 + k)
        plte = palette(depth) if colour == 3 else b""
        trns = {0: b"\0\1", 2: b"\0\1\0\2\0\3", 3: b"\x80"}.get(colour, b"") if k % 3 == 0 else b""
        out.append(Img("geo %d: c%d d%d %dx%d f%d" % (k, colour, depth, w, h, k % 7), w, h, colour, depth, k % 7, raw, plte, trns))
    return out


def geometry_facts():
    g = geometry()
    return dict(pairs={(i.colour, i.depth) for i in g}, widths={i.width for i in g}, heights={i.height for i in g}, filters={i.filter for i in g},
                bpp={i.bpp for i in g})


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


@functools.lru_cache(maxsize=None)
def each_wins_raw():
    """33 x 130 RGB 8: rows built so that each of the five types is some row's cheapest; row 64 is built for Paeth and row 128
    for Up, where filter value 5 must take None or Sub."""
    w, h, bpp = 33, 130, 3
    rb = w * bpp
    rs = np.random.RandomState(99)
    rows = []
    for r in range(h):
        kind = (r + 5) % 6
        prev = rows[-1] if rows else [0] * rb
        if kind == 0:
            row = [int(x) for x in rs.randint(0, 256, rb)]
        elif kind == 1:  # Up: the row above once more
            row = list(prev)
        elif kind == 2:  # Average
            row = []
            for i in range(rb):
                row.append(((row[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)
        elif kind == 3:  # Paeth: a first pixel off the one above (else the row is the row above again, and Up ties), then the predictor
            row = [(prev[i] + 50) & 255 for i in range(bpp)]
            for i in range(bpp, rb):
                row.append(_paeth(row[i - bpp], prev[i], prev[i - bpp]))
        elif kind == 4:  # Sub: one colour
            row = [100, 150, 200] * w
        else:            # None: +1 and -1 in turn
            row = [1 if i % 2 == 0 else 255 for i in range(rb)]
        rows.append(row)
    return bytes(x for row in rows for x in row)


def each_wins(filt):
    return Img("each filter wins f%d" % filt, 33, 130, 2, 8, filt, each_wins_raw())


def zeros(filt=6):
    return Img("all zeros f%d" % filt, 40, 70, 2, 8, filt, bytes(40 * 3 * 70))


def rgba16(filt=6):
    return Img("rgba 16 f%d" % filt, 21, 67, 6, 16, filt, smooth(21 * 8, 67, 32))


def smooth(rowbytes, height, seed):
    """Rows that drift: neighbours differ by little, so the predicting filters pay."""
    rs = np.random.RandomState(seed)
    a = np.cumsum(rs.randint(-2, 3, size=(height, rowbytes)), axis=1) + np.cumsum(rs.randint(-3, 4, size=(height, 1)), axis=0)
    return (a & 255).astype(np.uint8).tobytes()


def grey4(filt=5):
    return Img("grey 4 f%d" % filt, 37, 66, 0, 4, filt, _png.pixels(_png.shape(37, 66, 0, 4)[2], 33))


def random_rgba():
    return Img("random rgba", 96, 192, 6, 8, 5, _png.pixels(96 * 4 * 192, 34))


def lowent_rgba():
    return Img("low entropy rgba", 256, 256, 6, 8, 5, bytes(np.random.RandomState(35).randint(0, 16, 256 * 4 * 256, dtype=np.uint8)))


def refused():
    """F = 131073 twice: 2 x 43691 and 43690 x 3 grey 8."""
    return [Img("refused 2x43691", 2, 43691, 0, 8, 0, _png.pixels(2 * 43691, 36)), Img("refused 43690x3", 43690, 3, 0, 8, 1, smooth(43690, 3, 37))]


def nine():
    """Nine small images: one group, or groups of 4, 4 and 1 under ZES_F_PIECES."""
    return [Img("nine %d" % k, 20 + k, 10 + k, 2, 8, 5, smooth((20 + k) * 3, 10 + k, 50 + k)) for k in range(9)]


def bad_records():
    """One image of each step-1 kind and one of step 2, as (Img-like record, in_len, status)."""
    ARG, UNS = _png.ZES_E_ARG, _png.ZES_E_UNSUPPORTED
    rec = lambda w=4, h=3, d=8, c=0, f=0, pad=0, pl=0, tr=0: (w, h, d, c, f, pad, pl, tr)
    return [
        (rec(c=2, d=4), 12, ARG), (rec(c=5), 12, ARG), (rec(w=0), 0, ARG), (rec(h=1 << 31), 4 << 31, ARG), (rec(f=7), 12, ARG), (rec(pad=1), 12, ARG),
        (rec(), 13, ARG), (rec(c=3, pl=4), 12, ARG), (rec(c=3, pl=0), 12, ARG), (rec(c=3, d=2, pl=15), 3, ARG), (rec(c=0, pl=3), 12, ARG),
        (rec(c=4, pl=3), 24, ARG), (rec(c=0, tr=1), 12, ARG), (rec(c=2, tr=2), 36, ARG), (rec(c=3, pl=6, tr=3), 12, ARG), (rec(c=4, tr=2), 24, ARG),
        (rec(c=6, tr=2), 48, ARG), (rec(w=65536, h=65536, c=6, d=16), 65536 * 65536 * 8, UNS),
    ]


# ---------------------------------------------------------------------------------------------------------------------
# the callers
# ---------------------------------------------------------------------------------------------------------------------
def records(z, ims):
    rec = np.zeros(max(len(ims), 1), dtype=z.PNGW_IMAGE)
    for i, im in enumerate(ims):
        rec[i] = im.record() if isinstance(im, Img) else im
    return rec


def aux_of(ims):
    return b"".join(im.plte + im.trns for im in ims)


def run_dev(z, gpu, ims, flags=0, in_shift=None, out_off=None, cap=None, null_out=False):
    """zes_pngwrite_dev into a tensor filled with 0xA5 -> (host copy of the tensor, off, out_len, status).  Image i's scanlines
    start at a byte whose residue mod 16 is in_shift[i] (default: i + 1); its file at out_off[i] (default: 16-byte steps with
    the bound's room and a gap of 5 + i bytes)."""
    import torch

    n = len(ims)
    in_shift = [(i + 1) % 16 for i in range(n)] if in_shift is None else in_shift
    in_off, at = [], 0
    for i, im in enumerate(ims):
        at = (at + 15) // 16 * 16 + in_shift[i]
        in_off.append(at)
        at += len(im.raw)
    flat = np.full(at + 16, 0x5A, dtype=np.uint8)
    for o, im in zip(in_off, ims):
        flat[o:o + len(im.raw)] = np.frombuffer(im.raw, dtype=np.uint8)
    bounds = [bound(im) for im in ims]
    if out_off is None:
        out_off, at = [], 3
        for i, b in enumerate(bounds):
            out_off.append(at)
            at += b + 5 + i
    cap = bounds if cap is None else cap
    total = max([int(o) + int(c) for o, c in zip(out_off, cap)] + [0]) + 32
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
    if null_out:
        res = z.png_encode_tensor(torch.from_numpy(flat).to(gpu), in_off, [len(im.raw) for im in ims], records(z, ims)[:n], aux_of(ims), out=None, off=out_off,
                                  cap=cap, flags=flags)
        return None, out_off, res[2], res[3]
    _, off, out_len, status = z.png_encode_tensor(torch.from_numpy(flat).to(gpu), in_off, [len(im.raw) for im in ims], records(z, ims)[:n], aux_of(ims), out=out,
                                                  off=out_off, cap=cap, flags=flags)
    return out.cpu().numpy(), [int(o) for o in off], out_len, status


def check_dev(host, off, out_len, status, want):
    """Every file byte for byte (want[i]: the bytes, or None for an image that writes nothing), and every other byte 0xA5."""
    mask = np.zeros(host.size, dtype=bool)
    for i, w in enumerate(want):
        if w is None:
            continue
        assert status[i] == 0 and out_len[i] == len(w), (i, status[i], out_len[i], len(w))
        got = host[off[i]:off[i] + len(w)].tobytes()
        if got != w:
            first = next(k for k in range(len(w)) if got[k] != w[k])
            raise AssertionError("image %d differs at byte %d of %d" % (i, first, len(w)))
        mask[off[i]:off[i] + len(w)] = True
    assert (host[~mask] == 0xA5).all(), "a byte outside the files was written"


def run_host(z, ims, flags=0):
    """zes_pngwrite through the package -> a list of bytes or error codes."""
    res = z.png_encode_batch([dict(rows=im.rows(), width=im.width, colour=im.colour, depth=im.depth, filter=im.filter, palette=im.plte, trns=im.trns)
                              for im in ims], flags)
    return [r.code if isinstance(r, Exception) else r.tobytes() for r in res]


def raw_call(z, recs, lens, form="dev", d_in=0x1000, d_out=0x2000, aux=b"", flags=0, count=None, null=()):
    """The C entry points with arguments as they are (pointers are never followed when no image passes the checks) ->
    (rc, out_len, status)."""
    n = len(recs) if count is None else count
    rec = records(z, recs)
    ln = np.array(list(lens) + [0], dtype=np.uint64)
    zero = np.zeros(n + 1, dtype=np.uint64)
    cap = np.full(n + 1, 1 << 40, dtype=np.uint64)
    out_len = np.full(n + 1, 77, dtype=np.uint64)
    status = np.full(n + 1, 77, dtype=np.int32)
    a = np.frombuffer(bytes(aux) + b"\0", dtype=np.uint8)
    p = lambda name, arr: None if name in null else arr.ctypes.data
    if form == "dev":
        rc = z.lib().zes_pngwrite_dev(None if "d_in" in null else d_in, p("in_off", zero), p("in_len", ln), p("img", rec), p("aux", a), n,
                                      None if "d_out" in null else d_out, p("out_off", zero), p("out_cap", cap), p("out_len", out_len), p("status", status), flags)
    else:
        keep = [np.zeros(16, dtype=np.uint8) for _ in range(n + 1)]
        ptrs = (C.c_void_p * (n + 1))(*[None if ("in%d" % i) in null else k.ctypes.data for i, k in enumerate(keep)])
        alloc = z.ALLOC_FN(lambda _u, _i, _n: None)
        rc = z.lib().zes_pngwrite(None if "in" in null else ptrs, p("in_len", ln), p("img", rec), p("aux", a), n,
                                  C.cast(None, z.ALLOC_FN) if "alloc" in null else alloc, None, p("out_len", out_len), p("status", status), flags)
    return rc, [int(x) for x in out_len[:n]], [int(x) for x in status[:n]]
