"""The TIFF writer's expected bytes, built independently of the library: the file layout of include/zes.h ("zes_tiffwrite*")
stated once more here — header, segments at even offsets, out-of-line arrays in their order, the directory — around segment
bytes from _tiff.segments_of and streams from the CPU oracle's deflate, or the stored form restated; the case table the CPU and
the GPU tests share; the records the calls must refuse; and the callers of both forms.

expect(case, oracle) -> (file, routes): the route of a segment is "stream", "stored" (the stream was not shorter), "refused" (a
length the encoder does not take) or, under Compression 1, where there is nothing to choose, "none"."""
import ctypes as C
import struct
import zlib

import numpy as np

import _tiff as T

PIECES = 4  # ZES_F_PIECES
BLOCK, BLK = 65535, 131072
GROUP, GROUP_PIECES = 1024, 4
CODINGS = ((1, 1), (8, 1), (8, 2), (32946, 2))
SENTINEL = 0xA5


class Case:
    def __init__(self, name, px, layout, order="II", compression=8, predictor=2, sample_format=1):
        self.name, self.px, self.layout, self.order = name, np.ascontiguousarray(px), layout, order
        self.compression, self.predictor, self.sample_format = compression, predictor, sample_format

    def record(self):
        h, w, spp = self.px.shape
        bits = self.px.dtype.itemsize * 8
        tiled = self.layout[0] == "tiles"
        sw, sh = (self.layout[1], self.layout[2]) if tiled else (w, min(self.layout[1], h))
        return dict(width=w, height=h, seg_w=sw, seg_h=sh, across=-(-w // sw), down=-(-h // sh), bits=bits, spp=spp, compression=self.compression,
                    predictor=self.predictor, photometric=2 if spp >= 3 else 1, sample_format=self.sample_format, extra_samples=2 if spp in (2, 4) else 0,
                    big_endian=int(self.order == "MM"), tiled=int(tiled), out_size=w * h * spp * bits // 8)

    def segments(self):
        return T.segments_of(T.page(self.px, self.layout, self.compression, self.predictor), self.order)

    def raw(self):
        """The input of the write calls: the pixels as tiff_read gives them."""
        return np.ascontiguousarray(self.px).view(np.uint8).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# the file, stated once more
# ---------------------------------------------------------------------------------------------------------------------
def stored(f):
    out = [b"\x78\x01"]
    for at in range(0, len(f), BLOCK):
        part = f[at:at + BLOCK]
        out.append(struct.pack("<BHH", 1 if at + BLOCK >= len(f) else 0, len(part), len(part) ^ 0xFFFF) + part)
    out.append(struct.pack(">I", zlib.adler32(f)))
    return b"".join(out)


def stored_len(E, compression=8):
    return E if compression == 1 else 2 + 5 * ((E + BLOCK - 1) // BLOCK) + E + 4


def refuses(n):
    return n == 1 or n % BLK == 1


def stream(f, compression, oracle):
    """(a segment's bytes in the file, its route)."""
    if compression == 1:
        return f, "none"
    if refuses(len(f)):
        return stored(f), "refused"
    zs = oracle.deflate(np.frombuffer(f, dtype=np.uint8)).tobytes()
    return (zs, "stream") if len(zs) < stored_len(len(f)) else (stored(f), "stored")


def entries_of(rec, offs, lens):
    """tag -> (type, values) of the one directory."""
    spp, base, tiled = rec["spp"], 3 if rec["photometric"] == 2 else 1, rec["tiled"]
    tags = {256: (4, [rec["width"]]), 257: (4, [rec["height"]]), 258: (3, [rec["bits"]] * spp), 259: (3, [rec["compression"]]),
            262: (3, [rec["photometric"]]), 277: (3, [spp]), 284: (3, [1])}
    if tiled:
        tags.update({322: (4, [rec["seg_w"]]), 323: (4, [rec["seg_h"]]), 324: (4, list(offs)), 325: (4, list(lens))})
    else:
        tags.update({273: (4, list(offs)), 278: (4, [rec["seg_h"]]), 279: (4, list(lens))})
    if rec["predictor"] == 2:
        tags[317] = (3, [2])
    if spp > base:
        tags[338] = (3, [rec["extra_samples"]] * (spp - base))
    if rec["sample_format"] != 1:
        tags[339] = (3, [rec["sample_format"]] * spp)
    return tags


def file_of(rec, datas):
    """(file, offsets, lengths): the layout around the segments' bytes as they go into the file."""
    e = ">" if rec["big_endian"] else "<"
    body = bytearray(b"MM\x00*" if rec["big_endian"] else b"II*\x00") + bytearray(4)
    offs, lens = [], []
    for d in datas:
        assert len(body) % 2 == 0
        offs.append(len(body))
        lens.append(len(d))
        body += d
        if len(body) & 1:
            body += b"\x00"
    tags = entries_of(rec, offs, lens)
    blob = lambda t: struct.pack(e + {3: "H", 4: "I"}[tags[t][0]] * len(tags[t][1]), *tags[t][1])
    placed = {}
    for t in (258, 338, 339, 324 if rec["tiled"] else 273, 325 if rec["tiled"] else 279):
        if t in tags and len(blob(t)) > 4:
            assert len(body) % 2 == 0
            placed[t] = len(body)
            body += blob(t)
    assert len(body) % 2 == 0
    struct.pack_into(e + "I", body, 4, len(body))
    body += struct.pack(e + "H", len(tags))
    for t in sorted(tags):
        body += struct.pack(e + "HHI", t, tags[t][0], len(tags[t][1]))
        body += struct.pack(e + "I", placed[t]) if t in placed else blob(t).ljust(4, b"\x00")
    body += bytes(4)
    return bytes(body), offs, lens


_EXPECT = {}


def expect(case, oracle):
    """(file, routes) of a case, made once."""
    if case.name not in _EXPECT:
        got = [stream(f, case.compression, oracle) for f in case.segments()]
        _EXPECT[case.name] = (file_of(case.record(), [d for d, _ in got])[0], [r for _, r in got])
    return _EXPECT[case.name]


def seg_sizes(rec):
    """The decoded size of every segment, from the record alone."""
    ps = rec["spp"] * rec["bits"] // 8
    out = []
    for sy in range(rec["down"]):
        rows = rec["seg_h"] if rec["tiled"] else min(rec["seg_h"], rec["height"] - sy * rec["seg_h"])
        out += [rec["seg_w"] * rows * ps] * rec["across"]
    return out


def bound(rec):
    """The file with every segment in the stored form: the layout above around bytes of those lengths."""
    return len(file_of(rec, [bytes(stored_len(E, rec["compression"])) for E in seg_sizes(rec)])[0])


def groups(rec, flags=0):
    """How many segments each group of a call takes when the count alone limits it (small segments)."""
    most = GROUP_PIECES if flags & PIECES else GROUP
    n = rec["across"] * rec["down"]
    return [min(most, n - k) for k in range(0, n, most)]


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def grid(layouts=T.LAYOUTS, depths=(8, 16, 32), samples=(1, 3, 4), orders=("II", "MM"), codings=CODINGS, w=37, h=23):
    for lay in layouts:
        for bits in depths:
            for spp in samples:
                for order in orders:
                    for comp, pred in codings:
                        name = "%s %s %d bits x %d %s c%d p%d" % (lay[0], "x".join(map(str, lay[1:])), bits, spp, order, comp, pred)
                        yield Case(name, T.pixels(w, h, spp, bits, w * 1000 + h * 10 + spp + bits), lay, order, comp, pred)


def shapes():
    """Where the cut kernel can go wrong: width 1; exactly one tile; strip rows longer than a wave's runs for both run sizes, so
    that the pixel in front of a run crosses the chunks of a row; two samples; a tile wider than the image by most of itself."""
    mk = lambda name, w, h, spp, bits, lay, order="II", comp=8, pred=2: Case(name, T.pixels(w, h, spp, bits, w * 1000 + h * 10 + spp + bits), lay, order, comp, pred)
    return [
        mk("width 1", 1, 9, 3, 8, ("strips", 4)),
        mk("width 1, tiled", 1, 9, 1, 16, ("tiles", 16, 16), "MM"),
        mk("one tile", 16, 16, 4, 8, ("tiles", 16, 16)),
        mk("one tile, uncompressed", 16, 16, 1, 8, ("tiles", 16, 16), "II", 1, 1),
        mk("1100 x 2 strips of 8 bits x 3", 1100, 2, 3, 8, ("strips", 2), "II", 32946),
        mk("1100 x 3 strips of 8 bits x 1", 1100, 3, 1, 8, ("strips", 2)),
        mk("1100 x 2 strips of 16 bits x 3", 1100, 2, 3, 16, ("strips", 1), "MM"),
        mk("300 x 3 strips of 32 bits x 4", 300, 3, 4, 32, ("strips", 3), "MM"),
        mk("two samples", 37, 23, 2, 16, ("tiles", 32, 16), "MM"),
        mk("272 x 17 tiles of 272 x 16, 32 bits x 4", 272, 17, 4, 32, ("tiles", 272, 16), "MM"),
        mk("zero rows below", 40, 35, 3, 8, ("tiles", 16, 32)),
        mk("a tile of 1040 pixels of 8 bits x 3", 1030, 3, 3, 8, ("tiles", 1040, 16)),
    ]


def kinds():
    """Signed 16-bit and float32 samples."""
    s = (np.arange(37 * 23 * 2, dtype=np.int64).reshape(23, 37, 2) * 37 - 30000).astype(np.int16)
    fl = np.linspace(-3, 3, 23 * 37, dtype=np.float32).reshape(23, 37, 1)
    i8 = (np.arange(16 * 16 * 3).reshape(16, 16, 3) % 251 - 120).astype(np.int8)
    return [Case("signed 16 bits x 2", s, ("tiles", 16, 16), "MM", 8, 2, 2), Case("float32", fl, ("strips", 5), "II", 32946, 1, 3),
            Case("float32, Predictor 2, MM", fl, ("tiles", 16, 16), "MM", 8, 2, 3), Case("signed 8 bits x 3, uncompressed", i8, ("tiles", 16, 16), "II", 1, 1, 2)]


def refused():
    """Lengths the encoder does not take: 1, and 1 mod 131072."""
    one = np.array([[[77]]], dtype=np.uint8)
    long = (np.arange(131073, dtype=np.uint32) * 7 % 251).astype(np.uint8).reshape(1, 131073, 1)
    return [Case("refused: 1 x 1", one, ("strips", 1), "II", 8, 1), Case("refused: 131073 x 1", long, ("strips", 1), "MM", 8, 2)]


def six_tiles():
    return Case("six tiles", T.pixels(37, 23, 3, 8, 71), ("tiles", 16, 16), "II", 8, 2)


def many_strips():
    return Case("1025 strips", T.pixels(16, 1025, 1, 8, 72), ("strips", 1), "MM", 8, 2)


MIXED_SEED = 5


def mixed(seed=MIXED_SEED):
    """64 x 48 RGB of twelve 16 x 16 tiles: noise in the tiles whose index is even, one colour in the others."""
    rng = np.random.default_rng(seed)
    px = np.zeros((48, 64, 3), dtype=np.uint8)
    for k in range(12):
        sy, sx = divmod(k, 4)
        px[sy * 16:(sy + 1) * 16, sx * 16:(sx + 1) * 16] = rng.integers(0, 256, size=(16, 16, 3), dtype=np.uint8) if k % 2 == 0 else 10 + k
    return Case("mixed routes, seed %d" % seed, px, ("tiles", 16, 16), "II", 8, 2)


def rgba_tiles(side):
    """The launch-list images: side x side RGBA of 16 x 16 tiles."""
    return Case("rgba %d" % side, np.random.default_rng(side).integers(0, 256, size=(side, side, 4), dtype=np.uint8), ("tiles", 16, 16), "II", 8, 2)


def gpu_cases():
    """Every case the GPU tests write, the grid aside."""
    return shapes() + kinds() + refused() + [six_tiles(), many_strips(), mixed(), rgba_tiles(32)]


def bad_records():
    """[(name, record, n or None for out_size, status)]: one record for every line of statuses 1 and 2 that a record or n reaches."""
    ARG, UNS = T.E_ARG, T.E_UNSUPPORTED
    good = Case("good", T.pixels(37, 23, 3, 8, 1), ("tiles", 16, 16)).record()
    strips = Case("good strips", T.pixels(37, 23, 1, 8, 1), ("strips", 5)).record()

    def alt(base=good, **kw):
        r = dict(base)
        r.update(kw)
        return r

    def sized(**kw):
        """a consistent record of these fields: across, down and out_size follow"""
        r = alt(**kw)
        r["across"], r["down"] = -(-r["width"] // r["seg_w"]), -(-r["height"] // r["seg_h"])
        r["out_size"] = (r["width"] * r["height"] * r["spp"] * r["bits"] // 8) & 0xFFFFFFFFFFFFFFFF
        return r

    return [
        ("width 0", alt(width=0), None, ARG), ("across off by one", alt(across=4), None, ARG), ("down off by one", alt(down=3), None, ARG),
        ("out_size off by one", alt(out_size=good["out_size"] + 1), None, ARG), ("n one short", good, good["out_size"] - 1, ARG),
        ("n one long", good, good["out_size"] + 1, ARG), ("big_endian 2", alt(big_endian=2), None, ARG), ("tiled 2", alt(tiled=2), None, ARG),
        ("12 bits", sized(bits=12), None, ARG), ("64 bits", sized(bits=64), None, ARG), ("no samples", sized(spp=0), None, ARG),
        ("five samples", sized(spp=5), None, ARG), ("tile width 24", sized(seg_w=24), None, ARG), ("tile length 0", alt(seg_h=0), None, ARG),
        ("a strip narrower than the image", alt(strips, seg_w=36, across=2), None, ARG), ("RowsPerStrip above the height", alt(strips, seg_h=24), None, ARG),
        ("LZW", alt(compression=5), None, ARG), ("Predictor 3", alt(predictor=3), None, ARG), ("Predictor 0", alt(predictor=0), None, ARG),
        ("palette", alt(photometric=3), None, ARG), ("RGB of one sample", sized(base=strips, photometric=2), None, ARG),
        ("extra_samples 3", sized(spp=4, extra_samples=3), None, ARG), ("extra samples without a sample for them", alt(extra_samples=1), None, ARG),
        ("sample_format 0", alt(sample_format=0), None, ARG), ("sample_format 4", alt(sample_format=4), None, ARG),
        ("float at 8 bits", alt(sample_format=3), None, ARG), ("float at 16 bits", sized(bits=16, sample_format=3), None, ARG),
        # the first that applies: ZES_E_ARG although the record is unsupported too
        ("Predictor 2 uncompressed and a wrong out_size", alt(compression=1, out_size=7), None, ARG),
        ("Predictor 2 uncompressed", alt(compression=1), None, UNS),
        ("a tile of 2^32 bytes", sized(width=1, height=1, seg_w=65536, seg_h=65536, spp=1, photometric=1), None, UNS),
        ("2^31 segments", sized(base=strips, width=1, height=1 << 31, seg_w=1, seg_h=1, compression=1, predictor=1), None, UNS),
        ("a bound above 0xFFFFFFFF", sized(width=32768, height=32768, seg_w=256, seg_h=256, spp=4), None, UNS),
        ("a bound above 0xFFFFFFFF by the arrays", sized(base=strips, width=1, height=500000000, seg_w=1, seg_h=1, compression=1, predictor=1), None, UNS),
    ]


# ---------------------------------------------------------------------------------------------------------------------
# the callers
# ---------------------------------------------------------------------------------------------------------------------
def record_array(z, rec):
    img = np.zeros(1, dtype=z.TIFF_IMAGE)
    for k in T.FIELDS:
        img[0][k] = rec[k]
    return img


def bound_call(z, rec):
    """zes_tiffwrite_bound as it is: (status, cap, segments)."""
    img = record_array(z, rec)
    cap, nseg = C.c_uint64(77), C.c_uint64(77)
    rc = z.lib().zes_tiffwrite_bound(img.ctypes.data, C.byref(cap), C.byref(nseg))
    return rc, cap.value, nseg.value


def raw_call(z, rec, n=None, form="dev", flags=0, null=(), d_in=0x1000, d_out=0x2000, cap=1 << 40):
    """The C entry points with arguments as they are (pointers are never followed when the checks refuse the call) ->
    (status, out_len)."""
    img = record_array(z, rec)
    n = rec["out_size"] if n is None else n
    out_len = C.c_uint64(77)
    p_img = None if "img" in null else img.ctypes.data
    p_len = None if "out_len" in null else C.byref(out_len)
    if form == "dev":
        rc = z.lib().zes_tiffwrite_dev(None if "in" in null else d_in, n, p_img, None if "d_out" in null else d_out, cap, p_len, None, None, flags)
    else:
        keep = np.zeros(16, dtype=np.uint8)
        alloc = C.cast(None, z.ALLOC_FN) if "alloc" in null else z.ALLOC_FN(lambda _u, _i, _n: None)
        rc = z.lib().zes_tiffwrite(None if "in" in null else keep.ctypes.data, n, p_img, alloc, None, p_len, flags)
    return rc, out_len.value


def on_device(a, gpu, lead=1):
    import torch

    return torch.from_numpy(np.concatenate([np.zeros(lead, dtype=np.uint8), np.asarray(a, dtype=np.uint8)])).to(gpu)[lead:]


def run_dev(z, gpu, case, at=0, flags=0, lead=1, cap=None):
    """zes_tiffwrite_dev into a tensor of sentinel bytes, the file at offset `at` of it and the input `lead` bytes behind an
    allocation's start -> (file bytes, seg_off, seg_len); every byte outside the file's range is checked against the sentinel."""
    import torch

    rec = case.record()
    room_for = bound(rec) if cap is None else cap
    room = torch.full((at + room_for + 41,), SENTINEL, dtype=torch.uint8, device=gpu)
    f, off, ln = z.tiff_write_tensor(on_device(case.raw(), gpu, lead), rec, out=room[at:at + room_for], flags=flags)
    n = int(f.numel())
    host = room.cpu().numpy()
    assert (host[:at] == SENTINEL).all() and (host[at + n:] == SENTINEL).all(), "a byte outside the file's range was written"
    return host[at:at + n].tobytes(), [int(v) for v in off], [int(v) for v in ln]


def run_host(z, case, flags=0):
    return z.tiff_write(case.px, case.record(), flags)


def first_difference(got, want):
    if got == want:
        return None
    if len(got) != len(want):
        return "length %d, expected %d" % (len(got), len(want))
    return "byte %d of %d" % (next(k for k in range(len(want)) if got[k] != want[k]), len(want))
