"""The PNG pixel forms' tests, in numpy: the conversion rule of include/zes.h restated (rule(): the definition the tests
compare against) and the case table (cases()) that the CPU and the GPU tests walk, built on the writer of tests/_png.py.

The table has every (colour, depth) pair at every width of WIDTHS, the heights of HEIGHTS taken in turn so that every pair
and every width meets each of them, without a tRNS and — for colour types 0, 2 and 3 — with one whose key equals a stored
sample; and the special cases: keys that match in the high byte only (depth 16), keys that a scaling reader confuses (depths
2 and 4), palettes shorter than 1 << depth with indices beyond them in the data, a tRNS shorter than the palette, and a tRNS
of a length that does not fit the colour type, which is ignored."""
import functools

import numpy as np

import _png

WIDTHS = (1, 3, 4, 5, 7, 8, 9, 17, 63, 64, 65)
HEIGHTS = (1, 2, 65)  # 65 crosses an unfilter band
SCALE = {1: 255, 2: 85, 4: 17}
# what Pillow's convert("RGBA") agrees with: (colour, depth, with a tRNS).  The other 7 combinations are the rule's alone
PIL_AGREES = {(0, 1, False), (0, 1, True), (0, 2, False), (0, 4, False), (0, 8, False), (0, 8, True), (2, 8, False), (2, 8, True), (2, 16, False),
              (3, 1, False), (3, 1, True), (3, 2, False), (3, 2, True), (3, 4, False), (3, 4, True), (3, 8, False), (3, 8, True),
              (4, 8, False), (4, 16, False), (6, 8, False), (6, 16, False)}
PIL_DIFFERS = {(0, 2, True), (0, 4, True), (0, 16, False), (0, 16, True), (2, 16, True)}  # it compares the key after its own conversion, or clips
assert len(PIL_AGREES) == 21 and len(PIL_DIFFERS) == 5 and not PIL_AGREES & PIL_DIFFERS  # the 15 pairs, and the 11 of colours 0, 2, 3 with a tRNS


def samples(raw, width, height, colour, depth):
    """The stored samples at their full depth: a uint32 array of height x width x channels."""
    ch = _png.CHANNELS[colour]
    _, rowbytes, _ = _png.shape(width, height, colour, depth)
    rows = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(height, rowbytes)
    if depth < 8:  # one sample a pixel, the first one of a byte in its high bits; the bits behind the row's last pixel are padding
        bits = np.unpackbits(rows, axis=1)[:, :width * depth].reshape(height, width, depth).astype(np.uint32)
        s = (bits << np.arange(depth - 1, -1, -1, dtype=np.uint32)).sum(axis=2).reshape(height, width, 1)
    elif depth == 8:
        s = rows[:, :width * ch].reshape(height, width, ch)
    else:
        b = rows[:, :2 * width * ch].reshape(height, width, ch, 2).astype(np.uint32)
        s = b[..., 0] << 8 | b[..., 1]
    return s.astype(np.uint32)


def to8(s, depth):
    return (s * SCALE[depth] if depth < 8 else s if depth == 8 else s >> 8).astype(np.uint8)


def fitting(colour, plte, trns):
    """The tRNS bytes that count: a length that does not fit the colour type is no tRNS."""
    n = len(trns)
    ok = n == 2 if colour == 0 else n == 6 if colour == 2 else colour == 3 and n <= len(plte) // 3
    return bytes(trns) if ok else b""


def rule(raw, width, height, colour, depth, plte=b"", trns=b""):
    """The conversion rule: height x width x 4 bytes of R, G, B, A."""
    s = samples(raw, width, height, colour, depth)
    t = fitting(colour, plte, trns)
    out = np.empty((height, width, 4), dtype=np.uint8)
    out[..., 3] = 255
    if colour == 3:
        table = np.zeros((256, 4), dtype=np.uint8)
        table[:, 3] = 255
        n = min(len(plte) // 3, 256)
        table[:n, :3] = np.frombuffer(bytes(plte), dtype=np.uint8)[:3 * n].reshape(n, 3)
        table[:len(t), 3] = np.frombuffer(t, dtype=np.uint8)
        return table[s[..., 0]]
    if colour in (0, 4):
        out[..., :3] = to8(s[..., :1], depth)
    else:
        out[..., :3] = to8(s[..., :3], depth)
    if colour in (4, 6):
        out[..., 3] = to8(s[..., -1], depth)
    elif t:
        key = np.frombuffer(t, dtype=">u2").astype(np.uint32)  # one key a sample, all 16 bits of it
        out[..., 3] = np.where((s == key).all(axis=2), 0, 255)
    return out


class Case:
    def __init__(self, name, kind, colour, depth, width, height, raw, plte, trns, k):
        self.name, self.kind = name, kind
        self.colour, self.depth, self.width, self.height = colour, depth, width, height
        self.raw, self.plte, self.trns = bytes(raw), bytes(plte), bytes(trns)
        self.k = k  # where the filter cycle starts

    @property
    def fits(self):
        """The writer's records can say it (zes_pngpix_expand_dev takes it): every tRNS but one of an unfitting length."""
        return fitting(self.colour, self.plte, self.trns) == self.trns

    @functools.cached_property
    def want(self):
        return rule(self.raw, self.width, self.height, self.colour, self.depth, self.plte, self.trns)

    def file(self, stream=6):
        """The PNG file; stream: a zlib level, or a callable that makes the zlib stream of the filtered bytes."""
        before = ([_png.chunk(b"PLTE", self.plte)] if self.plte else []) + ([_png.chunk(b"tRNS", self.trns)] if self.trns else [])
        return _png.write(self.width, self.height, self.colour, self.depth, self.raw, _png.pattern(self.height, self.k), before=before, palette=False,
                          stream=stream)

    @functools.cached_property
    def blob(self):
        return self.file()

    def record(self):
        """The fields of a PNGW_IMAGE record."""
        return (self.width, self.height, self.depth, self.colour, 0, 0, len(self.plte), len(self.trns))


def be16(*keys):
    return b"".join(int(k).to_bytes(2, "big") for k in keys)


def _key(s, colour, at):
    """A tRNS whose key is the stored pixel at row-major place `at`."""
    px = s.reshape(-1, s.shape[2])[at % (s.shape[0] * s.shape[1])]
    return be16(*px[:3 if colour == 2 else 1])


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    rs = np.random.RandomState(4242)

    def add(kind, colour, depth, w, h, plte=b"", trns=None, raw=None):
        k = len(out)
        raw = _png.pixels(_png.shape(w, h, colour, depth)[2], 5000 + k) if raw is None else raw
        if callable(trns):
            trns = trns(samples(raw, w, h, colour, depth))
        c = Case("%s c%d d%d %dx%d" % (kind, colour, depth, w, h), kind, colour, depth, w, h, raw, plte, trns or b"", k)
        out.append(c)
        return c

    full = lambda depth: rs.randint(0, 256, size=3 << depth, dtype=np.uint8).tobytes()
    for pi, (colour, depth) in enumerate(_png.PAIRS):
        for wi, w in enumerate(WIDTHS):
            h = HEIGHTS[(wi + pi) % 3]
            plte = full(depth) if colour == 3 else b""
            add("plain", colour, depth, w, h, plte)
            if colour == 3:  # an alpha for every entry
                add("trns", colour, depth, w, h, plte, rs.randint(0, 256, size=1 << depth, dtype=np.uint8).tobytes())
            elif colour in (0, 2):  # the key is a stored pixel
                add("trns", colour, depth, w, h, plte, lambda s, colour=colour, wi=wi: _key(s, colour, 3 * wi + 1))
    # depth 16: the key equals a stored pixel in the high bytes only, which must not match
    for colour in (0, 2):
        for w, h in ((5, 2), (17, 65)):
            def high_only(s, colour=colour):
                px = s.reshape(-1, s.shape[2])[2 % (s.shape[0] * s.shape[1])][:3 if colour == 2 else 1].copy()
                px[-1] ^= 0x5A  # the low byte of the last sample
                assert not (s == px).all(axis=2).any()
                return be16(*px)
            add("trns high byte only", colour, 16, w, h, b"", high_only)
    # depths 2 and 4: keys that a reader who compares after scaling confuses: a non-zero stored sample (its scaled value is
    # another number), and the scaled value of a stored sample (above the depth's range: it matches nothing)
    for depth in (2, 4):
        for w, h in ((7, 2), (65, 65)):
            for kind, key in (("trns small key", 1), ("trns scaled key", SCALE[depth])):
                raw = b"\x1b" + _png.pixels(_png.shape(w, h, 0, depth)[2], 6000 + len(out))[1:]  # the samples 0, 1, 2, 3 or 1, 11: a 1 among them
                add(kind, 0, depth, w, h, b"", be16(key), raw)
    # palettes shorter than 1 << depth (random data then has indices beyond them), and a tRNS shorter than the palette
    for depth, entries in ((1, 1), (2, 3), (4, 9), (8, 200)):
        for w, h in ((9, 2), (64, 65)):
            plte = rs.randint(0, 256, size=3 * entries, dtype=np.uint8).tobytes()
            for kind, trns in (("short palette", b""), ("short palette short trns", rs.randint(0, 256, size=(entries + 1) // 2, dtype=np.uint8).tobytes())):
                raw = b"\xff" + _png.pixels(_png.shape(w, h, 3, depth)[2], 7000 + len(out))[1:]  # the first index is the depth's largest
                c = add(kind, 3, depth, w, h, plte, trns, raw)
                assert (samples(c.raw, w, h, 3, depth) >= entries).any() and (samples(c.raw, w, h, 3, depth) < entries).any()
    # a tRNS of a length that does not fit the colour type: ignored
    for colour, depth, n in ((0, 8, 3), (0, 16, 6), (2, 8, 2), (2, 16, 7), (3, 4, 17), (3, 8, 257), (4, 8, 2), (6, 8, 6), (6, 16, 8)):
        plte = full(depth) if colour == 3 else b""
        add("unfitting trns", colour, depth, 17, 2, plte, bytes(n))  # (zeros: a key that fitted would match the zero samples)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def facts():
    """What the table is there for (tests/test_pngpix_cpu.py asserts it)."""
    cs = cases()
    return dict(pairs={(c.colour, c.depth) for c in cs}, widths={c.width for c in cs}, heights={c.height for c in cs},
                pair_heights={(c.colour, c.depth, c.height) for c in cs}, kinds={c.kind for c in cs}, count=len(cs),
                keyed={(c.colour, c.depth) for c in cs if c.kind == "trns" and c.colour != 3 and (c.want[..., 3] == 0).any()})


def subset():
    """A part of the table that spans the pairs and the kinds: for the placement tests and the poison catalogue."""
    cs = cases()
    seen, out = set(), []
    for c in cs[::7] + cs:
        key = (c.colour, c.depth, c.kind)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def damaged():
    """The damage table of tests/_png.py (but the capacity case) between its two good neighbours, in turn:
    [(name, file, the decode calls' status, the pixels the rule gives)]."""
    g = _png.geometry()
    pix = lambda geo, raw: rule(raw, geo[2], geo[3], geo[0], geo[1])
    good = [(g[k].name, g[k].blob, 0, pix(_png._GEOMETRY[k], g[k].want)) for k in (9, 19)]
    assert (g[9], g[19]) == _png.neighbours()
    rows = [good[0]]
    for c in _png.damage():
        if not c.short:
            rows += [(c.name, c.blob, c.status, pix(_png.BASE, c.want) if c.status == 0 else None), good[len(rows) // 2 % 2]]
    return rows


def pack(blobs, first=1, gap=3):
    """The files at odd places of one buffer: (flat, offsets, lengths)."""
    off = np.cumsum([first] + [len(b) + gap for b in blobs])[:-1].astype(np.uint64)
    flat = np.zeros(int(off[-1]) + len(blobs[-1]) + 1, dtype=np.uint8)
    for o, b in zip(off, blobs):
        flat[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return flat, off, np.array([len(b) for b in blobs], dtype=np.uint64)
