"""The TIFF reader on the GPU: every case of tests/_tiff.py's table through the device form (zes_tiff_index_dev,
zes_tiff_read_dev: the file at an odd offset, the result at d_out offsets 0, 1 and 3 inside a tensor of sentinel bytes, none of
which may change outside the rectangle's range) and the host form (zes_tiff_read_alloc), against the helper's independent
reader; rectangles of the tiled cases with the segments they touch; one tile of twelve broken each way; the kernel names of a
4-tile and a 256-tile call; the second directory of a file."""
import numpy as np
import pytest

import _tiff as T
import _tiff_poison  # noqa: F401  (the catalogue entries and COVERS / EXEMPT lines of the new entry points)

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def on_device(f, gpu, lead=1):
    import torch

    return torch.from_numpy(np.concatenate([np.zeros(lead, dtype=np.uint8), np.frombuffer(bytes(f), dtype=np.uint8)])).to(gpu)[lead:]


def dev_read(z, gpu, f, dir=0, rect=None, at=0, flags=0, lead=1):
    """(pixel bytes, seg_status, status) of the device form, the bytes around the result checked against the sentinel."""
    import torch

    t = on_device(f, gpu, lead)
    idx = z.tiff_index_tensor(t, dir)
    info = idx[0]
    rec, off, ln, dirs = T.rule(f, dir)
    assert info == dict(rec, dirs=dirs) and list(idx[1]) == off and list(idx[2]) == ln
    w, h = (rec["width"], rec["height"]) if rect is None else rect[2:]
    size = w * h * rec["spp"] * rec["bits"] // 8
    room = torch.full((at + size + 41,), SENTINEL, dtype=torch.uint8, device=gpu)
    pix, st, rc = z.tiff_read_tensor(t, idx, rect, out=room[at:at + size], flags=flags)
    host = room.cpu().numpy()
    assert pix.shape == (h, w, rec["spp"] * rec["bits"] // 8)
    assert (host[:at] == SENTINEL).all() and (host[at + size:] == SENTINEL).all(), "a byte outside the rectangle's range was written"
    return host[at:at + size], st, rc


def check_both_forms(z, gpu, name, f, want, dir=0, rect=None, offsets=(0, 1, 3)):
    want_bytes = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    for at in offsets:
        got, st, rc = dev_read(z, gpu, f, dir, rect, at)
        assert rc == 0 and not st.any(), (name, at, rc, st)
        assert (got == want_bytes).all(), (name, at, np.flatnonzero(got != want_bytes)[:8])
    host = z.tiff_read(f, dir, rect)
    assert host.shape == want.shape and host.dtype == want.dtype and (host == want).all(), name


@pytest.mark.parametrize("layout", T.LAYOUTS, ids=lambda lay: "-".join(map(str, lay)))
@pytest.mark.parametrize("bits", (8, 16, 32))
def test_layouts_and_kinds(z, gpu, layout, bits):
    n = 0
    for name, kw in T.grid(layouts=(layout,), depths=(bits,)):
        f, px = T.make(**kw)
        check_both_forms(z, gpu, name, f, px)
        n += 1
    assert n == 3 * 2 * len(T.CODINGS)


def test_long_rows_narrow_images_and_one_tile(z, gpu):
    for name, kw in T.extra_cases():
        f, px = T.make(**kw)
        check_both_forms(z, gpu, name, f, px)
        f, px = T.make(odd=False, **kw)
        check_both_forms(z, gpu, name + ", even positions", f, px, offsets=(0,))
    # the file at a 16-byte aligned place too (Compression 1 reads the segments where they lie)
    f, px = T.make(w=37, h=23, spp=3, bits=16, layout=("tiles", 16, 16), order="MM", compression=1, predictor=1, odd=False)
    got, st, rc = dev_read(z, gpu, f, lead=16)
    assert rc == 0 and (got == px.view(np.uint8).reshape(-1)).all()


def test_signed_and_float_samples(z, gpu):
    s = (np.arange(37 * 23 * 2, dtype=np.int64).reshape(23, 37, 2) * 37 - 30000).astype(np.int16)
    got = z.tiff_read(T.write([T.page(s, ("tiles", 16, 16), 8, 2, sample_format=2)], "MM", True))
    assert got.dtype == np.int16 and (got == s).all()
    fl = np.linspace(-3, 3, 23 * 37, dtype=np.float32).reshape(23, 37, 1)
    got = z.tiff_read(T.write([T.page(fl, ("strips", 5), 32946, 1, sample_format=3)], "II", True))
    assert got.dtype == np.float32 and (got == fl).all()
    i8 = (np.arange(16 * 16 * 3).reshape(16, 16, 3) % 251 - 120).astype(np.int8)
    got = z.tiff_read(T.write([T.page(i8, ("tiles", 16, 16), 1, 1, sample_format=2)], "II"))
    assert got.dtype == np.int8 and (got == i8).all()


@pytest.mark.parametrize("layout", T.LAYOUTS[:2], ids=lambda lay: "-".join(map(str, lay)))
def test_rectangles(z, gpu, layout):
    kinds = [dict(spp=3, bits=8, order="II", compression=8, predictor=2), dict(spp=1, bits=16, order="MM", compression=32946, predictor=2),
             dict(spp=4, bits=32, order="MM", compression=8, predictor=1), dict(spp=3, bits=16, order="II", compression=1, predictor=1)]
    for kind in kinds:
        f, px = T.make(w=37, h=23, layout=layout, **kind)
        rec, off, ln, _ = T.rule(f)
        for name, rect in T.rectangles(rec).items():
            x, y, w, h = rect
            want = px[y:y + h, x:x + w]
            assert (T.decode(f, 0, rect) == want).all()
            check_both_forms(z, gpu, name, f, want, rect=rect, offsets=(0, 3) if name == "whole" else (1,))
            # the host form uploads the touched segments and nothing else
            hit = T.touched(rec, rect)
            assert z.last_tiff_read() == (len(hit), sum(ln[k] for k in hit)), name
        hit = T.touched(rec, T.rectangles(rec)["straddling four tiles"])
        assert len(hit) == 4 and len(T.touched(rec, T.rectangles(rec)["inside one tile, off its column 0"])) == 1
    # a segment that is not touched is not looked at: its status stays ZES_OK although its stream is rubbish
    last = rec["across"] * rec["down"] - 1
    rubbish = lambda k, raw: b"\x00\x01\x02" if k == last else __import__("zlib").compress(raw, 6)
    f, px = T.make(w=37, h=23, layout=layout, compress=rubbish, **kinds[0])
    got, st, rc = dev_read(z, gpu, f, rect=(0, 0, 20, 10))
    assert rc == 0 and not st.any() and (got == px[0:10, 0:20].reshape(-1)).all()
    got, st, rc = dev_read(z, gpu, f)
    assert rc == -1 and st[last] == rc and not np.delete(st, last).any()  # (ZES_E_NOT_DEFLATE: a stream keeps its inflate status)
    # rectangles the call refuses, and a capacity below the rectangle's size
    t = on_device(f, gpu)
    idx = z.tiff_index_tensor(t)
    for rect in ((0, 0, 0, 1), (30, 0, 8, 1), (0, 23, 1, 1)):
        with pytest.raises(z.ZlibEsError) as e:
            z.tiff_read_tensor(t, idx, rect)
        assert e.value.code == T.E_ARG
    import torch

    with pytest.raises(z.ZlibEsError) as e:
        z.tiff_read_tensor(t, idx, (0, 0, 4, 4), out=torch.zeros(47, dtype=torch.uint8, device=gpu))
    assert e.value.code == T.E_NOSPACE and e.value.need == 48


def test_one_broken_tile_of_twelve(z, gpu, oracle):
    cases = T.segment_damage(oracle)
    assert len(cases) == 8 and {w for _, _, _, _, w in cases} >= {T.E_TIFF, T.E_CHECKSUM}
    for name, f, px, bad, want in cases:
        assert want != 0, name
        rec = T.rule(f)[0]
        got, st, rc = dev_read(z, gpu, f, at=1)
        print(name, rc, want)
        assert rc == want and st[bad] == want and not np.delete(st, bad).any(), (name, rc, want, st)
        # every other tile's pixels are right
        sy, sx = divmod(bad, rec["across"])
        keep = np.ones(px.shape, dtype=bool)
        keep[sy * 16:(sy + 1) * 16, sx * 16:(sx + 1) * 16] = False
        assert (got.reshape(px.shape)[keep] == px[keep]).all(), name
        with pytest.raises(z.ZlibEsError) as e:
            z.tiff_read(f)
        assert e.value.code == want, name
        # a rectangle beside the broken tile does not see it
        assert (z.tiff_read(f, rect=(0, 0, 16, 48)) == px[:, :16]).all(), name
    # two broken tiles: the first in segment order decides
    import zlib

    px = T.pixels(64, 48, 3, 8, 9)
    brk = lambda k, raw: zlib.compress(raw + b"\x00", 6) if k == 9 else zlib.compress(raw, 6)[:-2] if k == 3 else zlib.compress(raw, 6)
    f = T.write([T.page(px, ("tiles", 16, 16), 8, 2, compress=brk)], "II", True)
    got, st, rc = dev_read(z, gpu, f)
    assert rc == T.E_CHECKSUM and st[3] == T.E_CHECKSUM and st[9] == T.E_TIFF


def launches(z, gpu, f):
    z.set_profiling(True)
    try:
        got, st, rc = dev_read(z, gpu, f)
        assert rc == 0 and not st.any()
        return got, [(name, k) for name, _, k in z.last_kernel_times()]
    finally:
        z.set_profiling(False)


def test_kernel_names_of_4_tiles_and_of_256_are_the_same_list(z, gpu, oracle):
    """The streams are the project's own format (the CPU oracle's deflate), which the block-parallel tier decodes as one batch at
    any count: which tiers another encoder's streams reach is decided stream by stream."""
    reference = lambda k, raw: oracle.deflate(np.frombuffer(raw, dtype=np.uint8)).tobytes()
    names = {}
    for side in (32, 256):
        px = np.random.default_rng(side).integers(0, 256, size=(side, side, 4), dtype=np.uint8)
        f = T.write([T.page(px, ("tiles", 16, 16), 8, 2, compress=reference)], "II", True)
        got, names[side] = launches(z, gpu, f)
        print(side, names[side])
        assert (got == px.reshape(-1)).all()
        assert names[side][-1] == ("k_tiff_place", 1) and [n for n, _ in names[side]].count("k_tiff_place") == 1
    assert [n for n, _ in names[32]] == [n for n, _ in names[256]]
    assert [k for _, k in names[32]] == [k for _, k in names[256]]  # and no kernel runs once per tile


def test_reference_made_and_zlib_streams_in_one_image(z, gpu, oracle):
    import zlib

    mixed = lambda k, raw: oracle.deflate(np.frombuffer(raw, dtype=np.uint8)).tobytes() if k % 3 == 1 else zlib.compress(raw, 1 + k % 9)
    for kw in (dict(spp=3, bits=16, order="MM", layout=("tiles", 16, 16)), dict(spp=1, bits=8, order="II", layout=("strips", 5))):
        f, px = T.make(w=37, h=23, compression=8, predictor=2, compress=mixed, **kw)
        check_both_forms(z, gpu, str(kw), f, px, offsets=(1,))
        check_both_forms(z, gpu, str(kw), f, px, offsets=())
    f, px = T.make(w=37, h=23, spp=4, bits=8, order="II", layout=("tiles", 16, 16), compression=8, predictor=2)
    got, st, rc = dev_read(z, gpu, f, flags=z.ZES_F_PIECES)
    assert rc == 0 and (got == px.reshape(-1)).all()


def test_second_directory(z, gpu):
    f, (a, b) = T.two_directories()
    check_both_forms(z, gpu, "first", f, a, dir=0, offsets=(0,))
    check_both_forms(z, gpu, "second", f, b, dir=1, offsets=(3,))
    check_both_forms(z, gpu, "second, a rectangle", f, b[9:30, 2:19], dir=1, rect=(2, 9, 17, 21), offsets=(1,))
    with pytest.raises(z.ZlibEsError) as e:
        z.tiff_read(f, 2)
    assert e.value.code == T.E_ARG
