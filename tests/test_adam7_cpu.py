"""Adam7 without a GPU: the interlaced writer of tests/_adam7.py against PIL and against an independent per-pixel
deinterlace, the interlaced filtered size Fi, and what the decode calls do with ZES_F_PNG_INTERLACED before they reach a
device (the flag's value, which calls take it, the step-1 rule on the host)."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import _adam7
import _png

ARG, UNS, PNG, DEVICE = _png.ZES_E_ARG, _png.ZES_E_UNSUPPORTED, _png.ZES_E_PNG, _png.ZES_E_DEVICE
FLAG = 128


def body_of(blob):
    return zlib.decompress(b"".join(blob[d:d + n] for _, t, d, n in _png.chunks_of(blob) if t == b"IDAT"))


def header_of(blob):
    rec = _png.info_rule(blob)[1]
    return rec["width"], rec["height"], rec["colour"], rec["depth"]


def test_pil_reads_the_writer():
    Image = pytest.importorskip("PIL.Image")
    n = 0
    for colour, depth, mode in ((2, 8, "RGB"), (0, 8, "L"), (6, 8, "RGBA"), (3, 8, "P"), (0, 1, "1"), (4, 8, "LA")):
        for w in range(1, 10):
            for h in range(1, 10):
                raw = _adam7.pixels(w, h, colour, depth, 100 * w + h)
                filters = [[(p + r + w) % 5 for r in range(ph)] for p, (_, ph) in enumerate(_adam7.pass_dims(w, h))]
                blob = _adam7.write(w, h, colour, depth, raw, filters, pad_ones=depth < 8)
                im = Image.open(io.BytesIO(blob))
                im.load()
                assert (im.mode, im.size) == (mode, (w, h)) and im.tobytes() == raw, (mode, w, h)
                n += 1
    assert n == 486


def test_writer_equals_a_per_pixel_deinterlace_on_every_pair():
    cases = _adam7.pairs() + _adam7.small_grid()[::5] + _adam7.seams()[::9]
    assert {header_of(c.blob)[2:] for c in cases} == set(_png.PAIRS)
    for c in cases:
        w, h, colour, depth = header_of(c.blob)
        body = body_of(c.blob)
        assert len(body) == _adam7.fi(w, h, colour, depth), c.name
        assert _adam7.deinterlace(body, w, h, colour, depth) == c.want, c.name
    for c in _adam7.damaged()[:3]:
        assert _adam7.deinterlace(body_of(c.blob), *header_of(c.blob)) is None, c.name


def test_pass_geometry():
    assert _adam7.pass_dims(1, 1) == [(1, 1)] + [(0, 0)] * 6
    assert _adam7.pass_dims(8, 8) == [(1, 1), (1, 1), (2, 1), (2, 2), (4, 2), (4, 4), (8, 4)]
    assert _adam7.pass_dims(5, 1) == [(1, 1), (1, 1), (0, 0), (1, 1), (0, 0), (2, 1), (0, 0)]
    for w in range(1, 20):
        for h in range(1, 20):
            assert sum(pw * ph for pw, ph in _adam7.pass_dims(w, h)) == w * h
    assert _adam7.fi(1, 1, 6, 8) == 5 and _adam7.fi(8, 8, 0, 8) == 1 * 2 + 1 * 2 + 1 * 3 + 2 * 3 + 2 * 5 + 4 * 5 + 4 * 9
    # Fi can exceed the F that the file rule bounds
    assert 0x7fffffff * (1 + 1) <= 0xFFFFFFFF < _adam7.fi(2, 0x7fffffff, 0, 1)


def raw_alloc(z, pix, blobs, count=None, flags=0):
    calls = []

    def cb(_user, i, n):
        calls.append((i, n))
        return None

    arrs = [np.frombuffer(b, dtype=np.uint8) for b in blobs]
    cnt = len(arrs) if count is None else count
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data if a.size else None for a in arrs])
    ln = np.array([a.size for a in arrs] + [0], dtype=np.uint64)
    ol = np.zeros(max(cnt, 1), dtype=np.uint64)
    st = np.full(max(cnt, 1), 99, dtype=np.int32)
    fn = z.lib().zes_pngpix_alloc if pix else z.lib().zes_png_decode_alloc
    rc = fn(ptrs, ln.ctypes.data, cnt, z.ALLOC_FN(cb), None, ol.ctypes.data, st.ctypes.data, None, flags)
    return rc, [int(x) for x in st[:cnt]], calls


def raw_dev(z, pix, n, flags=0):
    """The device forms with pointers that are never followed (only for calls that end before the device)."""
    arr = {k: np.zeros(n + 1, dtype=np.uint64) for k in ("in_off", "in_len", "out_off", "out_cap", "out_len")}
    arr["in_len"][:n] = 100
    st = np.full(n + 1, 99, dtype=np.int32)
    p = lambda k: arr[k].ctypes.data
    fn = z.lib().zes_pngpix_dev if pix else z.lib().zes_png_decode_dev
    return fn(0x1000, p("in_off"), p("in_len"), n, 0x2000, p("out_off"), p("out_cap"), p("out_len"), st.ctypes.data, None, flags)


def test_flag_value_and_who_takes_it(z):
    import torch

    assert z.ZES_F_PNG_INTERLACED == 128 == _adam7.ZES_F_PNG_INTERLACED
    good = _adam7.pairs()[0].blob
    for pix in (False, True):
        for flags in (FLAG, FLAG | 4):
            assert raw_alloc(z, pix, [good], count=0, flags=flags) == (0, [], [])
            assert raw_alloc(z, pix, [], flags=flags) == (0, [], [])
            assert raw_dev(z, pix, 0, flags=flags) == 0
        for flags in (FLAG | 1, FLAG | 8, FLAG | 16, FLAG | 32, FLAG | 64, FLAG | 256):
            assert raw_alloc(z, pix, [good], flags=flags)[0] == ARG
            assert raw_dev(z, pix, 1, flags=flags) == ARG
    # the calls that do not decode files keep refusing it
    a = np.frombuffer(good, dtype=np.uint8)
    rec = np.zeros(1, dtype=z.PNG_INFO)
    assert z.lib().zes_png_info_get(a.ctypes.data, a.size, rec.ctypes.data, FLAG) == ARG
    assert z.lib().zes_png_info_get(a.ctypes.data, a.size, rec.ctypes.data, 0) == 0 and int(rec[0]["interlace"]) == 1
    img = np.zeros(16, dtype=np.uint8)
    img.view(np.uint32)[:2] = (4, 3)
    img[8] = 8
    one = np.array([12, 0], dtype=np.uint64)
    zero, cap = np.zeros(2, dtype=np.uint64), np.full(2, 1 << 40, dtype=np.uint64)
    ol, st = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.int32)
    expand = lambda flags: z.lib().zes_pngpix_expand_dev(0x1000, zero.ctypes.data, one.ctypes.data, img.ctypes.data, None, 1, 0x2000, zero.ctypes.data,
                                                         cap.ctypes.data, ol.ctypes.data, st.ctypes.data, flags)
    assert expand(FLAG) == ARG and expand(FLAG | 4) == ARG
    if not torch.cuda.is_available():  # a file that passes step 1 under the flag is a call for the device
        for pix in (False, True):
            assert raw_alloc(z, pix, [good], flags=FLAG)[0] == DEVICE
            assert raw_alloc(z, pix, [good], flags=FLAG | 4)[0] == DEVICE


def test_step_1_on_the_host(z):
    good = _adam7.pairs()[0].blob
    huge = _adam7.wrap(2, 0x7fffffff, 0, 1, b"x")  # the file rule passes it (F = 2^32 - 2); its seven passes hold more
    assert _png.info_rule(huge)[0] == 0 and z.png_info(huge)["interlace"] == 1
    bad = [c.blob for c in _png.damage()[:6]] + [huge]
    want = [PNG] * 5 + [UNS, UNS]
    for pix in (False, True):
        # without the flag an interlaced file is refused as before, on the host
        assert raw_alloc(z, pix, [good, huge]) == (0, [UNS, UNS], [])
        assert raw_alloc(z, pix, [good, huge], flags=4) == (0, [UNS, UNS], [])
        # with it, a batch that the rule rejects is answered without a device and without the allocator
        assert raw_alloc(z, pix, bad, flags=FLAG) == (0, want, [])
        assert raw_alloc(z, pix, [huge], flags=FLAG | 4) == (0, [UNS], [])
    res = z.png_decode_batch(bad, z.ZES_F_PNG_INTERLACED)
    assert [r.code for r in res] == want
    with pytest.raises(z.ZlibEsError) as e:
        z.png_pixels(huge, z.ZES_F_PNG_INTERLACED)
    assert e.value.code == UNS
    with pytest.raises(z.ZlibEsError) as e:
        z.png_decode(good)
    assert e.value.code == UNS
