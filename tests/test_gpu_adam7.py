"""Adam7-interlaced PNG files on the MI355X (ZES_F_PNG_INTERLACED; k_png_unfilter over the passes, k_png_deinterlace): the
files of tests/_adam7.py — every combination of passes without pixels, every (colour, depth) pair with the pass rows' pad
bits set, a second unfilter band inside a pass, images of several deinterlace tiles, files and outputs at every alignment, damage between good neighbours, the
pixel forms against the non-interlaced path, the launches, poisoned scratch and ZES_F_PIECES.  Expected bytes are the
writer's inputs.  The device form writes into a tensor filled with 0xA5, so every byte outside the images' ranges is
checked; each test uses the alloc form as well."""
import numpy as np
import pytest

import _adam7
import _png

pytestmark = pytest.mark.gpu

NOSPACE = _png.ZES_E_NOSPACE
FLAG = _adam7.ZES_F_PNG_INTERLACED


def pack(blobs, at=0):
    """The files in one array, the first one `at` bytes in, 1 to 5 bytes between them: (array, offsets, lengths)."""
    off, pos = [], at
    for i, b in enumerate(blobs):
        off.append(pos)
        pos += len(b) + 1 + i % 5
    flat = np.zeros(pos, dtype=np.uint8)
    for o, b in zip(off, blobs):
        flat[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return flat, off, [len(b) for b in blobs]


def places(sizes, residue=None):
    """Unaligned, non-overlapping places: a gap of 1 to 13 bytes in front of each; residue(i): the place's offset mod 16."""
    off, at = [], 0
    for i, n in enumerate(sizes):
        at += 1 + (5 * i) % 13
        if residue is not None:
            at += (residue(i) - at) % 16
        off.append(at)
        at += n
    return off, at + 40


def run_dev(z, gpu, cases, at=0, residue=None, flags=FLAG, pix=False, want=None):
    """zes_png_decode_dev (pix: zes_pngpix_dev) into a tensor filled with 0xA5: every status, length and byte checked.
    want[i]: the bytes expected of image i (default: the case's scanlines).  Returns the statuses."""
    import torch

    flat, ioff, ilen = pack([c.blob for c in cases], at)
    t = torch.from_numpy(flat).to(gpu)
    want = [c.want for c in cases] if want is None else want
    sizes = [len(w) if w is not None else 0 for w in want]
    off, room = places(sizes, residue)
    out = torch.full((room,), 0xA5, dtype=torch.uint8, device=gpu)
    fn = z.png_pixels_tensor if pix else z.png_decode_tensor
    got, _, out_len, status, info = fn(t, ioff, ilen, out=out, off=off, flags=flags, cap=sizes)
    host = got.cpu().numpy()
    untouched = np.ones(host.size, dtype=bool)
    for i, c in enumerate(cases):
        assert status[i] == c.status, (c.name, i, status[i], c.status)
        assert out_len[i] == (sizes[i] if status[i] == 0 else 0), (c.name, i, out_len[i])
        untouched[off[i]:off[i] + sizes[i]] = False
        if status[i] == 0:
            assert host[off[i]:off[i] + sizes[i]].tobytes() == want[i], (c.name, i)
            assert _png.info_dict(info[i]) == _png.info_rule(c.blob)[1], c.name
    assert (host[untouched] == 0xA5).all(), "a byte outside the images' ranges was written"
    return status


def run_host(z, cases, flags=FLAG, pix=False, want=None):
    """zes_png_decode_alloc (pix: zes_pngpix_alloc) through the package: every status and every byte checked."""
    res = (z.png_pixels_batch if pix else z.png_decode_batch)([c.blob for c in cases], flags)
    want = [c.want for c in cases] if want is None else want
    for c, w, r in zip(cases, want, res):
        if isinstance(r, Exception):
            assert r.code == c.status, (c.name, r.code, c.status)
        else:
            assert c.status == 0, c.name
            info, rows = r
            assert rows.tobytes() == w, c.name
            assert rows.shape == ((int(info["height"]), int(info["width"]), 4) if pix else (int(info["height"]), int(info["rowbytes"]))), c.name
            assert _png.info_dict(info) == _png.info_rule(c.blob)[1], c.name


def both(z, gpu, cases, **kw):
    st = run_dev(z, gpu, cases, **kw)
    run_host(z, cases, **{k: v for k, v in kw.items() if k in ("flags", "pix", "want")})
    return st


_PIXELS = {}


def plain_pixels(z, cases):
    """The RGBA bytes of the cases' pixels by the existing path: the same scanlines written non-interlaced, no flag.  Made once."""
    key = tuple(c.name for c in cases)
    if key not in _PIXELS:
        res = z.png_pixels_batch([_adam7.plain_of(c).blob for c in cases])
        assert not any(isinstance(r, Exception) for r in res)
        _PIXELS[key] = [r[1].tobytes() for r in res]
    return _PIXELS[key]


def test_every_combination_of_empty_passes(z, gpu):
    g = _adam7.small_grid()
    assert len(g) == 162 and {tuple(bool(pw) for pw, _ in _adam7.pass_dims(w, h)) for w in range(1, 10) for h in range(1, 10)} >= {
        (True, False, False, False, False, False, False), (True,) * 7}
    assert both(z, gpu, g, at=1) == [0] * len(g)


def test_every_colour_and_depth_with_pad_bits_set(z, gpu):
    g = _adam7.pairs()
    assert {c.name.split(" ")[0] + c.name.split(" ")[1] for c in g} == {"c%dd%d" % p for p in _png.PAIRS}
    assert both(z, gpu, g) == [0] * len(g)


def test_band_seams_inside_passes(z, gpu):
    assert _adam7.pass_dims(5, 131)[6][1] == 65 and _adam7.pass_dims(3, 513)[0][1] == 65
    g = _adam7.seams()
    assert both(z, gpu, g, at=3) == [0] * len(g)


def test_images_of_more_than_one_tile(z, gpu):
    """k_png_deinterlace cuts an image into tiles of about 32 KiB of output rows: images of several tiles, the last one short,
    one of them with rows of more 16-byte units than the workgroup has threads; scanlines and pixels, at every alignment."""
    g = _adam7.tiled()
    rows = [_png.shape(*_adam7_header(c))[1:] for c in g]
    assert all(size > 2 * 32768 for _, size in rows) and any(rb // 16 + 2 > 256 for rb, _ in rows) and any(32768 // rb >= 8 for rb, _ in rows)
    assert both(z, gpu, g, at=1, residue=lambda i: (5 + 7 * i) % 16) == [0] * len(g)
    both(z, gpu, g, at=2, residue=lambda i: (4 * i) % 16, pix=True, want=plain_pixels(z, g))


def _adam7_header(c):
    rec = _png.info_rule(c.blob)[1]
    return rec["width"], rec["height"], rec["colour"], rec["depth"]


def test_placement_of_files_and_outputs(z, gpu):
    g = _adam7.pairs()[::2] + _adam7.pairs()[:1]  # 13 x 11, sixteen of them: an output at every residue mod 16
    assert len(g) == 16
    for at in (0, 1, 7):
        run_dev(z, gpu, g, at=at, residue=lambda i: (i + at) % 16)
    wide = _adam7.pairs()[1::2] + _adam7.pairs()[1:2]  # 37 x 19: rows longer than a 16-byte group
    run_dev(z, gpu, wide, at=1, residue=lambda i: (15 - i) % 16)
    run_host(z, g)


def test_mixed_batch_with_damaged_neighbours(z, gpu):
    inter, plain = _adam7.pairs()[7], _png.geometry()[19]
    cases = [inter]
    for k, c in enumerate(_adam7.damaged()):
        cases += [c, plain if k % 2 == 0 else inter]
    cases += [_png.geometry()[9], _adam7.pairs()[20]]
    st = both(z, gpu, cases, at=3)
    assert [s for s in st if s] == [_png.ZES_E_PNG] * 3 + [_png.ZES_E_CHECKSUM]
    # every damaged image alone, and all of them without a good one
    both(z, gpu, _adam7.damaged())
    for c in _adam7.damaged():
        run_dev(z, gpu, [c])


def test_pixel_forms_equal_the_plain_path(z, gpu):
    for g in (_adam7.small_grid(), _adam7.pairs()):
        both(z, gpu, g, at=1, pix=True, want=plain_pixels(z, g))


def launches(z):
    return {name: n for name, _, n in z.last_kernel_times()}


def test_launches(z, gpu):
    import torch

    inter, plain = _adam7.pairs()[::5], _png.geometry()[::6]
    z.set_profiling(True)
    try:
        run_dev(z, gpu, inter)
        names = launches(z)
        assert names.get("k_png_walk") == 1 and names.get("k_png_unfilter") == 1 and names.get("k_png_deinterlace") == 1, names
        run_dev(z, gpu, inter, pix=True, want=plain_pixels(z, inter))
        names = launches(z)
        assert names.get("k_png_unfilter") == 1 and names.get("k_png_deinterlace") == 1 and names.get("k_png_expand") == 1, names
        # no interlaced file in the batch: the flag changes no launch
        run_dev(z, gpu, plain, flags=0)
        without = launches(z)
        run_dev(z, gpu, plain)
        assert launches(z) == without and "k_png_deinterlace" not in without
        # the sizing pass costs the walk alone
        flat, ioff, ilen = pack([c.blob for c in inter])
        t = torch.from_numpy(flat).to(gpu)
        zero = [0] * len(inter)
        _, _, out_len, status, _ = z.png_decode_tensor(t, ioff, ilen, out=torch.zeros(16, dtype=torch.uint8, device=gpu), off=zero, cap=zero, flags=FLAG)
        assert status == [NOSPACE] * len(inter) and out_len == [len(c.want) for c in inter]
        assert launches(z) == {"k_png_walk": 1}
        # without the flag: refused, the walk alone
        _, _, out_len, status, _ = z.png_decode_tensor(t, ioff, ilen, out=torch.zeros(1 << 16, dtype=torch.uint8, device=gpu), off=zero, flags=0)
        assert status == [_png.ZES_E_UNSUPPORTED] * len(inter) and out_len == zero
        assert launches(z) == {"k_png_walk": 1}
    finally:
        z.set_profiling(False)


def test_step_1_in_the_device_form(z, gpu):
    """Fi above 0xFFFFFFFF where the file rule's F is not: ZES_E_UNSUPPORTED behind the walk, between files that decode."""
    huge = _png.Case("2 x (2^31 - 1), 1 bit", _adam7.wrap(2, 0x7fffffff, 0, 1, b"x"), None, _png.ZES_E_UNSUPPORTED)
    assert _adam7.fi(2, 0x7fffffff, 0, 1) > 0xFFFFFFFF and _png.info_rule(huge.blob)[0] == 0
    a, b = _adam7.pairs()[3], _adam7.pairs()[12]
    z.set_profiling(True)
    try:
        assert run_dev(z, gpu, [a, huge, b]) == [0, _png.ZES_E_UNSUPPORTED, 0]
        assert launches(z).get("k_png_deinterlace") == 1
        assert run_dev(z, gpu, [huge]) == [_png.ZES_E_UNSUPPORTED]
        assert launches(z) == {"k_png_walk": 1}
        assert run_dev(z, gpu, [huge], pix=True, want=[None]) == [_png.ZES_E_UNSUPPORTED]
    finally:
        z.set_profiling(False)
    res = z.png_decode_batch([a.blob, huge.blob, b.blob], FLAG)
    assert res[1].code == _png.ZES_E_UNSUPPORTED and res[0][1].tobytes() == a.want and res[2][1].tobytes() == b.want


def test_poisoned_scratch(z, gpu):
    """Every call, device form and alloc form, right behind a poison of its own: the scanlines of every (colour, depth) pair,
    and the pixel forms over those and over the 1..9 x 1..9 grid, whose slots of passes and scanlines are the smallest."""
    g, grid = _adam7.pairs(), _adam7.small_grid()
    want, want_grid = plain_pixels(z, g), plain_pixels(z, grid)  # (before the first poison: these are calls of their own)
    for word in (0, 0xFFFFFFFF, 0xA5A5A5A5):
        for cases, kw in ((g, {}), (g, dict(pix=True, want=want)), (grid, dict(pix=True, want=want_grid))):
            z.stage_poison(word)
            assert run_dev(z, gpu, cases, at=1, **kw) == [0] * len(cases)
            z.stage_poison(word)
            run_host(z, cases, **kw)
    z.trim()
    assert z.pool_bytes() == 0


def test_pieces_flag_gives_the_same_bytes(z, gpu):
    g = _adam7.pairs()
    assert both(z, gpu, g, flags=FLAG | _adam7.ZES_F_PIECES) == [0] * len(g)
