"""PNG files to 8-bit RGBA pixels on the MI355X (zes_pngpix_dev, zes_pngpix_alloc, zes_pngpix_expand_dev; k_png_expand): the
case table of tests/_pngpix.py — every (colour, depth) pair at widths that reach a row's padding bits, four-pixel groups that
straddle bytes and dwords and rows shorter than one store group, heights on either side of an unfilter band, tRNS keys that
match and keys that must not, short palettes — against the numpy rule.  The device forms write into tensors filled with
0xA5, so every byte outside the images' ranges is checked."""
import numpy as np
import pytest

import _png
import _pngpix as X
import _pngpix_poison  # noqa: F401  (adds the pixel forms' entries to the poison catalogue, tests/_poison_cases.py)

pytestmark = pytest.mark.gpu

NOSPACE = _png.ZES_E_NOSPACE


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def rows_of(cases):
    return [(c.name, c.blob, 0, c.want) for c in cases]


def places(sizes, residue=None, gap=True):
    """Non-overlapping places: a gap of 1 to 13 bytes in front of each (none: back to back); residue(i): the place mod 16."""
    off, at = [], 0
    for i, n in enumerate(sizes):
        at += 1 + (5 * i) % 13 if gap else 0
        if residue is not None:
            at += (residue(i) - at) % 16
        off.append(at)
        at += n
    return off, at + 40


def run_dev(z, gpu, rows, flags=0, residue=None, gap=True, first=1, short=(), info_of=None):
    """zes_pngpix_dev into a tensor filled with 0xA5: every status, length, byte and record checked.  rows: (name, file,
    status, pixels); short: the images whose capacity is one byte short.  Returns the statuses."""
    import torch

    flat, ioff, ilen = X.pack([r[1] for r in rows], first=first)
    sizes = [_png.info_rule(r[1])[1] for r in rows]
    sizes = [4 * s["width"] * s["height"] if s else 0 for s in sizes]
    off, room = places(sizes, residue, gap)
    cap = [n - 1 if i in short else n for i, n in enumerate(sizes)]
    out = torch.full((room,), 0xA5, dtype=torch.uint8, device=gpu)
    got, _, out_len, status, info = z.png_pixels_tensor(dev(flat, gpu), ioff, ilen, out=out, off=off, flags=flags, cap=cap)
    host = got.cpu().numpy()
    untouched = np.ones(host.size, dtype=bool)
    for i, (name, blob, st, want) in enumerate(rows):
        exp = NOSPACE if i in short and st == 0 else st
        assert status[i] == exp or (isinstance(exp, tuple) and status[i] in exp), (name, i, status[i], exp)
        assert out_len[i] == (sizes[i] if status[i] in (0, NOSPACE) else 0), (name, i, out_len[i])
        if i not in short:
            untouched[off[i]:off[i] + sizes[i]] = False  # (a failed image's range is unspecified)
        if status[i] == 0:
            px = host[off[i]:off[i] + sizes[i]]
            assert px.size == want.size and (px == want.reshape(-1)).all(), (name, i, np.flatnonzero(px != want.reshape(-1))[:4])
    assert (host[untouched] == 0xA5).all(), "a byte outside the images' ranges was written"
    if info_of is not None:
        info_of.append(info)
    return status


def run_host(z, rows, flags=0):
    """zes_pngpix_alloc through the package: every status, shape and byte checked.  Returns the records."""
    res = z.png_pixels_batch([r[1] for r in rows], flags)
    for (name, blob, st, want), r in zip(rows, res):
        if isinstance(r, Exception):
            assert r.code == st or (isinstance(st, tuple) and r.code in st), (name, r.code, st)
        else:
            info, rgba = r
            assert st == 0 and rgba.shape == want.shape == (int(info["height"]), int(info["width"]), 4) and (rgba == want).all(), name
    return [None if isinstance(r, Exception) else r[0] for r in res]


@pytest.fixture(scope="module")
def decoded(z, gpu):
    """The case table through zes_png_decode_dev, once: (scanlines on the device, off, out_len, status, info)."""
    flat, ioff, ilen = X.pack([c.blob for c in X.cases()])
    return z.png_decode_tensor(dev(flat, gpu), ioff, ilen)


@pytest.mark.parametrize("flags", [0, 4], ids=["default", "pieces"])
def test_case_table_both_forms(z, gpu, decoded, flags):
    rows = rows_of(X.cases())
    infos = []
    assert run_dev(z, gpu, rows, flags=flags, info_of=infos) == [0] * len(rows)
    recs = run_host(z, rows, flags)
    # the records are the decode calls'
    _, _, _, status, info = decoded
    assert status == [0] * len(rows)
    assert infos[0].tobytes() == info.tobytes()
    # (the alloc form sees each file from its first byte, as zes_png_decode_alloc does: the same positions)
    assert b"".join(r.tobytes() for r in recs) == info.tobytes()
    assert [_png.info_dict(r) for r in recs[::29]] == [_png.info_rule(c.blob)[1] for c in X.cases()[::29]]


def test_expand_over_the_decoded_scanlines(z, gpu, decoded):
    """zes_pngpix_expand_dev over what zes_png_decode_dev left on the device: the file path's pixels, for every image that
    the writer's records can describe; the filter field says nothing."""
    import torch

    lines, off, out_len, status, _ = decoded
    idx = [i for i, c in enumerate(X.cases()) if c.fits]
    cs = [X.cases()[i] for i in idx]
    assert len(cs) == len(X.cases()) - 9
    img = np.zeros(len(cs), dtype=z.PNGW_IMAGE)
    for k, c in enumerate(cs):
        img[k] = c.record()
        img[k]["filter"] = (0, 5, 9, 255)[k % 4]
    sizes = [c.want.size for c in cs]
    ooff, room = places(sizes)
    out = torch.full((room,), 0xA5, dtype=torch.uint8, device=gpu)
    z.set_profiling(True)
    try:
        _, _, got_len, st = z.png_expand_tensor(lines, [off[i] for i in idx], [out_len[i] for i in idx], img, b"".join(c.plte + c.trns for c in cs), out=out, off=ooff)
        assert [(name, n) for name, _, n in z.last_kernel_times()] == [("k_png_expand", 1)]  # that one launch and nothing else
        assert z.last_inflate_tier() == 0
    finally:
        z.set_profiling(False)
    assert st == [0] * len(cs) and got_len == sizes
    host = out.cpu().numpy()
    untouched = np.ones(host.size, dtype=bool)
    for c, o, n in zip(cs, ooff, sizes):
        assert (host[o:o + n] == c.want.reshape(-1)).all(), c.name
        untouched[o:o + n] = False
    assert (host[untouched] == 0xA5).all(), "a byte outside the images' ranges was written"


def test_expand_statuses_beside_good_images(z, gpu):
    """A refused record, an image without room and a null output between good images: the good ones come out, nothing else is written."""
    import torch

    cs = [c for c in X.subset() if c.fits][:9]
    flat, ioff, ilen = X.pack([c.raw for c in cs], first=3, gap=1)
    img = np.zeros(len(cs), dtype=z.PNGW_IMAGE)
    for k, c in enumerate(cs):
        img[k] = c.record()
    img[2]["depth"] = 3
    ilen[5] += 1
    sizes = [c.want.size for c in cs]
    cap = list(sizes)
    cap[7] -= 1
    ooff, room = places(sizes)
    out = torch.full((room,), 0xA5, dtype=torch.uint8, device=gpu)
    _, _, got_len, st = z.png_expand_tensor(dev(flat, gpu), ioff, ilen, img, b"".join(c.plte + c.trns for c in cs), out=out, off=ooff, cap=cap)
    assert st == [0, 0, -18, 0, 0, -18, 0, NOSPACE, 0] and got_len == [n if s in (0, NOSPACE) else 0 for n, s in zip(sizes, st)]
    host = out.cpu().numpy()
    untouched = np.ones(host.size, dtype=bool)
    for c, o, n, s in zip(cs, ooff, sizes, st):
        if s == 0:
            assert (host[o:o + n] == c.want.reshape(-1)).all(), c.name
            untouched[o:o + n] = False
    assert (host[untouched] == 0xA5).all()
    # no output at all: every image that passes the checks is ZES_E_NOSPACE with its size, and nothing runs
    res = z.png_expand_tensor(dev(flat, gpu), ioff, ilen, img, b"".join(c.plte + c.trns for c in cs), out=None, off=ooff, cap=cap)
    assert res[3] == [NOSPACE if s != -18 else -18 for s in st] and res[2] == got_len


def test_outputs_at_every_residue_and_back_to_back(z, gpu):
    rows = rows_of(X.subset())
    assert {(c.colour, c.depth) for c in X.subset()} == set(_png.PAIRS)
    for r in range(16):  # every image of the call at residue r, then r + 1, ... in turn
        run_dev(z, gpu, rows, residue=(lambda i, r=r: r) if r % 2 else (lambda i, r=r: (r + i) % 16), first=r)
    # back to back, image i + 1 where image i ends: from a 16-byte boundary, from a dword boundary, and from odd bytes (the byte path)
    import torch

    flat, ioff, ilen = X.pack([r[1] for r in rows])
    t = dev(flat, gpu)
    sizes = [r[3].size for r in rows]
    for start in (0, 4, 1, 2):
        off = np.concatenate([[start], start + np.cumsum(sizes)[:-1]])
        end = int(off[-1]) + sizes[-1]
        out = torch.full((end + 16,), 0xA5, dtype=torch.uint8, device=gpu)
        _, _, out_len, status, _ = z.png_pixels_tensor(t, ioff, ilen, out=out, off=off)
        host = out.cpu().numpy()
        assert status == [0] * len(rows) and (host[:start] == 0xA5).all() and (host[end:] == 0xA5).all()
        for (name, _, _, want), o, n in zip(rows, off, sizes):
            assert (host[int(o):int(o) + n] == want.reshape(-1)).all(), (start, name)


def test_damage_between_good_neighbours(z, gpu):
    rows = X.damaged()
    good = [i for i, r in enumerate(rows) if r[2] == 0]
    st = run_dev(z, gpu, rows, first=3, short=(good[2],))
    assert st.count(0) == len(good) - 1 and st.count(NOSPACE) == 1
    # the decode calls' statuses, image by image
    flat, ioff, ilen = X.pack([r[1] for r in rows], first=3)
    ref = z.png_decode_tensor(dev(flat, gpu), ioff, ilen)[3]
    for i, (a, b) in enumerate(zip(st, ref)):
        assert a == b or i == good[2] or (isinstance(rows[i][2], tuple) and a in rows[i][2] and b in rows[i][2]), (rows[i][0], a, b)
    run_host(z, rows)
    bad = [r for r in rows if r[2] != 0]
    run_dev(z, gpu, bad)  # a batch in which every image fails
    run_host(z, bad)


PNG_STEPS = ("k_png_walk", "k_crc32_seg", "k_adler_seg", "k_png_unfilter", "k_png_expand")


def eight():
    """Eight images of 65 rows that span the colour types; the fourth is a palette image."""
    tall = [c for c in X.cases() if c.height == 65 and c.width >= 17]
    cs = tall[::len(tall) // 8][:8]
    assert len(cs) == 8 and {c.colour for c in cs} >= {0, 2, 3, 4} and cs[3].colour == 3
    return cs


def launches(z, gpu, batch):
    """[(kernel name, launches)] of one profiled zes_pngpix_dev call over the batch, every byte checked."""
    z.set_profiling(True)
    try:
        run_dev(z, gpu, batch)
        return [(name, k) for name, _, k in z.last_kernel_times()]
    finally:
        z.set_profiling(False)


def own_streams(z, cs):
    """The files with zlib streams of the project's own encoder: the block-parallel tier decodes them as one batch at any
    count.  (Fewer than 16 short streams of another encoder go through the inflate driver's per-buffer tiers, a launch each.)"""
    reference = lambda filtered: z.deflate(np.frombuffer(filtered, dtype=np.uint8)).tobytes()
    return [(c.name, c.file(reference), 0, c.want) for c in cs]


def test_sizing_pass_and_launch_accounting(z, gpu):
    import torch

    cs = eight()
    z.set_profiling(True)
    try:
        flat, ioff, ilen = X.pack([c.blob for c in cs])
        zero = [0] * len(cs)
        _, _, out_len, status, _ = z.png_pixels_tensor(dev(flat, gpu), ioff, ilen, out=torch.zeros(16, dtype=torch.uint8, device=gpu), off=zero, cap=zero)
        assert status == [NOSPACE] * len(cs) and out_len == [c.want.size for c in cs]  # the pixel size, not the scanlines'
        assert {name: n for name, _, n in z.last_kernel_times()} == {"k_png_walk": 1}  # the sizing pass costs the walk alone
        # nothing to decode: no launch
        assert z.png_pixels_tensor(dev(flat, gpu), [], [])[2:4] == ([], [])
        assert z.last_kernel_times() == [] and z.last_inflate_tier() == 0
    finally:
        z.set_profiling(False)
    # one image, eight, and eight with CPython's streams: every PNG step is one launch, k_png_expand among them, and the last one
    own = own_streams(z, cs)
    got = {}
    for n, batch in ((1, own[3:4]), (8, own), ("zlib", rows_of(cs))):
        got[n] = launches(z, gpu, batch)
        print(n, got[n])
        assert [k for name, k in got[n] if name in PNG_STEPS] == [1] * len(PNG_STEPS), got[n]
        assert got[n][-1] == ("k_png_expand", 1) and len({name for name, _ in got[n]}) == len(got[n]), got[n]
    # no kernel of the eight runs once per image (the batch of the project's own streams)
    assert max(k for _, k in got[8]) <= 3, got[8]


def test_kernel_names_of_one_image_and_of_eight_are_the_same_list(z, gpu):
    """For batches of 1 and of 8 images the kernel names that zes_last_kernel_times reports are the same list, and the list
    contains k_png_expand exactly once.  The pixel forms have the block-parallel tier follow a single stream's chain with
    k_inf_chain, as it follows a batch's (the decode forms let the host follow a single chain).  The files carry streams of
    the project's own encoder: which tiers other encoders' streams reach is decided stream by stream."""
    cs = eight()
    own = own_streams(z, cs)
    one, all8 = launches(z, gpu, own[3:4]), launches(z, gpu, own)
    print(one)
    print(all8)
    assert [name for name, _ in one].count("k_png_expand") == 1 and [name for name, _ in all8].count("k_png_expand") == 1
    assert [name for name, _ in one] == [name for name, _ in all8]


def test_pools_hold_the_scanlines_and_trim_gives_them_back(z, gpu):
    cs = [c for c in X.cases() if c.height == 65][:12]
    flat, ioff, ilen = X.pack([c.blob for c in cs])
    t = dev(flat, gpu)
    z.trim()
    assert z.pool_bytes() == 0
    z.png_decode_tensor(t, ioff, ilen)
    plain = z.pool_bytes()
    z.trim()
    assert z.pool_bytes() == 0
    _, _, _, status, info = z.png_pixels_tensor(t, ioff, ilen)
    assert status == [0] * len(cs)
    assert z.pool_bytes() >= plain + sum(int(r["out_size"]) for r in info)  # the scanlines' scratch is a pool
    z.trim()
    assert z.pool_bytes() == 0
    run_dev(z, gpu, rows_of(cs))  # and the call after a trim is whole
