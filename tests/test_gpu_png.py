"""The PNG reader on the MI355X (zes_png_decode_dev, zes_png_decode_alloc; k_png_walk, k_png_unfilter): the files of
tests/_png.py at the smallest shapes that matter — every (colour, depth) pair, widths and heights on either side of a band of
64 rows, every filter unit and row alignment, chains of one filter type across two band seams, restart rows on and beside the
seams, IDAT runs cut in every way, files and outputs at every alignment — and every kind of damage between good neighbours.
Expected bytes are the writer's inputs.  The device form writes into a tensor filled with 0xA5, so every byte outside the
images' ranges is checked; each test uses the alloc form as well."""
import io
import zlib

import numpy as np
import pytest

import _png
import _png_poison  # noqa: F401  (adds the PNG entries to the poison catalogue, tests/_poison_cases.py)

pytestmark = pytest.mark.gpu

NOSPACE = _png.ZES_E_NOSPACE


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


def dev(flat, gpu):
    import torch

    return torch.from_numpy(flat).to(gpu)


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


def run_dev(z, gpu, cases, at=0, residue=None, flags=0):
    """zes_png_decode_dev into a tensor filled with 0xA5: every status, length and byte checked.  Returns the statuses."""
    import torch

    flat, ioff, ilen = pack([c.blob for c in cases], at)
    t = dev(flat, gpu)
    sizes = [len(c.want) if c.want is not None else 0 for c in cases]
    off, room = places(sizes, residue)
    cap = [n - 1 if c.short else n for n, c in zip(sizes, cases)]
    out = torch.full((room,), 0xA5, dtype=torch.uint8, device=gpu)
    got, off2, out_len, status, info = z.png_decode_tensor(t, ioff, ilen, out=out, off=off, flags=flags, cap=cap)
    host = got.cpu().numpy()
    untouched = np.ones(host.size, dtype=bool)
    for i, c in enumerate(cases):
        exp = NOSPACE if c.short else c.status
        assert status[i] == exp or (isinstance(exp, tuple) and status[i] in exp), (c.name, i, status[i], exp)
        assert out_len[i] == (sizes[i] if status[i] in (0, NOSPACE) else 0), (c.name, i, out_len[i])
        if not c.short:
            untouched[off[i]:off[i] + sizes[i]] = False
        if status[i] == 0:
            assert host[off[i]:off[i] + sizes[i]].tobytes() == c.want, (c.name, i)
            assert _png.info_dict(info[i]) == _png.info_rule(c.blob)[1], c.name
    assert (host[untouched] == 0xA5).all(), "a byte outside the images' ranges was written"
    return status


def run_host(z, cases, flags=0):
    """zes_png_decode_alloc through the package: every status and every byte checked."""
    res = z.png_decode_batch([c.blob for c in cases], flags)
    for c, r in zip(cases, res):
        if isinstance(r, Exception):
            assert r.code == c.status or (isinstance(c.status, tuple) and r.code in c.status), (c.name, r.code, c.status)
        else:
            assert c.status == 0, c.name
            info, rows = r
            assert rows.tobytes() == c.want and rows.shape == (int(info["height"]), int(info["rowbytes"])), c.name
            assert _png.info_dict(info) == _png.info_rule(c.blob)[1], c.name


def both(z, gpu, cases, **kw):
    st = run_dev(z, gpu, cases, **kw)
    run_host(z, cases, kw.get("flags", 0))
    return st


def image(name, colour, depth, w, h, filters, seed, **kw):
    raw = _png.pixels(_png.shape(w, h, colour, depth)[2], seed)
    return _png.Case(name, _png.write(w, h, colour, depth, raw, filters, **kw), raw)


def test_geometry_in_one_batch(z, gpu):
    g = _png.geometry()
    assert both(z, gpu, g, at=1) == [0] * len(g)
    run_dev(z, gpu, g, at=0, flags=z.ZES_F_PIECES)


def test_chains_of_one_filter_type_across_two_seams(z, gpu):
    cases = []
    for ft in range(5):
        cases.append(image("type %d, bpp 3" % ft, 2, 8, 33, 130, [ft] * 130, 200 + ft))
        cases.append(image("type %d, bpp 8" % ft, 6, 16, 9, 130, [ft] * 130, 210 + ft))
        cases.append(image("type %d, bpp 1" % ft, 0, 4, 37, 130, [ft] * 130, 220 + ft))
    both(z, gpu, cases)


def test_restart_rows_on_and_beside_the_seams(z, gpu):
    cases = []
    for tag, rows in (("on the seams", (64, 128)), ("beside the seams", (63, 65)), ("every band", (64, 128, 192))):
        for ft in (0, 1):
            f = [4] * 200
            for r in rows:
                f[r] = ft
            cases.append(image("%s, type %d" % (tag, ft), 6, 8, 19, 200, f, 300 + ft + len(cases)))
    f = [3] * 200
    f[64], f[128], f[192] = 0, 1, 0
    cases.append(image("average, every band a restart", 4, 8, 5, 200, f, 320))
    both(z, gpu, cases)


def test_idat_shapes_and_stream_makers(z, gpu):
    colour, depth, w, h = 2, 8, 65, 130
    f = _png.pattern(h, 7)
    reference = lambda filtered: z.deflate(np.frombuffer(filtered, dtype=np.uint8)).tobytes()
    makers = {"level 0": 0, "level 9": 9, "Z_FIXED": _png.fixed_stream, "the reference's stream": reference}
    plans = {"one chunk": None, "40 one-byte chunks": [1] * 40, "empty chunks between full ones": [0, 100, 0, 0, 50, 0],
             "cuts at every residue mod 16": [17] * 16}
    cases = [image("%s, %s" % (m, p), colour, depth, w, h, f, 400 + i, stream=makers[m], plan=plans[p])
             for i, (m, p) in enumerate((m, p) for m in makers for p in plans)]
    both(z, gpu, cases)
    cuts = {c[2] % 16 for c in _png.chunks_of(cases[3].blob) if c[1] == b"IDAT"}
    assert len(cuts) == 16
    # one image a call: the tier where the stream decides it, and the call's launches
    z.set_profiling(True)
    try:
        run_dev(z, gpu, [cases[12]])
        assert z.last_inflate_tier() == 1  # a reference-made stream: the block-parallel tier
        names = {name: n for name, _, n in z.last_kernel_times()}
        assert names.get("k_png_walk") == 1 and names.get("k_png_unfilter") == 1 and names.get("k_crc32_seg") == 1 and names.get("k_adler_seg") == 1, names
        run_dev(z, gpu, [cases[5]])
        assert z.last_inflate_tier() in (2, 3, 4)
        names = {name: n for name, _, n in z.last_kernel_times()}
        assert names.get("k_png_walk") == 2 and names.get("k_png_unfilter") == 1, names  # 43 chunks: more than the first walk's share
        # the sizing pass costs the walk alone
        import torch

        flat, ioff, ilen = pack([c.blob for c in cases[::4]])
        _, _, out_len, status, _ = z.png_decode_tensor(dev(flat, gpu), ioff, ilen, out=torch.zeros(16, dtype=torch.uint8, device=gpu), off=[0] * 4, cap=[0] * 4)
        assert status == [NOSPACE] * 4 and out_len == [len(c.want) for c in cases[::4]]
        assert {name: n for name, _, n in z.last_kernel_times()} == {"k_png_walk": 1}
        # nothing to decode: no launch
        assert z.png_decode_tensor(dev(flat, gpu), [], [])[2:4] == ([], [])
        assert z.last_kernel_times() == [] and z.last_inflate_tier() == 0
    finally:
        z.set_profiling(False)


def test_placement_of_files_and_outputs(z, gpu):
    g = _png.geometry()[3:35:2]
    assert len(g) == 16
    for at in (0, 1, 7):
        run_dev(z, gpu, g, at=at, residue=lambda i: (i + at) % 16)
    run_host(z, g)


def test_damage_between_good_neighbours(z, gpu):
    a, b = _png.neighbours()
    cases = [a]
    for c in _png.damage():
        cases += [c, b if len(cases) % 4 == 1 else a]
    st = run_dev(z, gpu, cases, at=3)
    assert st.count(0) == len(_png.damage()) + 1 and st.count(NOSPACE) == 1
    run_host(z, [c for c in cases if not c.short])
    # a batch in which every image fails, and a single damaged image
    bad = [c for c in _png.damage() if not c.short]
    both(z, gpu, bad)
    for c in bad:
        run_dev(z, gpu, [c])


def test_walk_equals_the_host_rule(z, gpu):
    import torch

    cases = _png.everything()
    flat, ioff, ilen = pack([c.blob for c in cases], at=5)
    zero = [0] * len(cases)
    _, _, out_len, status, info = z.png_decode_tensor(dev(flat, gpu), ioff, ilen, out=torch.zeros(16, dtype=torch.uint8, device=gpu), off=zero, cap=zero)
    for i, c in enumerate(cases):
        try:
            want, st = z.png_info(c.blob), 0
        except z.ZlibEsError as e:
            want, st = np.zeros(1, dtype=z.PNG_INFO)[0], e.code
        assert info[i].tobytes() == want.tobytes(), c.name
        if st:
            assert (status[i], out_len[i]) == (st, 0), c.name
        elif int(want["interlace"]):
            assert (status[i], out_len[i]) == (_png.ZES_E_UNSUPPORTED, 0), c.name
        else:
            assert (status[i], out_len[i]) == (NOSPACE, int(want["out_size"])), c.name


def test_files_of_a_real_encoder(z, gpu):
    Image = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(9)
    cases = []
    for mode, ch, (w, h) in (("L", 1, (200, 150)), ("RGB", 3, (131, 129)), ("RGBA", 4, (96, 200)), ("RGB", 3, (64, 64))):
        yy, xx = np.mgrid[0:h, 0:w]
        a = ((xx * 2 + yy * 3)[:, :, None] + np.arange(ch) * 40 + rs.randint(0, 6, size=(h, w, ch))).astype(np.uint8)
        im = Image.fromarray(a[:, :, 0] if ch == 1 else a, mode)
        buf = io.BytesIO()
        im.save(buf, "PNG")
        cases.append(_png.Case("PIL %s %dx%d" % (mode, w, h), buf.getvalue(), im.tobytes()))
    both(z, gpu, cases, at=1)
    # libpng chose the filters: more than one type is in use
    filtered = zlib.decompress(b"".join(cases[1].blob[d:d + n] for _, t, d, n in _png.chunks_of(cases[1].blob) if t == b"IDAT"))
    assert len({filtered[r * (1 + 131 * 3)] for r in range(129)}) >= 2
