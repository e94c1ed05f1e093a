"""The PNG writer on the GPU: every file byte for byte against tests/_pngwrite.py's model (numpy filters, the CPU oracle's
stream, _png.chunk), read back by zes_png_decode* and by PIL, through both forms.  The device form writes into a tensor filled
with 0xA5 and every byte outside the files is checked."""
import io
import json
import os

import numpy as np
import pytest

import _png
import _pngwrite as W
import _pngwrite_poison  # noqa: F401  (registers the writer's catalogue entries)
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MINE = ("k_png_filter", "k_png_pack", "k_crc32_seg", "k_crc32_put", "k_adler_seg")
PIL_MODES = {(0, 1): "1", (0, 8): "L", (0, 16): "I;16", (2, 8): "RGB", (3, 1): "P", (3, 2): "P", (3, 4): "P", (3, 8): "P", (4, 8): "LA", (6, 8): "RGBA"}


def read_back(z, ims, blobs):
    """zes_png_decode_alloc gives every image's scanlines back; PIL opens and loads every file and, where it keeps the samples
    as they are (8 bits a sample, no tRNS), gives the same bytes."""
    got = z.png_decode_batch(blobs)
    for im, blob, g in zip(ims, blobs, got):
        assert not isinstance(g, Exception), (im.name, g)
        info, rows = g
        assert rows.tobytes() == im.raw, im.name
        assert (int(info["width"]), int(info["height"]), int(info["colour"]), int(info["depth"])) == (im.width, im.height, im.colour, im.depth)
        assert int(info["plte_len"]) == len(im.plte) and int(info["trns_len"]) == len(im.trns), im.name
        assert int(info["idat_count"]) == len(W.idats(blob)), im.name
    Image = pytest.importorskip("PIL.Image")
    for im, blob in zip(ims, blobs):
        with Image.open(io.BytesIO(blob)) as p:
            p.load()
            assert p.size == (im.width, im.height), im.name
            if im.depth == 8 and not im.trns and im.colour != 3:
                assert p.mode == PIL_MODES[(im.colour, im.depth)] and p.tobytes() == im.raw, im.name


def both_forms(z, gpu, oracle, ims, flags=0, **kw):
    """The batch through both forms, every file compared, every byte outside the files checked -> the files."""
    want = [W.expect(im, oracle)[0] for im in ims]
    host, off, out_len, status = W.run_dev(z, gpu, ims, flags, **kw)
    W.check_dev(host, off, out_len, status, want)
    assert W.run_host(z, ims, flags) == want
    return want


def test_geometry_every_pair_size_and_filter_value(z, gpu, oracle):
    ims = W.geometry()
    f = W.geometry_facts()
    assert f["pairs"] == set(_png.PAIRS) and f["widths"] == {1, 2, 3, 5, 17, 63, 64, 65, 300} and f["heights"] == {1, 2, 63, 64, 65, 129}
    assert f["filters"] == set(range(7)) and f["bpp"] == {1, 2, 3, 4, 6, 8}
    want = both_forms(z, gpu, oracle, ims)
    read_back(z, ims, want)
    # the same batch in groups of four: the same bytes
    assert len(W.groups(ims, W.PIECES)) >= len(ims) // 4 and W.groups(ims) == [len(ims)]
    assert both_forms(z, gpu, oracle, ims, W.PIECES) == want


def test_adaptive_choice(z, gpu, oracle):
    ims = [W.each_wins(5), W.each_wins(6), W.zeros(6), W.zeros(5), W.rgba16(6), W.rgba16(5), W.grey4(5), W.grey4(6)]
    want = both_forms(z, gpu, oracle, ims)
    read_back(z, ims, want)
    for im, blob in zip(ims, want):  # the filter bytes in the files are the model's choice (the conditions: test_pngwrite_cpu.py)
        import zlib

        f = zlib.decompress(b"".join(blob[d:d + n] for _, t, d, n in _png.chunks_of(blob) if t == b"IDAT"))
        assert list(f[::1 + im.rowbytes]) == W.choose(im), im.name


def test_stream_routes(z, gpu, oracle):
    rnd, low = W.random_rgba(), W.lowent_rgba()
    ims = [rnd, low]
    want = both_forms(z, gpu, oracle, ims)
    assert W.expect(rnd, oracle)[1] == "stored" and W.idats(want[0]) == [65536, W.stored_len(rnd.F) - 65536] and rnd.F > 65535
    assert W.expect(low, oracle)[1] == "stream" and len(W.idats(want[1])) >= 3 and set(W.idats(want[1])[:-1]) == {65536}
    read_back(z, ims, want)


def test_lengths_the_encoder_refuses(z, gpu, oracle):
    ims = W.refused()
    assert [im.F for im in ims] == [131073, 131073]
    z.set_profiling(True)
    try:
        want = both_forms(z, gpu, oracle, ims)
        n = {name: k for name, _, k in z.last_kernel_times()}
        assert n.get("k_adler_seg") == 1 and n.get("k_png_filter") == 1 and n.get("k_png_pack") == 1, n
        assert not set(n) - set(MINE), n  # no encoder launch: the group has no slot
        both = ims + W.nine()[:2]
        both_forms(z, gpu, oracle, both)
        assert {name: k for name, _, k in z.last_kernel_times()}.get("k_adler_seg") == 1
        both_forms(z, gpu, oracle, W.nine()[:2])
        assert "k_adler_seg" not in {name for name, _, _ in z.last_kernel_times()}
    finally:
        z.set_profiling(False)
    for blob in want:
        assert W.idats(blob) == [65536, 65536, 131073 + 2 + 15 + 4 - 131072]
    read_back(z, ims, want)


def test_placement_every_residue(z, gpu, oracle):
    ims = [W.Img("place %d" % k, 9 + k, 5 + k % 3, 2, 8, 5, W.smooth((9 + k) * 3, 5 + k % 3, 70 + k)) for k in range(16)]
    want = [W.expect(im, oracle)[0] for im in ims]
    for first in (0, 1, 7):
        out_off, at = [], first
        for k, w in enumerate(want):
            at += (k + first - at) % 16  # file k at residue k + first mod 16 (file 0: the offset itself)
            out_off.append(at)
            at += len(w)
        host, off, out_len, status = W.run_dev(z, gpu, ims, in_shift=[(k + first) % 16 for k in range(16)], out_off=out_off, cap=[len(w) for w in want])
        assert sorted(o % 16 for o in off) == list(range(16)) and off[0] == first
        W.check_dev(host, off, out_len, status, want)


def test_nospace(z, gpu, oracle):
    ims = W.nine()[:3]
    want = [W.expect(im, oracle)[0] for im in ims]
    caps = [len(want[0]), len(want[1]) - 1, len(want[2])]
    host, off, out_len, status = W.run_dev(z, gpu, ims, cap=caps)
    assert status == [0, _png.ZES_E_NOSPACE, 0] and out_len[1] == len(want[1])
    W.check_dev(host, off, out_len, status, [want[0], None, want[2]])
    host, off, out_len, status = W.run_dev(z, gpu, ims, cap=[0, 0, 0])
    assert status == [_png.ZES_E_NOSPACE] * 3 and out_len == [len(w) for w in want] and (host == 0xA5).all()
    _, _, out_len, status = W.run_dev(z, gpu, ims, null_out=True)
    assert status == [_png.ZES_E_NOSPACE] * 3 and out_len == [len(w) for w in want]


def test_bad_records_between_good_neighbours(z, gpu, oracle):
    import torch

    a, b = W.nine()[0], W.nine()[1]
    wa, wb = W.expect(a, oracle)[0], W.expect(b, oracle)[0]
    bad = W.bad_records()
    flat = torch.from_numpy(np.frombuffer(a.raw + b.raw, dtype=np.uint8).copy()).to(gpu)
    recs = [a.record()]
    in_off, in_len, out_off, cap = [0], [len(a.raw)], [0], [len(wa)]
    for r, n, _ in bad:
        recs += [r, b.record()]
        in_off += [0, len(a.raw)]
        in_len += [n, len(b.raw)]
        out_off += [out_off[-1] + cap[-1] + 3, out_off[-1] + cap[-1] + 3]
        cap += [0, len(wb)]
    aux = bytes(sum(r[6] + r[7] for r in recs))
    out = torch.full((out_off[-1] + cap[-1] + 16,), 0xA5, dtype=torch.uint8, device=gpu)
    rec = W.records(z, recs)
    # (the package's wrapper checks ranges for images the bound accepts only)
    _, off, out_len, status = z.png_encode_tensor(flat, in_off, in_len, rec, aux, out=out, off=out_off, cap=cap)
    want_status = [0] + [s for _, _, st in bad for s in (st, 0)]
    assert status == want_status
    W.check_dev(out.cpu().numpy(), [int(o) for o in off], out_len, status, [wa] + [w for _ in bad for w in (None, wb)])
    assert all(n == 0 for n, s in zip(out_len, status) if s != 0)
    # every image fails: nothing is launched
    z.set_profiling(True)
    try:
        only = W.records(z, [r for r, _, _ in bad])
        _, _, out_len, status = z.png_encode_tensor(flat, [0] * len(bad), [n for _, n, _ in bad], only, bytes(64), out=out, off=[0] * len(bad), cap=[0] * len(bad))
        assert status == [st for _, _, st in bad] and out_len == [0] * len(bad) and z.last_kernel_times() == []
    finally:
        z.set_profiling(False)


def launches(z, gpu, oracle, ims, flags):
    z.set_profiling(True)
    try:
        host, off, out_len, status = W.run_dev(z, gpu, ims, flags)
        n = {name: k for name, _, k in z.last_kernel_times()}
    finally:
        z.set_profiling(False)
    W.check_dev(host, off, out_len, status, [W.expect(im, oracle)[0] for im in ims])
    return {"launches": {k: n[k] for k in sorted(n) if k in MINE}, "others": {k: n[k] for k in sorted(n) if k not in MINE}}


def test_launches_per_group(z, gpu, oracle):
    """What include/zes.h and DESIGN.md state: per group one k_png_filter, one batch encode, one k_png_pack, one k_crc32_seg
    and one k_crc32_put; nothing grows with the images of a group.  Recorded in tests/golden/pngwrite_launches.json."""
    nine = W.nine()
    got = {"one image": launches(z, gpu, oracle, nine[:1], 0), "nine images": launches(z, gpu, oracle, nine, 0),
           "nine images in groups of four": launches(z, gpu, oracle, nine, W.PIECES)}
    for name, groups in (("one image", 1), ("nine images", 1), ("nine images in groups of four", 3)):
        assert got[name]["launches"] == {"k_png_filter": groups, "k_png_pack": groups, "k_crc32_seg": groups, "k_crc32_put": groups}, (name, got[name])
        assert got[name]["others"], name  # the encoder ran
    assert got["one image"]["others"] == got["nine images"]["others"]  # no count grows with the images of a group
    assert sorted(got["nine images in groups of four"]["others"]) == sorted(got["nine images"]["others"])
    with open(os.path.join(GOLDEN, "pngwrite_launches.json")) as f:
        assert got == json.load(f)
