"""The TIFF writer on the GPU: every case of tests/_tiffwrite.py's tables through the device form (zes_tiffwrite_dev: the input
at an odd device address, the file at d_out offsets 0, 1 and 3 inside a tensor of sentinel bytes, none of which may change
outside the file's range) and the host form (zes_tiffwrite), byte for byte against the restated layout around the CPU oracle's
streams; the written files through the project's own reader; the shapes where the cut kernel can go wrong; refused lengths;
groups; ZES_E_NOSPACE; the launch lists of a 4-tile and a 256-tile call; both routes in one image."""
import numpy as np
import pytest

import _tiff as T
import _tiffwrite as W
import _tiffwrite_poison  # noqa: F401  (the catalogue entries and COVERS / EXEMPT lines of the new entry points)

pytestmark = pytest.mark.gpu


def check_both_forms(z, gpu, oracle, case, offsets=(0, 1, 3), flags=0, lead=1):
    want, _ = W.expect(case, oracle)
    rec, off, ln, _ = T.rule(want)
    for at in offsets:
        got, goff, glen = W.run_dev(z, gpu, case, at=at, flags=flags, lead=lead)
        assert W.first_difference(got, want) is None, (case.name, at, W.first_difference(got, want))
        assert goff == off and glen == ln, (case.name, at)
    host = W.run_host(z, case, flags)
    assert W.first_difference(host, want) is None, (case.name, "host", W.first_difference(host, want))
    return want


def round_trip(z, gpu, case, f):
    """The written file through zes_tiff_index_dev and zes_tiff_read_dev: the input record and the input pixels."""
    t = W.on_device(np.frombuffer(f, dtype=np.uint8), gpu)
    idx = z.tiff_index_tensor(t)
    assert idx[0] == dict(case.record(), dirs=1), case.name
    pix, st, rc = z.tiff_read_tensor(t, idx)
    assert rc == 0 and not st.any() and (pix.cpu().numpy().reshape(-1) == case.raw()).all(), case.name


@pytest.mark.parametrize("layout", T.LAYOUTS, ids=lambda lay: "-".join(map(str, lay)))
@pytest.mark.parametrize("bits", (8, 16, 32))
def test_layouts_and_kinds(z, gpu, oracle, layout, bits):
    n = 0
    for case in W.grid(layouts=(layout,), depths=(bits,)):
        f = check_both_forms(z, gpu, oracle, case)
        if case.order == "MM" or case.compression == 8:
            round_trip(z, gpu, case, f)
        n += 1
    assert n == 3 * 2 * len(W.CODINGS)


def test_shapes_where_the_cut_can_go_wrong(z, gpu, oracle):
    for case in W.shapes():
        f = check_both_forms(z, gpu, oracle, case)
        round_trip(z, gpu, case, f)
    # the input at a 16-byte aligned device address, and at one that is 3 mod 4
    for lead in (0, 16, 3):
        for case in (W.shapes()[4], W.shapes()[5], W.six_tiles()):
            check_both_forms(z, gpu, oracle, case, offsets=(1,), lead=lead)


def test_signed_and_float_samples(z, gpu, oracle):
    for case in W.kinds():
        f = check_both_forms(z, gpu, oracle, case, offsets=(1,))
        got = z.tiff_read(f)
        assert got.dtype == case.px.dtype and (got.view(np.uint8) == case.px.view(np.uint8)).all(), case.name
        assert z.tiff_info(f) == dict(case.record(), dirs=1)


def test_lengths_the_encoder_refuses_go_stored(z, gpu, oracle):
    for case in W.refused():
        assert W.expect(case, oracle)[1] == ["refused"]
        z.set_profiling(True)
        try:
            f = check_both_forms(z, gpu, oracle, case, offsets=(1,))
            names = [name for name, _, _ in z.last_kernel_times()]
        finally:
            z.set_profiling(False)
        assert "k_adler_seg" in names and "k_tiff_cut" in names and "k_tiff_pack" in names, names
        round_trip(z, gpu, case, f)


def test_groups_give_the_same_bytes(z, gpu, oracle):
    six = W.six_tiles()
    assert W.groups(six.record(), W.PIECES) == [4, 2]
    plain = check_both_forms(z, gpu, oracle, six, offsets=(0,))
    pieces = check_both_forms(z, gpu, oracle, six, offsets=(3,), flags=W.PIECES)
    assert plain == pieces
    z.set_profiling(True)
    try:
        W.run_dev(z, gpu, six, flags=W.PIECES)
        counts = {name: k for name, _, k in z.last_kernel_times()}
    finally:
        z.set_profiling(False)
    assert counts["k_tiff_cut"] == 2 and counts["k_tiff_pack"] == 2, counts
    many = W.many_strips()
    assert W.groups(many.record()) == [1024, 1]
    f = check_both_forms(z, gpu, oracle, many, offsets=(1,))
    round_trip(z, gpu, many, f)


def test_nospace(z, gpu, oracle):
    import torch

    for case in (W.six_tiles(), W.mixed(), next(iter(W.grid(codings=((1, 1),))))):
        want, _ = W.expect(case, oracle)
        for cap in (len(want) - 1, 8, 0):
            with pytest.raises(z.ZlibEsError) as e:
                W.run_dev(z, gpu, case, at=1, cap=cap)
            assert e.value.code == T.E_NOSPACE and e.value.need == len(want), (case.name, cap)
        # cap one short: the size needed, and every byte behind cap intact
        room = torch.full((len(want) + 40,), W.SENTINEL, dtype=torch.uint8, device=gpu)
        with pytest.raises(z.ZlibEsError) as e:
            z.tiff_write_tensor(W.on_device(case.raw(), gpu), case.record(), out=room[3:3 + len(want) - 1])
        assert e.value.code == T.E_NOSPACE and e.value.need == len(want)
        host = room.cpu().numpy()
        assert (host[:3] == W.SENTINEL).all() and (host[3 + len(want) - 1:] == W.SENTINEL).all(), case.name
        # cap exactly the file's size is enough
        got, _, _ = W.run_dev(z, gpu, case, at=1, cap=len(want))
        assert got == want
    # cap == 0 with a null d_out is the sizing call
    import ctypes as C

    case = W.six_tiles()
    want, _ = W.expect(case, oracle)
    t = W.on_device(case.raw(), gpu)
    n = C.c_uint64()
    img = W.record_array(z, case.record())
    assert z.lib().zes_tiffwrite_dev(t.data_ptr(), t.numel(), img.ctypes.data, None, 0, C.byref(n), None, None, 0) == T.E_NOSPACE
    assert n.value == len(want)


def launches(z, gpu, oracle, case):
    z.set_profiling(True)
    try:
        got, _, _ = W.run_dev(z, gpu, case)
        assert got == W.expect(case, oracle)[0]
        return [(name, k) for name, _, k in z.last_kernel_times()]
    finally:
        z.set_profiling(False)


def test_kernel_names_of_4_tiles_and_of_256_are_the_same_list(z, gpu, oracle):
    names = {side: launches(z, gpu, oracle, W.rgba_tiles(side)) for side in (32, 256)}
    print(names)
    for side in (32, 256):
        assert [n for n, _ in names[side]].count("k_tiff_cut") == 1 and [n for n, _ in names[side]].count("k_tiff_pack") == 1
        assert dict(names[side])["k_tiff_cut"] == 1 and dict(names[side])["k_tiff_pack"] == 1
    assert [n for n, _ in names[32]] == [n for n, _ in names[256]]
    assert [k for _, k in names[32]] == [k for _, k in names[256]]  # and no kernel runs once per tile


def test_stream_and_stored_segments_in_one_image(z, gpu, oracle):
    case = W.mixed()
    routes = W.expect(case, oracle)[1]
    assert "stream" in routes and "stored" in routes
    f = check_both_forms(z, gpu, oracle, case)
    round_trip(z, gpu, case, f)
    check_both_forms(z, gpu, oracle, case, offsets=(1,), flags=W.PIECES)


def test_index_read_write_round_trips_a_foreign_file(z, gpu, oracle):
    """A file of the reader's own helper (CPython's zlib streams, segments at odd positions): its index record and its pixels
    written again give a file whose index is that record again and whose pixels are the same."""
    f, px = T.make(w=37, h=23, spp=4, bits=16, layout=("tiles", 32, 16), order="MM", compression=32946, predictor=2)
    info, _, _ = z.tiff_index(f)
    pix = z.tiff_read(f)
    rec = {k: info[k] for k in T.FIELDS}
    again = z.tiff_write(pix, rec)
    assert z.tiff_info(again) == info and (z.tiff_read(again) == px).all() and (T.decode(again) == px).all()
