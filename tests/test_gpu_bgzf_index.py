"""The BGZF member index on the MI355X: the parallel finder (k_bgzf_mark) and the serial walk (ZES_F_INDEX_WALK) against
the host form and against tests/_bgzf.py's walk."""
import ctypes as C
import struct

import numpy as np
import pytest

import _bgzf
import _bgzf_index_cases as cases

pytestmark = pytest.mark.gpu

T = 16384  # ZES_BGZF_MARK_TILE of zlib.es_amd/csrc/zes_kernels.h: the bytes a workgroup of k_bgzf_mark covers


def place(gpu, blob, off=0, tail=0):
    """The blob at byte `off` of a tensor whose other bytes are 0x1f (a signature's first byte) -> tensor."""
    import torch

    a = np.full(off + len(blob) + tail + 16, 0x1F, dtype=np.uint8)
    a[off:off + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    t = torch.from_numpy(a).to(gpu)
    assert t.data_ptr() % 16 == 0
    return t


def dev_index(z, t, off, c, flags=0, cap=None):
    return cases.c_index(z.lib().zes_bgzf_index_dev, t.data_ptr() + off, c, flags, cap)


def check(z, gpu, blob, off=0):
    """Device index == host index == the walk's, by the finder and by the serial walk."""
    coff, uoff = cases.expected(blob)
    hc, hu = z.bgzf_index(blob)
    assert (hc == coff).all() and (hu == uoff).all()
    t = place(gpu, blob, off)
    for flags in (0, z.ZES_F_INDEX_WALK):
        rc, members, gc, gu = dev_index(z, t, off, len(blob), flags)
        assert rc == 0 and members == coff.size - 1, (flags, rc, members)
        assert (gc == coff).all() and (gu == uoff).all(), flags
    if off == 0:
        pc, pu = z.bgzf_index_tensor(t[:len(blob)])
        assert (pc == coff).all() and (pu == uoff).all()


@pytest.fixture(scope="module")
def files():
    out = cases.files()
    out["bare_signature"] = cases.bare_signature_file()
    return out


def test_kernel_choice(z, gpu, files):
    blob = files["ragged"][0]
    t = place(gpu, blob)
    z.set_profiling(True)
    try:
        assert dev_index(z, t, 0, len(blob), 0, cap=64)[0] == 0
        first = [k[0] for k in z.last_kernel_times()]
        assert dev_index(z, t, 0, len(blob), z.ZES_F_INDEX_WALK, cap=64)[0] == 0
        second = [k[0] for k in z.last_kernel_times()]
    finally:
        z.set_profiling(False)
    assert "k_bgzf_mark" in first and "k_gz_walk" not in first
    assert "k_gz_walk" in second and "k_bgzf_mark" not in second


def test_every_file(z, gpu, files):
    for name, (blob, _) in files.items():
        check(z, gpu, blob)


@pytest.mark.parametrize("off", [0, 1, 3, 15])
def test_alignment(z, gpu, files, off):
    check(z, gpu, files["ragged"][0], off)


def seam_file(start):
    """A file whose second member starts at byte `start`: the first one carries a dummy subfield and a stored payload of the
    length that takes."""
    extra = b"XY" + struct.pack("<H", 7) + b"padding"
    payload = cases.text(start - (12 + len(extra) + 6 + 5 + 8), 30)
    m0 = _bgzf.member(payload, _bgzf.raw_body(payload, 0), extra_before=extra)
    assert len(m0) == start
    return m0 + _bgzf.bgzf([cases.text(700, 31), cases.text(70, 32)])


@pytest.mark.parametrize("off", [0, 5])
def test_tile_seams(z, gpu, off):
    # the signature of the second member split 3|1, 2|2, 1|3 across the end of the first tile, and whole on either side of it;
    # with the file at byte 5 of its tensor the tiles' ends lie at file positions T - 5, 2T - 5, ...
    for d in (-3, -2, -1, 0, 1):
        for start in {T + d, T - off + d}:
            blob = seam_file(start)
            assert _bgzf.walk(blob)[1][0] == start
            check(z, gpu, blob, off)


def test_bounded_by_c(z, gpu, files):
    blob = files["ragged"][0]
    last = _bgzf.walk(blob)[-1][0]
    t = place(gpu, blob, 0)
    for off, tt in ((0, t), (3, place(gpu, blob, 3))):
        for c in (last + 5, last + 17, len(blob) - 3, len(blob) - 8):  # inside the last member's header, inside its trailer
            a = np.frombuffer(blob[:c], dtype=np.uint8)
            assert cases.c_index(z.lib().zes_bgzf_index, a.ctypes.data, c)[0] == z.ZES_E_GZIP
            for flags in (0, z.ZES_F_INDEX_WALK):
                assert dev_index(z, tt, off, c, flags)[0] == z.ZES_E_GZIP, (off, c, flags)
        # (the whole file behind the same pointer is fine)
        assert dev_index(z, tt, off, len(blob))[0] == 0


def test_overflow_goes_to_the_walk(z, gpu):
    blob = _bgzf.bgzf([]) * 1300
    assert len(blob) == 36400 and len(blob) // 256 + 1024 == 1166
    check(z, gpu, blob)
    t = place(gpu, blob)
    z.set_profiling(True)
    try:
        rc, members, _, _ = dev_index(z, t, 0, len(blob), 0, cap=1301)
        names = [k[0] for k in z.last_kernel_times()]
    finally:
        z.set_profiling(False)
    assert rc == 0 and members == 1300
    assert "k_bgzf_mark" in names and "k_gz_walk" in names and names.index("k_bgzf_mark") < names.index("k_gz_walk")


def test_statuses_match_the_host_form(z, gpu, files):
    chunks = cases.damage_chunks()
    for kind in cases.GZIP_KINDS + cases.OK_KINDS:
        blob, _ = _bgzf.damage(chunks, kind)
        a = np.frombuffer(blob, dtype=np.uint8)
        want = cases.c_index(z.lib().zes_bgzf_index, a.ctypes.data, a.size)
        assert want[0] == (z.ZES_E_GZIP if kind in cases.GZIP_KINDS else 0), kind
        t = place(gpu, blob, 3)
        for flags in (0, z.ZES_F_INDEX_WALK):
            got = dev_index(z, t, 3, len(blob), flags)
            assert got[0] == want[0], (kind, flags)
            if want[0] == 0:
                assert got[1] == want[1] and (got[2] == want[2]).all() and (got[3] == want[3]).all(), (kind, flags)
    blob = files["ragged"][0]
    t = place(gpu, blob)
    want = len(_bgzf.walk(blob))
    m = C.c_uint64()
    for flags in (0, z.ZES_F_INDEX_WALK):
        assert z.lib().zes_bgzf_index_dev(t.data_ptr(), len(blob), None, None, 0, C.byref(m), flags) == z.ZES_E_NOSPACE and m.value == want
        rc, members, coff, uoff = dev_index(z, t, 0, len(blob), flags, cap=want)
        assert rc == z.ZES_E_NOSPACE and members == want and (coff == 0xA5A5A5A5A5A5A5A5).all() and (uoff == 0xA5A5A5A5A5A5A5A5).all()
    with pytest.raises(z.ZlibEsError) as ei:
        z.bgzf_index_tensor(place(gpu, _bgzf.damage(chunks, "garbage")[0])[:len(_bgzf.damage(chunks, "garbage")[0])])
    assert ei.value.code == z.ZES_E_GZIP
