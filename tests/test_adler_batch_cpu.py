"""The segmented Adler-32 kernel's cut rule and closed form (tests/_adler_cases.py), checked against CPython's
zlib.adler32 on the case list the GPU test runs; and the Python side of the feature: the wrapper and the flag."""
import zlib as pz

import numpy as np
import pytest

import _adler_cases as cases


@pytest.fixture(scope="module")
def arena(z):
    return cases.arena(lambda n: z.gen("xorshift", 77, n))


def test_chunks_are_cut_at_64k_steps_from_the_aligned_start():
    assert cases.chunks(4096, 0) == []
    assert cases.chunks(4096, 65536) == [(0, 65536)]
    assert cases.chunks(4096 + 1, 65536) == [(0, 65535), (65535, 65536)]
    assert cases.chunks(4096 + 15, 1) == [(0, 1)]
    assert cases.chunks(4096 + 15, 2) == [(0, 2)]  # two groups, one chunk
    assert cases.chunks(4096 + 7, 131072 - 7) == [(0, 65529), (65529, 131065)]
    assert cases.chunks(4096 + 7, 131072 - 6) == [(0, 65529), (65529, 131065), (131065, 131066)]
    for addr, n in ((4096 + 9, 200000), (16, 1), (31, 300000)):
        c = cases.chunks(addr, n)
        assert c[0][0] == 0 and c[-1][1] == n and all(a[1] == b[0] for a, b in zip(c, c[1:]))
        assert all((addr + s) % 16 == 0 for s, _ in c[1:]) and all(e - s <= cases.CHUNK for s, e in c)


def test_restatement_matches_zlib_on_the_grid(arena):
    checked = 0
    for label, off, n in cases.grid() + cases.overlapping() + cases.many_short(200):
        seg = arena[off:off + n]
        assert seg.size == n, label
        # (the arena of the GPU test starts on a 16-byte boundary: the offset stands for the address)
        assert cases.adler_by_chunks(seg, off) == pz.adler32(seg.tobytes()), label
        checked += 1
    assert checked > 300


def test_largest_sums():
    """64 KiB of 0xFF overflows 32 bits in B_c; 300000 bytes of 0xFF puts len - e above 65521 for the first chunks."""
    ff = np.full(300000, 0xFF, dtype=np.uint8)
    b = ff[:65536].astype(np.int64)
    assert int((b * np.arange(65536, 0, -1, dtype=np.int64)).sum()) > 1 << 32
    c = cases.chunks(7, 300000)
    assert 300000 - c[0][1] > cases.MOD
    assert cases.adler_by_chunks(ff, 7) == pz.adler32(ff.tobytes())


def test_wrapper_and_flag_exist(z):
    assert callable(z.adler32_batch_tensor)
    assert z.ZES_F_CHECK_ADLER == 16 and z.ZES_E_CHECKSUM == -21
    assert hasattr(z.lib(), "zes_adler32_batch_dev")
    assert "ZES_F_CHECK_ADLER" in z.inflate_batch.__doc__ and "ZES_F_CHECK_ADLER" in z.inflate_batch_tensor.__doc__
