"""zes_adler32_batch_dev (k_adler_seg): the Adler-32 of many segments of one arena, at any alignment, in one launch.
Expected values are CPython's zlib.adler32 of the same bytes; the case list is tests/_adler_cases.py."""
import ctypes as C
import zlib as pz

import numpy as np
import pytest

import _adler_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(z):
    return cases.arena(lambda n: z.gen("xorshift", 77, n))


@pytest.fixture(scope="module")
def arena(host, gpu):
    import torch

    t = torch.from_numpy(host).to(gpu)
    assert t.data_ptr() % 16 == 0  # (the case list's alignments are offsets into the arena)
    return t


def run(z, arena, host, segs):
    got = z.adler32_batch_tensor(arena, [o for _, o, _ in segs], [n for _, _, n in segs])
    assert len(got) == len(segs)
    for (label, o, n), g in zip(segs, got):
        assert g == pz.adler32(host[o:o + n].tobytes()), (label, hex(g))
    return got


def test_alignment_and_length_grid(z, arena, host):
    """Every content x alignment x length in one call; one launch."""
    segs = cases.grid()
    z.set_profiling(True)
    try:
        run(z, arena, host, segs)
        launches = {k: n for k, ms, n in z.last_kernel_times()}
    finally:
        z.set_profiling(False)
    assert launches == {"k_adler_seg": 1}, launches


def test_overlapping_identical_and_last_byte(z, arena, host):
    got = run(z, arena, host, cases.overlapping())
    assert got[0] == got[1]


def test_3000_short_segments(z, arena, host):
    run(z, arena, host, cases.many_short())


def test_agrees_with_the_single_call(z, arena, host):
    segs = [s for s in cases.grid() if s[0].startswith("xorshift") and s[2]] + cases.overlapping()
    got = run(z, arena, host, segs)
    for (label, o, n), g in zip(segs, got):
        assert g == z.adler32_tensor(arena[o:o + n]), label


def test_empty_and_error_cases(z, arena, host):
    L = z.lib()
    assert z.adler32_batch_tensor(arena, [], []) == []
    assert L.zes_adler32_batch_dev(None, None, None, None, 0) == 0  # count == 0: nothing is looked at
    z.set_profiling(True)
    try:
        assert z.adler32_batch_tensor(arena, [0, 5, cases.ARENA], [0, 0, 0]) == [1, 1, 1]
        assert z.last_kernel_times() == []  # only empty segments: no launch
    finally:
        z.set_profiling(False)
    one, out = (C.c_uint64 * 1)(16), (C.c_uint32 * 1)()
    assert L.zes_adler32_batch_dev(arena.data_ptr(), None, one, out, 1) == -18
    assert L.zes_adler32_batch_dev(arena.data_ptr(), one, None, out, 1) == -18
    assert L.zes_adler32_batch_dev(arena.data_ptr(), one, one, None, 1) == -18
    assert L.zes_adler32_batch_dev(None, one, one, out, 1) == -18  # a null d_in with a non-zero length
    zero = (C.c_uint64 * 1)(0)
    assert L.zes_adler32_batch_dev(None, zero, zero, out, 1) == 0 and out[0] == 1
