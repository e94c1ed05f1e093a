"""The BGZF writer without a GPU: the two sizing entry points, the expected-file builder the GPU tests compare against,
and that zes_bgzip refuses to compute without a device."""
import ctypes as C
import gzip as pygzip

import numpy as np
import pytest

import _bgzf
import _bgzip_expect as E

SIZES = (0, 1, 2, 65279, 65280, 65281, 2 * 65280, (1 << 32) + 5)


def test_members_and_bound_answer_without_a_device(z):
    L = z.lib()
    v = C.c_uint64()
    for n in SIZES:
        assert L.zes_bgzip_members(n, C.byref(v)) == 0 and v.value == -(-n // 65280) + 1 == E.members(n), n
        tail = n % 65280
        want = n // 65280 * 65311 + (tail + 31 if tail else 0) + 28
        assert L.zes_bgzip_bound(n, C.byref(v)) == 0 and v.value == want == E.bound(n), n
        assert z.bgzip_members(n) == E.members(n) and z.bgzip_bound(n) == want
    assert L.zes_bgzip_members(5, None) == z.ZES_E_ARG
    assert L.zes_bgzip_bound(5, None) == z.ZES_E_ARG


def test_bad_arguments_are_decided_before_the_device(z):
    L = z.lib()
    a = np.zeros(64, dtype=np.uint8)
    out = np.zeros(256, dtype=np.uint8)
    n = C.c_uint64()
    for fn in (L.zes_bgzip, L.zes_bgzip_dev):
        assert fn(a.ctypes.data, 64, out.ctypes.data, out.size, None, None, 0) == z.ZES_E_ARG
        assert fn(None, 64, out.ctypes.data, out.size, C.byref(n), None, 0) == z.ZES_E_ARG
        assert fn(a.ctypes.data, 64, None, out.size, C.byref(n), None, 0) == z.ZES_E_ARG
        for flags in (1, 2, 8, 32, 1 << 31):
            assert fn(a.ctypes.data, 64, out.ctypes.data, out.size, C.byref(n), None, flags) == z.ZES_E_ARG


def test_the_empty_input_is_the_marker_alone(z):
    got, off = z.bgzip(b"", index=True)
    assert got.tobytes() == E.EOF_MARKER == E.expect(b"") and off == [0]
    out = np.zeros(28, dtype=np.uint8)
    n = C.c_uint64()
    assert z.lib().zes_bgzip(None, 0, out.ctypes.data, 27, C.byref(n), None, 0) == z.ZES_E_NOSPACE and n.value == 28
    assert not out.any()


@pytest.mark.parametrize("kind", ["xorshift", "itext", "lowent4k"])
def test_expect_is_a_gzip_file_of_its_input(z, oracle, kind):
    for n in (0, 1, 2, 24, 32, 65281):
        x = z.gen(kind, 11, n).tobytes()
        blob = E.expect(x)
        assert pygzip.decompress(blob) == x
        ms = _bgzf.walk(blob)
        assert len(ms) == E.members(n)
        assert all(size <= 65311 and hlen == 18 for _, size, hlen in ms)
        assert blob.endswith(E.EOF_MARKER)


def test_expect_on_incompressible_data_meets_the_bound(z, oracle):
    n = 2 * 65280 + 1
    x = z.gen("xorshift", 12, n).tobytes()
    blob = E.expect(x)
    assert [size for _, size, _ in _bgzf.walk(blob)] == [65311, 65311, 32, 28]
    assert len(blob) == z.bgzip_bound(n)
    assert pygzip.decompress(blob) == x
    assert E.plan(x)[2] == [True, True, True]


def test_expect_reaches_both_body_rules_with_small_inputs(z, oracle):
    text = z.gen("itext", 13, 65280).tobytes()
    for n in (2, 24):
        assert E.body_of(text[:n])[1], n
    for n in (32, 4096, 65280):
        assert not E.body_of(text[:n])[1], n
    assert E.body_of(b"x") == (b"\x01\x01\x00\xfe\xffx", True)


def test_no_cpu_fallback_without_gpu(z):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    a = np.arange(100, dtype=np.uint8)
    out = np.zeros(z.bgzip_bound(a.size), dtype=np.uint8)
    n = C.c_uint64()
    assert z.lib().zes_bgzip(a.ctypes.data, a.size, out.ctypes.data, out.size, C.byref(n), None, 0) == z.ZES_E_DEVICE
    with pytest.raises(z.ZlibEsError) as ei:
        z.bgzip(a)
    assert ei.value.code == z.ZES_E_DEVICE
