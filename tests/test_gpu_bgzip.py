"""The BGZF writer on the MI355X (zes_bgzip, zes_bgzip_dev).  Expected bytes come from tests/_bgzip_expect.py, that is from
the CPU oracle and CPython, never from this library."""
import ctypes as C
import gzip as pygzip

import numpy as np
import pytest

import _bgzf
import _bgzip_expect as E

pytestmark = pytest.mark.gpu

KINDS = ("xorshift", "itext", "lowent4k")
SIZES = (0, 1, 2, 24, 32, 65279, 65280, 65281, 2 * 65280 + 1, 5 * 65280 + 12345)
CANARY = 64
_cache = {}


def data_of(z, kind, n, seed=21):
    key = (kind, n, seed)
    if key not in _cache:
        x = z.gen(kind, seed, n).tobytes()
        _cache[key] = (x, E.expect(x))
    return _cache[key]


def mixed(z, kinds, tail):
    """One full chunk per entry of `kinds`, then `tail` bytes of text -> (data, expected file)."""
    key = (tuple(kinds), tail)
    if key not in _cache:
        x = b"".join(z.gen(k, 30 + i, E.CHUNK).tobytes() for i, k in enumerate(kinds)) + z.gen("itext", 29, tail).tobytes()
        _cache[key] = (x, E.expect(x))
    return _cache[key]


def positions(blob):
    return [pos for pos, _, _ in _bgzf.walk(blob)]


def host_form(z, x, flags=0):
    """zes_bgzip -> (status, bytes, member_off)."""
    a = np.frombuffer(x, dtype=np.uint8)
    cap = z.bgzip_bound(len(x))
    out = np.full(cap + CANARY, 0xA5, dtype=np.uint8)
    off = (C.c_uint64 * z.bgzip_members(len(x)))()
    n = C.c_uint64()
    rc = z.lib().zes_bgzip(a.ctypes.data if len(x) else None, len(x), out.ctypes.data, cap, C.byref(n), off, flags)
    assert (out[n.value:] == 0xA5).all(), "the host form wrote behind its result"
    return rc, out[: n.value].tobytes(), list(off)


def dev_form(z, gpu, x, flags=0, in_at=3, out_at=5, cap=None):
    """zes_bgzip_dev with the input at byte in_at of its tensor and the output at byte out_at of a tensor that has CANARY
    bytes in front -> (status, out_len, bytes below cap, member_off).  Asserts that nothing outside
    [0, min(out_len, cap)) changed."""
    import torch

    t = torch.from_numpy(np.frombuffer(b"\x00" * in_at + x + b"\x00" * 16, dtype=np.uint8).copy()).to(gpu)
    cap = z.bgzip_bound(len(x)) if cap is None else cap
    buf = torch.full((CANARY + out_at + cap + CANARY + 16,), 0xA5, dtype=torch.uint8, device=gpu)
    assert t.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    at = CANARY + out_at
    off = (C.c_uint64 * z.bgzip_members(len(x)))()
    n = C.c_uint64()
    torch.cuda.synchronize()
    rc = z.lib().zes_bgzip_dev(t.data_ptr() + in_at, len(x), buf.data_ptr() + at, cap, C.byref(n), off, flags)
    h = buf.cpu().numpy()
    wrote = min(n.value, cap)
    assert (h[:at] == 0xA5).all(), "bytes in front of the result changed"
    assert (h[at + wrote:] == 0xA5).all() if rc == 0 else (h[at + cap:] == 0xA5).all(), "bytes behind the result changed"
    return rc, n.value, h[at: at + wrote].tobytes(), list(off)


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_bit_exact_with_the_expected_file(z, gpu, oracle, kind, n):
    x, want = data_of(z, kind, n)
    pos = positions(want)
    assert len(pos) == z.bgzip_members(n)
    rc, got, off = host_form(z, x)
    assert rc == 0 and got == want and off == pos
    rc, m, got, off = dev_form(z, gpu, x)
    assert rc == 0 and m == len(want) and got == want and off == pos


def test_python_forms(z, gpu, oracle):
    import torch

    x, want = data_of(z, "itext", 65281)
    got, off = z.bgzip(x, index=True)
    assert got.tobytes() == want and off == positions(want)
    assert z.bgzip(np.frombuffer(x, dtype=np.uint8)).tobytes() == want
    t = torch.from_numpy(np.frombuffer(b"\x00" + x, dtype=np.uint8).copy()).to(gpu)[1:]
    view, off = z.bgzip_tensor(t, index=True)
    assert view.cpu().numpy().tobytes() == want and off == positions(want)
    out = torch.zeros(z.bgzip_bound(len(x)) + 7, dtype=torch.uint8, device=gpu)[7:]
    assert z.bgzip_tensor(t, out=out).cpu().numpy().tobytes() == want
    with pytest.raises(z.ZlibEsError) as ei:
        z.bgzip_tensor(t, out=out[: len(want) - 1])
    assert ei.value.code == z.ZES_E_NOSPACE and ei.value.need == len(want)


# 2 ------------------------------------------------------------------------------------------------
def test_stored_and_stream_bodies_in_one_launch(z, gpu, oracle):
    x, want = mixed(z, ["itext", "xorshift"] * 3 + ["itext"], 1)
    stored = E.plan(x)[2]
    assert stored == [False, True] * 3 + [False, True]  # (the 1-byte tail goes stored too)
    rc, got, off = host_form(z, x)
    assert rc == 0 and got == want and off == positions(want)
    rc, m, got, off = dev_form(z, gpu, x)
    assert rc == 0 and got == want and off == positions(want)


# 3 ------------------------------------------------------------------------------------------------
def test_every_destination_alignment(z, gpu, oracle):
    x, want = data_of(z, "itext", 2 * 65280 + 1000)
    assert len(positions(want)) == 4
    for at in range(16):
        rc, m, got, off = dev_form(z, gpu, x, out_at=at)
        assert rc == 0 and m == len(want) and got == want, at


def test_every_source_alignment_of_stored_bodies(z, gpu, oracle):
    """(A stored body is copied out of the caller's input: the copy's source side.)"""
    x, want = data_of(z, "xorshift", 65280 + 100)
    for at in range(16):
        rc, m, got, off = dev_form(z, gpu, x, in_at=at, out_at=(5 * at + 1) % 16)
        assert rc == 0 and got == want, at


@pytest.mark.parametrize("kind", ("itext", "lowent4k"))
def test_every_source_alignment_of_stream_bodies(z, gpu, oracle, kind):
    """(A stream body is encoded from the caller's input where it lies: the deflate kernels' unaligned loads, on data with
    matches — text for k_lz_sort's own sort, the 4 KiB pattern for k_lz_index.)"""
    x, want = data_of(z, kind, 65280 + 100)
    assert not E.plan(x)[2][0]  # the full chunk goes as a stream (the pattern's 100-byte tail goes stored)
    rc, host, pos = host_form(z, x)
    assert rc == 0 and host == want
    for at in range(16):
        rc, m, got, off = dev_form(z, gpu, x, in_at=at, out_at=(5 * at + 1) % 16)
        assert rc == 0 and m == len(host) and got == host and off == pos, at


# 4 ------------------------------------------------------------------------------------------------
def test_group_seams(z, gpu, oracle):
    x, want = mixed(z, ["itext", "xorshift", "lowent4k", "xorshift", "itext", "lowent4k", "xorshift", "itext"], 2)
    pos = positions(want)
    assert len(pos) == 10 and E.plan(x)[2][-1]  # 4 + 4 + 1 members and the marker; the 2-byte chunk goes stored
    for flags in (z.ZES_F_PIECES, 0):
        rc, got, off = host_form(z, x, flags)
        assert rc == 0 and got == want and off == pos, flags
        rc, m, got, off = dev_form(z, gpu, x, flags)
        assert rc == 0 and got == want and off == pos, flags


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("itext", 0), ("itext", 1), ("itext", 24), ("lowent4k", 65281), ("xorshift", 2 * 65280 + 1),
                                    ("itext", 5 * 65280 + 12345)])
def test_the_reader_takes_the_result_as_one_batch(z, gpu, oracle, kind, n):
    import torch

    x, want = data_of(z, kind, n)
    rc, blob, _ = host_form(z, x)
    assert rc == 0 and blob == want
    assert pygzip.decompress(blob) == x
    members = z.bgzip_members(n) if n else 0  # (one member: the member-by-member path answers)
    assert z.gunzip(blob).tobytes() == x  # zes_gunzip_alloc
    assert z.last_gunzip_members() == members
    t = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(gpu)
    out = torch.empty(n + 64, dtype=torch.uint8, device=gpu)
    back = z.gunzip_tensor(t, out)
    assert back.cpu().numpy().tobytes() == x
    assert z.last_gunzip_members() == members


# 6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,flags", [("xorshift", 2 * 65280, 0), ("itext", 5 * 65280 + 12345, 0), ("itext", 5 * 65280 + 12345, 4)])
def test_capacity(z, gpu, oracle, kind, n, flags):
    x, want = data_of(z, kind, n)
    need = len(want)
    if kind == "xorshift":
        assert need == z.bgzip_bound(n)
    rc, m, _, _ = dev_form(z, gpu, x, flags, cap=need - 1)  # (dev_form checks the bytes from cap on)
    assert rc == z.ZES_E_NOSPACE and m == need
    rc, m, _, _ = dev_form(z, gpu, x, flags, cap=28)
    assert rc == z.ZES_E_NOSPACE and m == need
    rc, m, got, _ = dev_form(z, gpu, x, flags, cap=need)
    assert rc == 0 and m == need and got == want
    a = np.frombuffer(x, dtype=np.uint8)
    out = np.full(need + CANARY, 0xA5, dtype=np.uint8)
    k = C.c_uint64()
    assert z.lib().zes_bgzip(a.ctypes.data, n, out.ctypes.data, need - 1, C.byref(k), None, flags) == z.ZES_E_NOSPACE and k.value == need
    assert (out[need - 1:] == 0xA5).all()
    assert z.lib().zes_bgzip(a.ctypes.data, n, out.ctypes.data, need, C.byref(k), None, flags) == 0 and out[:need].tobytes() == want


# 7 ------------------------------------------------------------------------------------------------
def test_the_pack_kernel_is_timed(z, gpu, oracle):
    x, want = mixed(z, ["itext", "xorshift", "lowent4k", "xorshift", "itext", "lowent4k", "xorshift", "itext"], 2)
    z.set_profiling(True)
    try:
        rc, m, got, _ = dev_form(z, gpu, x, z.ZES_F_PIECES)
        times = {name: (ms, launches) for name, ms, launches in z.last_kernel_times()}
    finally:
        z.set_profiling(False)
    assert rc == 0 and got == want
    assert times["k_bgzf_pack"][1] == 3 and times["k_crc32_seg"][1] == 3 and times["k_emit"][1] == 3, times
    assert times["k_bgzf_pack"][0] > 0
