"""Member-parallel gunzip of BGZF files and the segmented CRC-32 on the MI355X.  Expected bytes and checksums come from
CPython's gzip / zlib, never from this library."""
import ctypes as C
import gzip as pygzip
import zlib

import numpy as np
import pytest

import _bgzf

pytestmark = pytest.mark.gpu

KINDS = ("xorshift", "lowent4k", "itext")


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def dev_form(z, gpu, blob, cap, flags=0):
    """zes_gunzip_dev with the input at offset 3 of its tensor -> (status, out_len, bytes)."""
    import torch

    t = dev(np.frombuffer(b"\x00" * 3 + blob + b"\x00", dtype=np.uint8), gpu)
    out = torch.empty(max(cap, 16), dtype=torch.uint8, device=gpu)
    n = C.c_uint64()
    rc = z.lib().zes_gunzip_dev(t.data_ptr() + 3, len(blob), out.data_ptr(), cap, C.byref(n), flags)
    return rc, n.value, (out[: n.value].cpu().numpy().tobytes() if rc == 0 else None)


def host_form(z, blob, flags=0):
    """zes_gunzip_alloc -> (status, bytes, sizes the allocator was asked for)."""
    a = np.frombuffer(blob, dtype=np.uint8)
    asked, keep = [], []

    def alloc(_user, _index, n):
        asked.append(int(n))
        keep.append(np.empty(max(int(n), 1), dtype=np.uint8))
        return keep[-1].ctypes.data

    n = C.c_uint64()
    rc = z.lib().zes_gunzip_alloc(a.ctypes.data, a.size, z.ALLOC_FN(alloc), None, C.byref(n), flags)
    return rc, (keep[0][: n.value].tobytes() if rc == 0 else None), asked


def check_parallel(z, gpu, blob, members):
    """Host form, device form and the serial-flag forms all give CPython's bytes; the first two count `members`."""
    want = pygzip.decompress(blob)
    rc, got, asked = host_form(z, blob)
    assert rc == 0 and got == want and asked == [len(want)]
    assert z.last_gunzip_members() == members
    rc, n, got = dev_form(z, gpu, blob, len(want) + 64)
    assert rc == 0 and n == len(want) and got == want
    assert z.last_gunzip_members() == members
    rc, got, asked = host_form(z, blob, z.ZES_F_GZIP_SERIAL)
    assert rc == 0 and got == want and asked == [len(want)] and z.last_gunzip_members() == 0
    rc, n, got = dev_form(z, gpu, blob, len(want) + 64, z.ZES_F_GZIP_SERIAL)
    assert rc == 0 and got == want and z.last_gunzip_members() == 0
    return want


# ---------------------------------------------------------------------------------------------
# segmented CRC-32
# ---------------------------------------------------------------------------------------------
EDGE_LENGTHS = (0, 1, 15, 16, 17, 31, 4095, 65280, 65535, 65536, 65537, 131073, (1 << 20) + 3)


@pytest.mark.parametrize("fill", ["random", "ff", "zero"])
def test_crc32_batch_edge_lengths_at_every_alignment(z, gpu, fill):
    offs, lens, cur = [], [], 0
    for n in EDGE_LENGTHS:
        for al in range(16):
            cur = (cur + 15) // 16 * 16 + al
            offs.append(cur)
            lens.append(n)
            cur += n
    total = cur + 16
    a = {"random": lambda: np.random.default_rng(5).integers(0, 256, total, dtype=np.uint8), "ff": lambda: np.full(total, 255, dtype=np.uint8),
         "zero": lambda: np.zeros(total, dtype=np.uint8)}[fill]()
    t = dev(a, gpu)
    assert t.data_ptr() % 16 == 0
    got = z.crc32_batch_tensor(t, offs, lens)
    mv = memoryview(a)
    for o, n, c in zip(offs, lens, got):
        assert c == zlib.crc32(mv[o:o + n]), (o % 16, n)


def test_crc32_batch_many_short_buffers_and_none(z, gpu):
    rng = np.random.default_rng(6)
    lens = rng.integers(1, 301, 5000).tolist()
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).tolist()
    a = rng.integers(0, 256, sum(lens), dtype=np.uint8)
    t = dev(a, gpu)
    got = z.crc32_batch_tensor(t, offs, lens)
    mv = memoryview(a)
    assert got == [zlib.crc32(mv[o:o + n]) for o, n in zip(offs, lens)]
    assert z.crc32_batch_tensor(t, [], []) == []
    assert z.lib().zes_crc32_batch_dev(t.data_ptr(), None, None, None, 0) == 0


# ---------------------------------------------------------------------------------------------
# the parallel path
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standard(z):
    a = z.gen("itext", 41, 5 * 65280 + 1234).tobytes()
    chunks = [a[i:i + 65280] for i in range(0, len(a), 65280)]
    assert [len(c) for c in chunks] == [65280] * 5 + [1234]
    return _bgzf.bgzf(chunks), a


def test_kernels_are_timed_by_name(z, gpu, standard):
    blob, a = standard
    z.set_profiling(True)
    try:
        assert z.gunzip(blob).tobytes() == a
        host = [k[0] for k in z.last_kernel_times()]
        rc, n, got = dev_form(z, gpu, blob, len(a) + 64)
        devn = [k[0] for k in z.last_kernel_times()]
    finally:
        z.set_profiling(False)
    assert rc == 0 and got == a
    assert "k_crc32_seg" in host and "k_gz_gather" in host and "k_gz_walk" not in host
    assert "k_crc32_seg" in devn and "k_gz_gather" in devn and "k_gz_walk" in devn


def test_standard_shape(z, gpu, standard):
    blob, a = standard
    assert check_parallel(z, gpu, blob, 7) == a


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_members_of_mixed_encoders(z, gpu, kind):
    """Members of 1 .. 65536 bytes from zlib level 0 (stored), 1, 9 and Z_FIXED and from this library's encoder, mixed in
    one file.  A member holds at most 64 KiB (BSIZE is 16 bits), so a chunk whose body does not fit one (65535 and 65536
    stored bytes, random bytes at any level) goes in as two members of half the size from the same encoder."""
    sizes = (1, 2, 15, 16, 17, 4097, 65535, 65536)
    a = z.gen(kind, 43, sum(sizes) * 4 + 2 * (131072 * 2 + 5) + 4).tobytes()
    chunks, bodies, p = [], [], 0

    def add(n, level, strategy=0, own=False):
        nonlocal p
        c = a[p:p + n]
        p += n
        body = z.deflate_raw(np.frombuffer(c, dtype=np.uint8)).tobytes() if own else _bgzf.raw_body(c, level, strategy)
        if 26 + len(body) > 65536:  # does not fit one member (incompressible bytes): in halves, the same encoder
            assert not own
            p -= n
            add(n // 2, level, strategy)
            add(n - n // 2, level, strategy)
            return
        chunks.append(c)
        bodies.append(body)

    for level, strategy in ((0, 0), (1, 0), (9, 0), (6, zlib.Z_FIXED)):
        for n in sizes:
            add(n, level, strategy)
    # this library's own encoder (the reference's: its streams take T1), more than one of its 128 KiB blocks where the
    # stream still fits a member's 64 KiB: 2 * 131072 + 5 bytes of lowent4k, 131072 + 5 of itext, 60000 random ones
    for n in (131072 * 2 + 5, 131072 + 5, 60000):
        if 26 + z.deflate_raw(np.frombuffer(a[p:p + n], dtype=np.uint8)).size <= 65536:
            add(n, 0, own=True)
            break
    else:
        raise AssertionError("no stream of the library's own encoder fits a member")
    add(2, 0, own=True)
    blob = _bgzf.bgzf(chunks, bodies=bodies)
    assert check_parallel(z, gpu, blob, len(chunks) + 1) == b"".join(chunks)


def test_other_subfields_stay_parallel_and_what_goes_serial(z, gpu):
    a = z.gen("itext", 44, 3000).tobytes()
    chunks = [a[:1000], a[1000:1016], a[1016:]]
    blob = _bgzf.bgzf(chunks, extra_before=b"XY\x03\x00abc", extra_after=b"ZZ\x00\x00Q1\x05\x00hello")
    check_parallel(z, gpu, blob, 4)
    ms = _bgzf.bgzf_members(chunks)
    named = ms[1][:3] + b"\x0c" + ms[1][4:18] + b"name\x00" + ms[1][18:]  # FEXTRA | FNAME: valid gzip, not a BGZF member
    check_parallel(z, gpu, ms[0] + named + ms[2] + ms[3], 0)
    check_parallel(z, gpu, _bgzf.bgzf([a], eof=False), 0)  # one qualifying member only


def test_more_members_than_one_inflate_group(z, gpu):
    a = z.gen("itext", 45, 4100 * 16).tobytes()
    blob = _bgzf.bgzf([a[i:i + 16] for i in range(0, len(a), 16)])
    want = pygzip.decompress(blob)
    assert want == a
    assert z.gunzip(blob).tobytes() == a and z.last_gunzip_members() == 4101
    rc, n, got = dev_form(z, gpu, blob, len(a))
    assert rc == 0 and got == a and z.last_gunzip_members() == 4101


# ---------------------------------------------------------------------------------------------
# fallback
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def damage_chunks(z):
    a = z.gen("itext", 46, 3000 + 65280 + 17 + 1234).tobytes()
    cuts = (0, 3000, 3000 + 65280, 3000 + 65280 + 17, len(a))
    return [a[cuts[i]:cuts[i + 1]] for i in range(4)]


@pytest.mark.parametrize("kind", _bgzf.DECODABLE)
def test_damage_cpython_still_reads(z, gpu, damage_chunks, kind):
    blob, _ = _bgzf.damage(damage_chunks, kind)
    check_parallel(z, gpu, blob, 0)


@pytest.mark.parametrize("kind", _bgzf.RAISING)
def test_damage_cpython_raises_on(z, gpu, damage_chunks, kind):
    blob, body_at = _bgzf.damage(damage_chunks, kind)
    with pytest.raises((pygzip.BadGzipFile, zlib.error, EOFError)):
        pygzip.decompress(blob)
    if kind == "body_bit":
        with pytest.raises(z.ZlibEsError) as ei:
            z.inflate_raw(np.frombuffer(blob, dtype=np.uint8), body_at)
        want = ei.value.code
    else:
        want = {"crc_flip": z.ZES_E_CHECKSUM, "isize_wrong": z.ZES_E_CHECKSUM, "cut_trailer": z.ZES_E_GZIP, "garbage": z.ZES_E_GZIP}[kind]
    cap = sum(len(c) for c in damage_chunks) + 64
    for flags in (0, z.ZES_F_GZIP_SERIAL):
        rc, got, asked = host_form(z, blob, flags)
        assert rc == want and asked == [] and z.last_gunzip_members() == 0, (kind, flags)
        rc, n, got = dev_form(z, gpu, blob, cap, flags)
        assert rc == want and z.last_gunzip_members() == 0, (kind, flags)


def test_capacity_one_short(z, gpu, standard):
    blob, a = standard
    for flags in (0, z.ZES_F_GZIP_SERIAL):
        rc, n, _ = dev_form(z, gpu, blob, len(a) - 1, flags)
        assert rc == z.ZES_E_NOSPACE and n == len(a)
        assert z.last_gunzip_members() == 0
    rc, n, got = dev_form(z, gpu, blob, len(a))  # exactly enough: the last data member's 16-byte groups would not fit
    assert rc == 0 and got == a and z.last_gunzip_members() == 7


def test_back_to_back_on_one_context(z, gpu, standard, damage_chunks):
    blob, a = standard
    small = _bgzf.bgzf(damage_chunks)
    plain = pygzip.compress(a[:100000], mtime=0)
    bad, _ = _bgzf.damage(damage_chunks, "crc_flip")
    pad, _ = _bgzf.damage(damage_chunks, "pad_between")
    for _ in range(2):
        check_parallel(z, gpu, blob, 7)
        check_parallel(z, gpu, plain, 0)
        assert host_form(z, bad)[0] == z.ZES_E_CHECKSUM and z.last_gunzip_members() == 0
        assert dev_form(z, gpu, bad, len(a))[0] == z.ZES_E_CHECKSUM and z.last_gunzip_members() == 0
        check_parallel(z, gpu, pad, 0)
        check_parallel(z, gpu, small, 5)


def test_pools_are_given_back(z, gpu, standard):
    blob, a = standard
    z.trim()
    assert z.pool_bytes() == 0
    check_parallel(z, gpu, blob, 7)
    assert z.pool_bytes() > 0
    z.trim()
    assert z.pool_bytes() == 0
    check_parallel(z, gpu, blob, 7)
