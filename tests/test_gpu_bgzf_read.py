"""Range reads of a BGZF file through its member index on the MI355X (zes_bgzf_read, zes_bgzf_read_dev).  Expected bytes
are slices of CPython's gzip.decompress of the same file."""
import ctypes as C
import gzip as pygzip

import numpy as np
import pytest

import _bgzf

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 0, 4096, 65280, 33, 5000)
KINDS = ("itext", "itext", "xorshift", "itext", "itext", "xorshift", "itext", "xorshift", "itext")
LEVELS = (6, 0, 1, 9, 6, 0, 6, 9, None)  # None: the library's own encoder (the block-parallel tier decodes it)


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope="module")
def standard(z, gpu):
    chunks, bodies = [], []
    for i, (n, kind, level) in enumerate(zip(SIZES, KINDS, LEVELS)):
        c = z.gen(kind, 50 + i, n).tobytes()
        chunks.append(c)
        bodies.append(z.deflate_raw(np.frombuffer(c, dtype=np.uint8)).tobytes() if level is None else _bgzf.raw_body(c, level))
    blob = _bgzf.bgzf(chunks, bodies=bodies)
    plain = pygzip.decompress(blob)
    assert plain == b"".join(chunks)
    index = z.bgzf_index(blob)
    assert index[1].tolist() == np.concatenate(([0], np.cumsum(SIZES + (0,)))).tolist()
    return blob, plain, index


def touched(uoff, pos, length):
    """Members with output that hold a byte of [pos, pos + length), clipped to the data: none for an empty range."""
    end = min(pos + length, int(uoff[-1]))
    return sum(1 for k in range(uoff.size - 1) if max(int(uoff[k]), pos) < min(int(uoff[k + 1]), end))


def ranges(uoff):
    total = int(uoff[-1])
    u = [int(v) for v in uoff]
    return [
        ("inside one member", u[6] + 55, 100),
        ("exactly one member", u[6], u[7] - u[6]),
        ("middle of member 2 to middle of member 6", u[2] + 4, u[6] + 6000 - (u[2] + 4)),
        ("starting on a boundary", u[5], 100),
        ("ending on a boundary", u[3] + 8, u[4] - (u[3] + 8)),
        ("the last byte", total - 1, 1),
        ("no bytes", 100, 0),
        ("at the end", total, 10),
        ("past the end", u[7] + 25, 10 ** 6),
        ("the whole file", 0, total),
    ]


def dev_read(z, gpu, t, t_off, c, index, pos, length, out_off=0, cap=None, flags=0, room=None):
    """zes_bgzf_read_dev with the file at byte t_off of t and the result at byte out_off of a tensor filled with 0xA5 ->
    (status, out_len, the whole output tensor on the host)."""
    import torch

    coff, uoff = index
    want = max(min(length, int(uoff[-1]) - pos), 0)
    room = want if room is None else room
    out = torch.full((out_off + room + 48,), 0xA5, dtype=torch.uint8, device=gpu)
    n = C.c_uint64()
    rc = z.lib().zes_bgzf_read_dev(t.data_ptr() + t_off, c, coff.ctypes.data, uoff.ctypes.data, coff.size - 1, pos, length, out.data_ptr() + out_off,
                                   room if cap is None else cap, C.byref(n), flags)
    return rc, n.value, out.cpu().numpy()


def host_read(z, blob, index, pos, length):
    """zes_bgzf_read -> (status, bytes)."""
    a = np.frombuffer(blob, dtype=np.uint8)
    coff, uoff = index
    out = np.full(max(min(length, int(uoff[-1]) - pos), 0) + 16, 0xA5, dtype=np.uint8)
    n = C.c_uint64()
    rc = z.lib().zes_bgzf_read(a.ctypes.data, a.size, coff.ctypes.data, uoff.ctypes.data, coff.size - 1, pos, length, out.ctypes.data, out.size - 16,
                               C.byref(n), 0)
    assert (out[out.size - 16:] == 0xA5).all()
    return rc, out[:n.value].tobytes()


def test_ranges_both_forms(z, gpu, standard):
    import torch

    blob, plain, index = standard
    t = dev(np.frombuffer(blob, dtype=np.uint8), gpu)
    for name, pos, length in ranges(index[1]):
        want = plain[pos:pos + length]
        count = touched(index[1], pos, length)
        got = z.bgzf_read(blob, index, pos, length)
        assert got.dtype == np.uint8 and got.tobytes() == want, name
        assert z.last_gunzip_members() == count, name
        out = torch.empty(len(want) + 1, dtype=torch.uint8, device=gpu)
        view = z.bgzf_read_tensor(t, index, pos, length, out)
        assert view.numel() == len(want) and view.cpu().numpy().tobytes() == want, name
        assert z.last_gunzip_members() == count, name
        if name == "the whole file":
            assert count == 8 and z.gunzip(blob).tobytes() == got.tobytes()
    for flags in (z.ZES_F_PIECES,):
        rc, n, out = dev_read(z, gpu, t, 0, len(blob), index, 20, 70000, flags=flags)
        assert rc == 0 and out[:n].tobytes() == plain[20:70020]


@pytest.mark.parametrize("out_off", [0, 1, 15])
def test_device_form_writes_its_bytes_only(z, gpu, standard, out_off):
    blob, plain, index = standard
    t3 = dev(np.frombuffer(b"\x1f\x8b\x08" + blob + b"\x1f", dtype=np.uint8), gpu)
    t0 = dev(np.frombuffer(blob, dtype=np.uint8), gpu)
    for t, t_off in ((t0, 0), (t3, 3)):
        for name, pos, length in ranges(index[1]):
            want = plain[pos:pos + length]
            rc, n, out = dev_read(z, gpu, t, t_off, len(blob), index, pos, length, out_off)
            assert rc == 0 and n == len(want), name
            assert out[out_off:out_off + n].tobytes() == want, name
            assert (out[:out_off] == 0xA5).all() and (out[out_off + n:] == 0xA5).all(), name


def test_capacity_one_short(z, gpu, standard):
    import torch

    blob, plain, index = standard
    t = dev(np.frombuffer(blob, dtype=np.uint8), gpu)
    for pos, length in ((10, 5000), (0, len(plain)), (len(plain) - 7, 100)):
        n_want = min(length, len(plain) - pos)
        rc, n, out = dev_read(z, gpu, t, 0, len(blob), index, pos, length, cap=n_want - 1)
        assert rc == z.ZES_E_NOSPACE and n == n_want and (out == 0xA5).all()
        assert z.last_gunzip_members() == 0
        with pytest.raises(z.ZlibEsError) as ei:
            z.bgzf_read_tensor(t, index, pos, length, torch.empty(n_want - 1, dtype=torch.uint8, device=gpu))
        assert ei.value.code == z.ZES_E_NOSPACE and ei.value.need == n_want


@pytest.fixture(scope="module")
def damage_chunks(z):
    a = z.gen("itext", 61, 3000 + 20000 + 1234).tobytes()
    return [a[:3000], a[3000:23000], a[23000:]]


def both_statuses(z, gpu, blob, index, pos, length):
    t = dev(np.frombuffer(blob, dtype=np.uint8), gpu)
    rc_h, got_h = host_read(z, blob, index, pos, length)
    members_h = z.last_gunzip_members()
    rc_d, n, out = dev_read(z, gpu, t, 0, len(blob), index, pos, length)
    members_d = z.last_gunzip_members()
    if rc_h == 0:
        assert got_h == out[:n].tobytes()
    else:
        assert members_h == 0 and members_d == 0
    assert rc_h == rc_d
    return rc_h, got_h


def test_damage_stays_in_its_member(z, gpu, damage_chunks):
    plain = b"".join(damage_chunks)
    # crc_flip: the first member alone reads fine, the damaged one does not
    blob, _ = _bgzf.damage(damage_chunks, "crc_flip")
    index = z.bgzf_index(blob)
    assert both_statuses(z, gpu, blob, index, 0, 3000) == (0, plain[:3000])
    assert both_statuses(z, gpu, blob, index, 23000, 1234) == (0, plain[23000:])
    assert both_statuses(z, gpu, blob, index, 2990, 20)[0] == z.ZES_E_CHECKSUM
    assert both_statuses(z, gpu, blob, index, 5000, 1)[0] == z.ZES_E_CHECKSUM
    # isize_wrong: the index follows the wrong field, the decoded length does not
    blob, _ = _bgzf.damage(damage_chunks, "isize_wrong")
    index = z.bgzf_index(blob)
    assert int(index[1][2]) == 3000 + (20000 ^ 1)
    assert both_statuses(z, gpu, blob, index, 10, 100) == (0, plain[10:110])
    assert both_statuses(z, gpu, blob, index, 3000, 50)[0] == z.ZES_E_CHECKSUM
    # body_bit: what zes_inflate_raw says about that body
    blob, body_at = _bgzf.damage(damage_chunks, "body_bit")
    index = z.bgzf_index(blob)
    with pytest.raises(z.ZlibEsError) as ei:
        z.inflate_raw(np.frombuffer(blob, dtype=np.uint8), body_at)
    assert both_statuses(z, gpu, blob, index, 10, 100) == (0, plain[10:110])
    assert both_statuses(z, gpu, blob, index, 2000, 3000)[0] == ei.value.code


def test_stale_index(z, gpu):
    a = z.gen("itext", 62, 6000).tobytes()
    # two files of the same length: stored members, the first two cut differently; the third is the same in both
    file_a = _bgzf.bgzf([a[:1000], a[1000:3000], a[3000:]], level=0)
    file_b = _bgzf.bgzf([a[:2000], a[2000:3000], a[3000:]], level=0)
    assert len(file_a) == len(file_b) and file_a != file_b
    index_a = z.bgzf_index(file_a)
    assert both_statuses(z, gpu, file_b, index_a, 3000, 3000) == (0, a[3000:])
    assert both_statuses(z, gpu, file_b, index_a, 10, 10)[0] == z.ZES_E_GZIP
    assert both_statuses(z, gpu, file_b, index_a, 1500, 10)[0] == z.ZES_E_GZIP
    assert both_statuses(z, gpu, file_b, index_a, 2990, 20)[0] == z.ZES_E_GZIP
    shifted = (index_a[0].copy(), index_a[1].copy())
    shifted[0][1] += 1
    assert both_statuses(z, gpu, file_a, shifted, 3000, 3000) == (0, a[3000:])
    assert both_statuses(z, gpu, file_a, shifted, 10, 10)[0] == z.ZES_E_GZIP
    assert both_statuses(z, gpu, file_a, shifted, 1500, 10)[0] == z.ZES_E_GZIP
    assert both_statuses(z, gpu, file_a, index_a, 10, 5000) == (0, a[10:5010])


def test_back_to_back_on_one_context(z, gpu, standard):
    blob, plain, index = standard
    z.trim()
    before = z.pool_bytes()
    first = z.bgzf_read(blob, index, 30, 70000).tobytes()
    assert first == plain[30:70030]
    assert z.gunzip(blob).tobytes() == plain
    assert z.bgzf_read(blob, index, 30, 70000).tobytes() == first
    t = dev(np.frombuffer(blob, dtype=np.uint8), gpu)
    rc, n, out = dev_read(z, gpu, t, 0, len(blob), index, 30, 70000)
    assert rc == 0 and out[:n].tobytes() == first
    assert z.pool_bytes() > before
    z.trim()
    assert z.pool_bytes() == before
