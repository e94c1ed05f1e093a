"""The BGZF member index on the host (zes_bgzf_index needs no device), and what zes_bgzf_index* / zes_bgzf_read* decide
before a device is touched.  Expected indexes come from tests/_bgzf.py's walk and the ISIZE fields, never from the library."""
import ctypes as C
import gzip as pygzip

import numpy as np
import pytest

import _bgzf
import _bgzf_index_cases as cases
import _bgzip_expect


@pytest.fixture(scope="module")
def files():
    return cases.files()


def host_index(z, blob, cap=None):
    a = np.frombuffer(blob, dtype=np.uint8)
    return cases.c_index(z.lib().zes_bgzf_index, a.ctypes.data if a.size else None, a.size, 0, cap)


def test_host_index_is_the_walk(z, files):
    for name, (blob, plain) in files.items():
        assert pygzip.decompress(blob) == plain, name
        coff, uoff = cases.expected(blob)
        rc, members, got_c, got_u = host_index(z, blob)
        assert rc == 0 and members == coff.size - 1, name
        assert (got_c == coff).all() and (got_u == uoff).all(), name
        assert int(got_u[-1]) == len(plain) and int(got_c[-1]) == len(blob), name
        pc, pu = z.bgzf_index(blob)
        assert pc.dtype == np.uint64 and pu.dtype == np.uint64 and (pc == coff).all() and (pu == uoff).all(), name
    assert files["marker_alone"][0] == _bgzip_expect.EOF_MARKER and z.bgzf_index(files["marker_alone"][0])[0].tolist() == [0, 28]
    assert z.bgzf_index(files["one_member_no_marker"][0])[0].size == 2


def test_host_index_of_the_writers_files(z, files):
    for n in cases.WRITER_SIZES:
        blob, plain = files["writer_%d" % n]
        coff, uoff = z.bgzf_index(blob)
        assert coff.size == _bgzip_expect.members(n) + 1
        chunks, bodies, _ = _bgzip_expect.plan(plain)
        sizes = [len(m) for m in _bgzf.bgzf_members(chunks, bodies=bodies)]
        assert coff[:-1].tolist() == np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64).tolist()  # what the writer reports as member_off
        assert uoff.tolist() == [min(k * 65280, n) for k in range(coff.size)]


@pytest.mark.parametrize("exact", [False, True])
def test_fake_headers_in_stored_payloads_are_not_members(z, exact):
    blob, plain = cases.fake_header_file(exact)
    assert pygzip.decompress(blob) == plain
    # the fake header is complete and qualifies on its own ...
    tail = blob[cases.FAKE_AT:]
    size = int.from_bytes(tail[16:18], "little") + 1
    assert tail[:4] == b"\x1f\x8b\x08\x04" and tail[10:16] == b"\x06\x00BC\x02\x00" and 18 + 8 <= size <= len(tail)
    first = _bgzf.walk(blob)[0][1]
    assert (cases.FAKE_AT + size == first) == exact
    # ... and the index is that of the three real members
    coff, uoff = z.bgzf_index(blob)
    ec, eu = cases.expected(blob)
    assert coff.size == 4 and (coff == ec).all() and (uoff == eu).all()


def test_files_that_are_not_bgzf_to_the_last_byte(z):
    m = C.c_uint64(7)
    assert z.lib().zes_bgzf_index(None, 0, None, None, 0, C.byref(m), 0) == z.ZES_E_GZIP and m.value == 0
    chunks = cases.damage_chunks()
    for kind in cases.GZIP_KINDS:
        blob, _ = _bgzf.damage(chunks, kind)
        rc, members, _, _ = host_index(z, blob)
        assert rc == z.ZES_E_GZIP, kind
        with pytest.raises(z.ZlibEsError) as ei:
            z.bgzf_index(blob)
        assert ei.value.code == z.ZES_E_GZIP, kind
    whole = _bgzf.bgzf(chunks)
    for cut in (len(whole) - 28 + 5, len(whole) - 28 + 17, len(whole) - 1):  # inside the marker's header, inside its trailer
        assert host_index(z, whole[:cut])[0] == z.ZES_E_GZIP, cut


def test_damage_that_does_not_concern_the_index(z):
    chunks = cases.damage_chunks()
    for kind in cases.OK_KINDS:
        blob, _ = _bgzf.damage(chunks, kind)
        coff, uoff = cases.expected(blob)
        rc, members, got_c, got_u = host_index(z, blob)
        assert rc == 0 and members == 5 and (got_c == coff).all() and (got_u == uoff).all(), kind
    blob, _ = _bgzf.damage(chunks, "isize_wrong")
    _, uoff = z.bgzf_index(blob)
    assert int(uoff[3]) - int(uoff[2]) == len(chunks[2]) ^ 1  # the wrong field, followed


def test_count_query_and_nospace(z, files):
    blob = files["ragged"][0]
    a = np.frombuffer(blob, dtype=np.uint8)
    want = len(_bgzf.walk(blob))
    m = C.c_uint64(0)
    assert z.lib().zes_bgzf_index(a.ctypes.data, a.size, None, None, 0, C.byref(m), 0) == z.ZES_E_NOSPACE and m.value == want
    rc, members, coff, uoff = host_index(z, blob, cap=want)  # one entry short
    assert rc == z.ZES_E_NOSPACE and members == want
    assert (coff == 0xA5A5A5A5A5A5A5A5).all() and (uoff == 0xA5A5A5A5A5A5A5A5).all()
    rc, members, coff, uoff = host_index(z, blob, cap=want + 1)
    assert rc == 0 and members == want


def read_call(z, fn, blob_arr, coff, uoff, pos, length, out, cap, members=None, flags=0, null=()):
    n = C.c_uint64(0xDEAD)
    args = dict(inp=blob_arr.ctypes.data, coff=coff.ctypes.data, uoff=uoff.ctypes.data, out=out.ctypes.data, n=C.byref(n))
    for k in null:
        args[k] = None
    rc = fn(args["inp"], blob_arr.size, args["coff"], args["uoff"], coff.size - 1 if members is None else members, pos, length, args["out"], cap,
            args["n"], flags)
    return rc, n.value


def test_argument_errors_and_nospace_before_the_device(z, files):
    L = z.lib()
    blob, plain = files["ragged"]
    a = np.frombuffer(blob, dtype=np.uint8)
    coff, uoff = cases.expected(blob)
    m = C.c_uint64()
    big = np.zeros(coff.size, dtype=np.uint64)
    for fn in (L.zes_bgzf_index, L.zes_bgzf_index_dev):
        assert fn(a.ctypes.data, a.size, big.ctypes.data, big.ctypes.data, big.size, None, 0) == z.ZES_E_ARG  # null members
        assert fn(None, a.size, big.ctypes.data, big.ctypes.data, big.size, C.byref(m), 0) == z.ZES_E_ARG  # null input, c != 0
        for bad in (1, 4, 32, 128, z.ZES_F_INDEX_WALK | 2):
            assert fn(a.ctypes.data, a.size, big.ctypes.data, big.ctypes.data, big.size, C.byref(m), bad) == z.ZES_E_ARG, bad
        assert fn(a.ctypes.data, a.size, None, big.ctypes.data, big.size, C.byref(m), 0) == z.ZES_E_ARG  # only one array
        assert fn(a.ctypes.data, a.size, big.ctypes.data, None, big.size, C.byref(m), 0) == z.ZES_E_ARG
        assert fn(None, 0, None, None, 0, C.byref(m), 0) == z.ZES_E_GZIP  # c == 0: no file
    assert L.zes_bgzf_index(a.ctypes.data, a.size, big.ctypes.data, big.ctypes.data, big.size, C.byref(m), z.ZES_F_INDEX_WALK) == 0  # ignored by the host form
    total = len(plain)
    out = np.full(total + 16, 0xA5, dtype=np.uint8)
    for fn in (L.zes_bgzf_read, L.zes_bgzf_read_dev):
        for k in ("inp", "coff", "uoff", "out", "n"):
            assert read_call(z, fn, a, coff, uoff, 0, 10, out, out.size, null=(k,))[0] == z.ZES_E_ARG, k
        assert read_call(z, fn, a, coff, uoff, 0, 10, out, out.size, members=0)[0] == z.ZES_E_ARG
        assert read_call(z, fn, a, coff, uoff, total + 1, 10, out, out.size)[0] == z.ZES_E_ARG
        for bad in (1, 2, 8, 32, 64, z.ZES_F_PIECES | 1):
            assert read_call(z, fn, a, coff, uoff, 0, 10, out, out.size, flags=bad)[0] == z.ZES_E_ARG, bad
        # capacity one short: the size needed, decided from the index alone
        assert read_call(z, fn, a, coff, uoff, 5, 1000, out, 999) == (z.ZES_E_NOSPACE, 1000)
        assert read_call(z, fn, a, coff, uoff, total - 10, 1000, out, 9) == (z.ZES_E_NOSPACE, 10)
        # nothing to read: no device work
        assert read_call(z, fn, a, coff, uoff, 5, 0, out, out.size) == (0, 0)
        assert read_call(z, fn, a, coff, uoff, total, 77, out, out.size) == (0, 0)
        assert L.zes_last_gunzip_members() == 0
    assert (out == 0xA5).all()
    with pytest.raises(z.ZlibEsError) as ei:
        z.bgzf_read(blob, (coff, uoff), total + 1, 1)
    assert ei.value.code == z.ZES_E_ARG
    assert z.bgzf_read(blob, (coff, uoff), total, 5).size == 0


def test_no_device(z, files):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    blob, plain = files["ragged"]
    a = np.frombuffer(blob, dtype=np.uint8)
    coff, uoff = cases.expected(blob)
    out = np.zeros(64, dtype=np.uint8)
    assert read_call(z, z.lib().zes_bgzf_read, a, coff, uoff, 3, 20, out, out.size)[0] == z.ZES_E_DEVICE
    m = C.c_uint64()
    assert z.lib().zes_bgzf_index_dev(a.ctypes.data, a.size, None, None, 0, C.byref(m), 0) == z.ZES_E_DEVICE
    with pytest.raises(z.ZlibEsError) as ei:
        z.bgzf_read(blob, (coff, uoff), 3, 20)
    assert ei.value.code == z.ZES_E_DEVICE
