"""gzip (RFC 1952) and CRC-32 on the MI355X, against CPython's gzip and zlib: the CRC-32 kernel, the gzip writer (its
body is the reference's stream), the gzip reader over every inflate tier, where a raw stream ends (zes_inflate_raw_used)
and the opt-in Adler-32 trailer check of zlib inflate."""
import ctypes as C
import gzip as pygzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

KINDS = ("xorshift", "lowent4k", "itext")


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def member(body_raw, data, flg=0, extra=b"", name=b"", comment=b"", hcrc_ok=True):
    """A gzip member built by hand around a raw DEFLATE body."""
    h = bytearray(b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00\x00\xff")
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\x00"
    if flg & 16:
        h += comment + b"\x00"
    if flg & 2:
        v = zlib.crc32(bytes(h)) & 0xFFFF
        h += struct.pack("<H", v if hcrc_ok else v ^ 1)
    return bytes(h) + body_raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def raw_zlib(data, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def err_code(z, fn):
    with pytest.raises(z.ZlibEsError) as ei:
        fn()
    return ei.value.code


def gunzip_both(z, gpu, blob):
    """gunzip through the host form and the device form (input at an odd offset of its tensor)."""
    import torch

    host = z.gunzip(blob)
    want = pygzip.decompress(blob)
    assert host.tobytes() == want
    t = dev(np.frombuffer(b"\x00" * 3 + blob, dtype=np.uint8), gpu)[3:]
    out = torch.empty(len(want) + 64, dtype=torch.uint8, device=gpu)
    got = z.gunzip_tensor(t, out)
    assert got.cpu().numpy().tobytes() == want
    return want


# ---------------------------------------------------------------------------------------------
# CRC-32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 65535, 65536, 65537, 131073, (1 << 20) + 3, 64 << 20])
def test_crc32_matches_zlib(z, gpu, n):
    rng = np.random.default_rng(n)
    for a in (rng.integers(0, 256, n, dtype=np.uint8), np.full(n, 255, dtype=np.uint8), np.zeros(n, dtype=np.uint8)):
        want = zlib.crc32(a.tobytes())
        assert z.crc32_tensor(dev(a, gpu)) == want
        assert z.crc32(a) == want


def test_crc32_at_unaligned_offsets(z, gpu):
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (3 << 20) + 64, dtype=np.uint8)
    t = dev(base, gpu)
    assert t.data_ptr() % 16 == 0
    for off in (1, 3, 15):
        for n in (17, 65537, (1 << 20) + 3, 3 << 20):
            want = zlib.crc32(base[off:off + n].tobytes())
            assert z.crc32_tensor(t[off:off + n]) == want
            assert z.crc32(base[off:off + n]) == want
            v = C.c_uint32()
            assert z.lib().zes_crc32_dev(t.data_ptr() + off, n, C.byref(v)) == 0 and v.value == want


def test_crc32_kernel_is_timed(z, gpu):
    a = dev(np.arange(1 << 20, dtype=np.uint32).view(np.uint8), gpu)
    z.set_profiling(True)
    try:
        z.crc32_tensor(a)
        names = [k[0] for k in z.last_kernel_times()]
    finally:
        z.set_profiling(False)
    assert "k_crc32" in names


def test_pool_bytes_counts_what_trim_gives_back(z, gpu):
    """zes_pool_bytes is "what zes_trim would give back" (include/zes.h): the CRC-32 pools are freed by trim, so they count."""
    a = dev(np.arange(1 << 20, dtype=np.uint32).view(np.uint8), gpu)  # 4 MiB
    z.trim()
    assert z.pool_bytes() == 0
    z.crc32_tensor(a)
    assert z.pool_bytes() > 0
    z.trim()
    assert z.pool_bytes() == 0


# ---------------------------------------------------------------------------------------------
# gzip writer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 131072 * 3 + 5, (1 << 20) + 77, 64 << 20])
def test_gzip_writer(z, gpu, n):
    for kind in KINDS:
        a = z.gen(kind, 31, n)
        out = z.gzip(a)
        raw = z.deflate_raw(a)
        assert out[:10].tobytes() == bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
        assert out[10:-8].tobytes() == raw.tobytes()
        assert struct.unpack("<II", out[-8:].tobytes()) == (zlib.crc32(a.tobytes()), n & 0xFFFFFFFF)
        assert pygzip.decompress(out.tobytes()) == a.tobytes()
        t = z.gzip_tensor(dev(a, gpu))
        assert t.cpu().numpy().tobytes() == out.tobytes()


# ---------------------------------------------------------------------------------------------
# gzip reader, valid inputs
# ---------------------------------------------------------------------------------------------
def test_gunzip_cpython_levels_and_stored(z, gpu):
    for kind in ("itext", "xorshift"):
        a = z.gen(kind, 5, 3 << 20).tobytes()
        for level in (1, 6, 9):
            gunzip_both(z, gpu, pygzip.compress(a, compresslevel=level, mtime=0))
        gunzip_both(z, gpu, member(raw_zlib(a, 0), a))  # stored blocks: the parallel stored path


def test_gunzip_header_fields(z, gpu):
    a = z.gen("itext", 6, 200000).tobytes()
    body = raw_zlib(a, 6)
    for flg, kw in [(4, dict(extra=b"AB\x02\x00xy")), (8, dict(name=b"file.txt")), (16, dict(comment=b"c" * 5000)),
                    (2, {}), (2 | 4 | 8 | 16, dict(extra=b"\x00" * 300, name=b"n" * 9000, comment=b"hello"))]:
        gunzip_both(z, gpu, member(body, a, flg, **kw))


def test_gunzip_members_unaligned_with_padding(z, gpu):
    parts = [z.gen("itext", 7, n).tobytes() for n in (1000, 0, 131073, 17)]
    blob = pygzip.compress(parts[0]) + b"\x00" * 5 + pygzip.compress(parts[1]) + pygzip.compress(parts[2], 9) + b"\x00" \
        + pygzip.compress(parts[3]) + b"\x00" * 4100
    assert gunzip_both(z, gpu, blob) == b"".join(parts)


def test_gunzip_of_own_gzip_takes_tier1(z, gpu):
    a = z.gen("itext", 8, (8 << 20) + 3)
    blob = z.gzip(a).tobytes()
    assert z.gunzip(blob).tobytes() == a.tobytes()
    assert z.last_inflate_tier() == 1
    gunzip_both(z, gpu, blob)
    assert z.last_inflate_tier() == 1


def test_gunzip_foreign_64mib_takes_tier2(z, gpu):
    a = z.gen("itext", 9, 64 << 20).tobytes()
    blob = pygzip.compress(a, compresslevel=6, mtime=0)
    assert z.gunzip(blob).tobytes() == a
    assert z.last_inflate_tier() == 2


def test_gunzip_nospace_reports_size(z, gpu):
    import torch

    a = z.gen("itext", 10, 300000).tobytes()
    blob = pygzip.compress(a) + pygzip.compress(a[:1000])
    t = dev(np.frombuffer(blob, dtype=np.uint8), gpu)
    with pytest.raises(z.ZlibEsError) as ei:
        z.gunzip_tensor(t, torch.empty(4096, dtype=torch.uint8, device=gpu))
    assert ei.value.code == z.ZES_E_NOSPACE and ei.value.need == len(a) + 1000


# ---------------------------------------------------------------------------------------------
# gzip reader, bad inputs
# ---------------------------------------------------------------------------------------------
def test_gunzip_bad_inputs(z, gpu):
    import torch

    a = z.gen("itext", 11, 100000).tobytes()
    good = member(raw_zlib(a, 6), a, 2)  # with FHCRC
    n = len(good)
    cases = {
        "magic": (b"\x1f\x8a" + good[2:], z.ZES_E_GZIP),
        "cm": (good[:2] + b"\x09" + good[3:], z.ZES_E_GZIP),
        "reserved": (good[:3] + bytes([good[3] | 0x80]) + good[4:], z.ZES_E_GZIP),
        "short header": (good[:9], z.ZES_E_GZIP),
        "empty": (b"", z.ZES_E_GZIP),
        "trailer cut to 7": (good[:-1], z.ZES_E_GZIP),
        "crc": (good[:n - 8] + bytes([good[n - 8] ^ 1]) + good[n - 7:], z.ZES_E_CHECKSUM),
        "isize": (good[:n - 2] + bytes([good[n - 2] ^ 4]) + good[n - 1:], z.ZES_E_CHECKSUM),
        "fhcrc": (good[:10] + bytes([good[10] ^ 1]) + good[11:], z.ZES_E_CHECKSUM),
        "garbage after": (good + b"\x01garbage", z.ZES_E_GZIP),
    }
    for what, (blob, code) in cases.items():
        assert err_code(z, lambda: z.gunzip(blob)) == code, what
        buf = np.frombuffer(blob + b"\x00", dtype=np.uint8)
        t = dev(buf, gpu)[: len(blob)]
        assert err_code(z, lambda: z.gunzip_tensor(t, torch.empty(len(a) + 64, dtype=torch.uint8, device=gpu))) == code, what
    # an error inside a body: the status zes_inflate_raw gives on those bytes
    bad = bytearray(good)
    bad[12] |= 0x06  # BTYPE 3 (the body starts at 12 behind the FHCRC field)
    want = err_code(z, lambda: z.inflate_raw(bytes(bad), 12))
    assert err_code(z, lambda: z.gunzip(bytes(bad))) == want


# ---------------------------------------------------------------------------------------------
# where a raw stream ends
# ---------------------------------------------------------------------------------------------
def expected_used(body):
    d = zlib.decompressobj(-15)
    d.decompress(body + b"TRAILING")
    return len(body) + 8 - len(d.unused_data)


def test_inflate_raw_used_every_tier(z, gpu):
    seen = set()
    streams = []
    for kind in KINDS:
        a = z.gen(kind, 12, (3 << 20) + 1001)
        streams.append((a.tobytes(), z.deflate_raw(a).tobytes()))  # the reference's stream
        streams.append((a.tobytes(), raw_zlib(a.tobytes(), 6)))
    small = z.gen("itext", 13, 3000).tobytes()
    streams.append((small, raw_zlib(small, 9)))
    streams.append((b"", raw_zlib(b"", 6)))
    streams.append((small, raw_zlib(small, 0)))
    big = z.gen("itext", 14, 3 << 20).tobytes()
    streams.append((big, raw_zlib(big, 0)))
    for data, body in streams:
        padded = b"\x07" * 5 + body + b"TRAILING"
        want = expected_used(body)
        assert want == len(body)
        for flags in (0, z.ZES_F_NO_FASTPATH, z.ZES_F_PIECES):
            out, used = z.inflate_raw_used(padded, 5, flags)
            assert out.tobytes() == data and used == want, (len(data), flags, used, want)
            seen.add(z.last_inflate_tier())
            n, u = C.c_uint64(), C.c_uint64()
            import torch

            t = dev(np.frombuffer(padded, dtype=np.uint8), gpu)
            o = torch.empty(len(data) + 64, dtype=torch.uint8, device=gpu)
            rc = z.lib().zes_inflate_raw_used_dev(t.data_ptr(), t.numel(), 5, o.data_ptr(), o.numel(), C.byref(n), C.byref(u), flags)
            assert rc == 0 and n.value == len(data) and u.value == want
    assert {1, 2, 3} <= seen, seen


def test_inflate_raw_used_t2_pieces_in_child(z, gpu):
    script = r"""
import sys, zlib
sys.path.insert(0, %r)
import torch
import __graft_entry__ as ge
z = ge.load()
z.init(0)
a = z.gen("itext", 15, 24 << 20).tobytes()
co = zlib.compressobj(6, zlib.DEFLATED, -15)
body = co.compress(a) + co.flush()
out, used = z.inflate_raw_used(body + b"TAIL", 0)
assert out.tobytes() == a, "output"
assert used == len(body), (used, len(body))
assert z.last_inflate_tier() == 2, z.last_inflate_tier()
print("pieces ok")
""" % ROOT
    env = dict(os.environ, ZES_SEG_PIECE_MB="1")
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "pieces ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------
# ZES_F_CHECK_ADLER
# ---------------------------------------------------------------------------------------------
def test_check_adler_flag(z, gpu):
    import torch

    a = z.gen("itext", 16, (2 << 20) + 9)
    comp = z.deflate(a).tobytes()
    assert z.inflate(comp, z.ZES_F_CHECK_ADLER).tobytes() == a.tobytes()
    flipped = comp[:-1] + bytes([comp[-1] ^ 0x10])
    cut = comp[:-4]
    for bad in (flipped, cut):
        assert err_code(z, lambda: z.inflate(bad, z.ZES_F_CHECK_ADLER)) == z.ZES_E_CHECKSUM
        assert z.inflate(bad).tobytes() == a.tobytes()  # without the flag the trailer is ignored
    out = torch.empty(a.size + 64, dtype=torch.uint8, device=gpu)
    assert z.inflate_tensor(dev(np.frombuffer(comp, dtype=np.uint8), gpu), out, z.ZES_F_CHECK_ADLER).numel() == a.size
    assert err_code(z, lambda: z.inflate_tensor(dev(np.frombuffer(flipped, dtype=np.uint8), gpu), out, z.ZES_F_CHECK_ADLER)) == z.ZES_E_CHECKSUM
    # another encoder's stream (another tier) with its real trailer
    other = zlib.compress(a.tobytes(), 6)
    assert z.inflate(other, z.ZES_F_CHECK_ADLER).tobytes() == a.tobytes()


# ---------------------------------------------------------------------------------------------
# Node: gzip() / gunzip() of the N-API façade
# ---------------------------------------------------------------------------------------------
def test_node_gzip_gunzip(gpu):
    import shutil

    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_gzip_test.js")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "gzip node checks passed" in out.stdout
