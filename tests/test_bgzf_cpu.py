"""The BGZF test helper against CPython's gzip, and the new C entry points without a GPU."""
import ctypes as C
import gzip as pygzip
import struct
import zlib

import numpy as np
import pytest

import _bgzf


def test_helper_files_are_gzip_and_state_their_sizes():
    rng = np.random.default_rng(1)
    chunks = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1, 2, 15, 16, 17, 4097, 60000)] + [b"abc" * 21000]
    for kw in (dict(), dict(level=0), dict(level=1), dict(level=9), dict(strategy=zlib.Z_FIXED), dict(eof=False),
               dict(extra_before=b"XY\x03\x00abc", extra_after=b"ZZ\x00\x00"), dict(level=[0, 1, 9, 6, 6, 1, 0, 9])):
        blob = _bgzf.bgzf(chunks, **kw)
        assert pygzip.decompress(blob) == b"".join(chunks)
        ms = _bgzf.walk(blob)
        assert len(ms) == len(chunks) + (0 if kw.get("eof") is False else 1)
        for pos, size, hlen in ms:
            assert blob[pos:pos + 3] == b"\x1f\x8b\x08" and hlen + 8 <= size
    plain = _bgzf.bgzf(chunks[:2])
    assert plain[:18] == b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", _bgzf.walk(plain)[0][1] - 1)
    assert plain.endswith(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00\x1b\x00\x03\x00" + b"\x00" * 8)  # htslib's marker


def test_damages_do_what_they_say():
    chunks = [b"one " * 700, b"two " * 9000, b"three " * 3, b"four" * 300]
    want = b"".join(chunks)
    for kind in _bgzf.DECODABLE:
        blob, _ = _bgzf.damage(chunks, kind)
        assert blob != _bgzf.bgzf(chunks) and pygzip.decompress(blob) == want, kind
    for kind in _bgzf.RAISING:
        blob, _ = _bgzf.damage(chunks, kind)
        with pytest.raises((pygzip.BadGzipFile, zlib.error, EOFError)):
            pygzip.decompress(blob)


def test_new_entry_points_without_a_gpu(z):
    import torch

    L = z.lib()
    off, ln, crc = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(4), (C.c_uint32 * 1)()
    buf = np.zeros(16, dtype=np.uint8)
    # null arguments are refused before anything else, with or without a device
    assert L.zes_crc32_batch_dev(buf.ctypes.data, None, ln, crc, 1) == z.ZES_E_ARG
    assert L.zes_crc32_batch_dev(buf.ctypes.data, off, None, crc, 1) == z.ZES_E_ARG
    assert L.zes_crc32_batch_dev(buf.ctypes.data, off, ln, None, 1) == z.ZES_E_ARG
    if torch.cuda.is_available():
        return  # (what a device answers is the GPU tests' subject)
    assert L.zes_crc32_batch_dev(buf.ctypes.data, off, ln, crc, 1) == z.ZES_E_DEVICE
    assert L.zes_last_gunzip_members() == 0
    blob = np.frombuffer(_bgzf.bgzf([b"a" * 100, b"b" * 100]), dtype=np.uint8)
    for flags in (0, z.ZES_F_GZIP_SERIAL):
        with pytest.raises(z.ZlibEsError) as ei:
            z.gunzip(blob, flags)
        assert ei.value.code == z.ZES_E_DEVICE
