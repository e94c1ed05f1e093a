"""CPU-side checks of the gzip container and the CRC-32 kernel: status strings, the bound, the cases decided on the host
before the device, no CPU fallback, and a register check of the CRC kernel compiled on its own."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def test_gzip_status_strings(z):
    assert z.ZES_E_GZIP == -20 and z.ZES_E_CHECKSUM == -21 and z.ZES_F_CHECK_ADLER == 16
    g, c = z.strerror(z.ZES_E_GZIP), z.strerror(z.ZES_E_CHECKSUM)
    assert g and c and g != c
    assert g != z.strerror(-100) and c != z.strerror(-100)  # (not the unknown-status string)


def test_gzip_bound_arithmetic(z):
    for n in (0, 1, 2, 65535, 65536, 131072, 131073, 1 << 20, (64 << 20) + 5):
        assert z.gzip_bound(n) == z.deflate_bound(n) - 6 + 18


def test_gzip_throw_sizes_are_decided_before_the_device(z):
    for n in (0, 1, 131073):
        with pytest.raises(z.ZlibEsError) as ei:
            z.gzip(np.zeros(n, dtype=np.uint8))
        assert ei.value.code == -3  # ZES_E_CORRUPT, the reference's "Data is corrupted"


def test_gunzip_bad_header_is_decided_before_the_device(z):
    good = bytearray(gzip.compress(b"hello hello hello", mtime=0))
    for bad in (b"\x1f\x8c" + bytes(good[2:]),          # magic
                bytes(good[:2]) + b"\x07" + bytes(good[3:]),  # CM
                bytes(good[:3]) + b"\x20" + bytes(good[4:]),  # a reserved FLG bit
                bytes(good[:7]),                        # cut short
                b""):
        with pytest.raises(z.ZlibEsError) as ei:
            z.gunzip(bad)
        assert ei.value.code == z.ZES_E_GZIP


def test_no_cpu_fallback_for_crc_and_gzip(z):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    a = np.arange(1000, dtype=np.uint8)
    for call in (lambda: z.crc32(a), lambda: z.gzip(a), lambda: z.gunzip(gzip.compress(a.tobytes(), mtime=0))):
        with pytest.raises(z.ZlibEsError) as ei:
            call()
        assert ei.value.code == z.ZES_E_DEVICE


def test_crc_kernel_has_no_spills(tmp_path):
    src = os.path.join(ROOT, "zlib.es_amd", "csrc", "zes_crc.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "x.o"),
                          "-Wno-unused-function", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    assert any("k_crc32" in ln for ln in lines), out.stderr[-2000:]
    scratch = [ln for ln in lines if "ScratchSize [bytes/lane]" in ln]
    assert scratch and all(ln.rstrip().endswith(": 0 [-Rpass-analysis=kernel-resource-usage]") for ln in scratch), scratch
    spills = [ln for ln in lines if "Spill" in ln]
    assert spills and all(ln.rstrip().endswith(": 0 [-Rpass-analysis=kernel-resource-usage]") for ln in spills), spills
