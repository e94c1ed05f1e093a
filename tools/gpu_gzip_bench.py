"""gzip and CRC-32 against their zlib-format counterparts on 64 MiB (not a pytest); prints one JSON line.

    python tools/gpu_gzip_bench.py [reps]

k_crc32: kernel time from the library's own events (zes_last_kernel_times), aligned 64 MiB.  The entry points: median
wall time of `reps` calls on device buffers (each call ends synchronised), same input and same body for both sides:
zes_gzip_dev vs zes_deflate_dev, zes_gunzip_dev vs zes_inflate_dev of the stream zes_deflate_dev made (random64,
text64), and zes_gunzip_dev of CPython's gzip level 6 vs zes_inflate_dev of the zlib stream with the same body (text64).
"""
import ctypes as C
import json
import os
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

z = ge.load()
z.init(0)
L = z.lib()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
N = 64 << 20


def median_ms(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        rc = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, rc
    return sorted(ts)[len(ts) // 2]


def dev(b):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()


res = {"bytes": N, "reps": REPS}
n = C.c_uint64()
for name, kind in (("random64", "xorshift"), ("text64", "itext")):
    host = z.gen(kind, 12345, N)
    t = torch.from_numpy(host).cuda()
    out = torch.empty(z.gzip_bound(N), dtype=torch.uint8, device="cuda")
    back = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    if name == "random64":
        z.set_profiling(True)
        v = C.c_uint32()
        ks = []
        for _ in range(REPS + 1):
            assert L.zes_crc32_dev(t.data_ptr(), N, C.byref(v)) == 0
            ks.append(sum(ms for k, ms, _ in z.last_kernel_times() if k == "k_crc32"))
        z.set_profiling(False)
        kms = sorted(ks[1:])[REPS // 2]
        res["k_crc32_ms"] = round(kms, 4)
        res["k_crc32_GBps"] = round(N / kms / 1e6, 1)
    d_ms = median_ms(lambda: L.zes_deflate_dev(t.data_ptr(), N, out.data_ptr(), out.numel(), C.byref(n)))
    g_ms = median_ms(lambda: L.zes_gzip_dev(t.data_ptr(), N, out.data_ptr(), out.numel(), C.byref(n)))
    gz = out[: n.value].clone()
    assert L.zes_deflate_dev(t.data_ptr(), N, out.data_ptr(), out.numel(), C.byref(n)) == 0
    zl = out[: n.value].clone()
    assert torch.equal(zl[2:-4], gz[10:-8])
    i_ms = median_ms(lambda: L.zes_inflate_dev(zl.data_ptr(), zl.numel(), back.data_ptr(), back.numel(), C.byref(n), 0))
    u_ms = median_ms(lambda: L.zes_gunzip_dev(gz.data_ptr(), gz.numel(), back.data_ptr(), back.numel(), C.byref(n), 0))
    assert n.value == N and torch.equal(back[:N], t)
    res[name] = {"deflate_ms": round(d_ms, 3), "gzip_ms": round(g_ms, 3), "gzip_over_deflate": round(g_ms / d_ms, 3),
                 "inflate_ms": round(i_ms, 3), "gunzip_ms": round(u_ms, 3), "gunzip_over_inflate": round(u_ms / i_ms, 3)}
    if name == "text64":
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = co.compress(host.tobytes()) + co.flush()
        zs = dev(b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(host.tobytes())))
        gs = dev(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + body + struct.pack("<II", zlib.crc32(host.tobytes()), N))
        i6 = median_ms(lambda: L.zes_inflate_dev(zs.data_ptr(), zs.numel(), back.data_ptr(), back.numel(), C.byref(n), 0))
        u6 = median_ms(lambda: L.zes_gunzip_dev(gs.data_ptr(), gs.numel(), back.data_ptr(), back.numel(), C.byref(n), 0))
        assert n.value == N and torch.equal(back[:N], t) and z.last_inflate_tier() == 2
        res["text64_cpython6"] = {"inflate_ms": round(i6, 3), "gunzip_ms": round(u6, 3), "gunzip_over_inflate": round(u6 / i6, 3)}
print(json.dumps(res))
