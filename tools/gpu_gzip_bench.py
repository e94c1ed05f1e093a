"""gzip and CRC-32 against their zlib-format counterparts on 64 MiB (not a pytest); prints one JSON line.

    python tools/gpu_gzip_bench.py [reps]
    python tools/gpu_gzip_bench.py [reps] --bgzf     the member-parallel reader instead (below)

k_crc32: kernel time from the library's own events (zes_last_kernel_times), aligned 64 MiB.  The entry points: median
wall time of `reps` calls on device buffers (each call ends synchronised), same input and same body for both sides:
zes_gzip_dev vs zes_deflate_dev, zes_gunzip_dev vs zes_inflate_dev of the stream zes_deflate_dev made (random64,
text64), and zes_gunzip_dev of CPython's gzip level 6 vs zes_inflate_dev of the zlib stream with the same body (text64).

--bgzf: zes_gunzip_dev of a BGZF file of 64 MiB (65280-byte members, CPython level 6, the end-of-file marker), text and
random bytes: median wall time of the call as it is, of the same call with ZES_F_GZIP_SERIAL (the member-by-member path),
and from one profiled call the kernel times of k_gz_walk, k_gz_gather and k_crc32_seg.  CRC row: k_crc32_seg over the 1028
outputs of 65280 bytes in one launch against the sum of k_crc32 over the same buffers one call each.  A library without
the batch entry points (an older commit, for the baseline) reports the plain call and the k_crc32 sum only.
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
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
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


def bgzf_file(data, member=65280):
    out = []
    for i in range(0, len(data), member):
        c = data[i:i + member]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = co.compress(c) + co.flush()
        size = 18 + len(body) + 8
        if size > 65536:  # (level 6 on random bytes grows a little: the member holds stored blocks instead, as bgzip does)
            co = zlib.compressobj(0, zlib.DEFLATED, -15)
            body = co.compress(c) + co.flush()
            size = 18 + len(body) + 8
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", size - 1) + body
                   + struct.pack("<II", zlib.crc32(c), len(c)))
    out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00\x1b\x00\x03\x00" + b"\x00" * 8)
    return b"".join(out)


def bgzf_rows():
    batch = hasattr(L, "zes_crc32_batch_dev") and hasattr(z, "last_gunzip_members")
    res["mode"] = "bgzf"
    res["member_parallel"] = batch
    back = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    for name, kind in (("text64", "itext"), ("random64", "xorshift")):
        host = z.gen(kind, 12345, N)
        blob = bgzf_file(host.tobytes())
        t = dev(blob)
        row = {"file_bytes": len(blob), "members": (N + 65279) // 65280 + 1}
        row["gunzip_ms"] = round(median_ms(lambda: L.zes_gunzip_dev(t.data_ptr(), t.numel(), back.data_ptr(), back.numel(), C.byref(n), 0)), 3)
        assert n.value == N and torch.equal(back[:N], torch.from_numpy(host).cuda())
        if batch:
            row["members_parallel"] = z.last_gunzip_members()
            row["gunzip_serial_flag_ms"] = round(median_ms(
                lambda: L.zes_gunzip_dev(t.data_ptr(), t.numel(), back.data_ptr(), back.numel(), C.byref(n), z.ZES_F_GZIP_SERIAL)), 3)
            assert z.last_gunzip_members() == 0
            row["speedup_over_serial_flag"] = round(row["gunzip_serial_flag_ms"] / row["gunzip_ms"], 2)
            z.set_profiling(True)
            ks = []
            for _ in range(REPS + 1):
                assert L.zes_gunzip_dev(t.data_ptr(), t.numel(), back.data_ptr(), back.numel(), C.byref(n), 0) == 0
                ks.append({k: (ms, cnt) for k, ms, cnt in z.last_kernel_times()})
            z.set_profiling(False)
            for k in ("k_gz_walk", "k_gz_gather", "k_crc32_seg"):
                row[k + "_ms"] = round(sorted(x[k][0] for x in ks[1:])[REPS // 2], 4)
            row["kernels_ms"] = {k: round(v[0], 4) for k, v in ks[-1].items()}
        res["bgzf_" + name] = row
        if name == "random64":  # CRC row: the 1028 outputs where they lie
            offs = list(range(0, N, 65280))
            lens = [min(65280, N - o) for o in offs]
            want = [zlib.crc32(host[o:o + ln].tobytes()) for o, ln in zip(offs[:3], lens[:3])]
            crc = {"buffers": len(offs)}
            z.set_profiling(True)
            v = C.c_uint32()
            one = []
            for _ in range(3):
                tot = 0.0
                for o, ln in zip(offs, lens):
                    assert L.zes_crc32_dev(back.data_ptr() + o, ln, C.byref(v)) == 0
                    tot += sum(ms for k, ms, _ in z.last_kernel_times() if k == "k_crc32")
                one.append(tot)
            crc["k_crc32_one_by_one_ms"] = round(sorted(one)[1], 4)
            if batch:
                seg = []
                for _ in range(REPS + 1):
                    got = z.crc32_batch_tensor(back, offs, lens)
                    seg.append(sum(ms for k, ms, _ in z.last_kernel_times() if k == "k_crc32_seg"))
                assert got[:3] == want
                crc["k_crc32_seg_ms"] = round(sorted(seg[1:])[REPS // 2], 4)
                crc["k_crc32_seg_GBps"] = round(N / crc["k_crc32_seg_ms"] / 1e6, 1)
            z.set_profiling(False)
            res["bgzf_crc"] = crc
    print(json.dumps(res))


def zlib_rows():
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


if __name__ == "__main__":  # (tools/gpu_bgzf_read_bench.py imports bgzf_file and the helpers)
    if "--bgzf" in sys.argv:
        bgzf_rows()
    else:
        zlib_rows()
