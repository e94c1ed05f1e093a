"""The BGZF writer against the single-member gzip writer on 64 MiB (not a pytest); prints one JSON line and writes it to
profiles/bgzip_bench.json (or to the path behind --out).

    python tools/gpu_bgzip_bench.py [reps] [--out FILE]

For xorshift, itext and lowent4k bytes in device memory: median wall time of `reps` calls of zes_bgzip_dev and of
zes_gzip_dev on the same input in the same process (each call ends synchronised), their ratio, the result sizes, and from
one profiled call of each the kernel times of the library's own events (zes_last_kernel_times), so that the shares of
k_bgzf_pack and k_crc32_seg show.  The BGZF result is read back once by zes_gunzip_dev (all members as one batch) and
compared with the input; pool_bytes is the pooled device scratch behind the BGZF calls, counted from an empty pool.
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

z = ge.load()
z.init(0)
L = z.lib()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "bgzip_bench.json")
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


def profiled(fn):
    z.set_profiling(True)
    try:
        assert fn() == 0
        return {k: {"ms": round(ms, 4), "launches": cnt} for k, ms, cnt in z.last_kernel_times()}
    finally:
        z.set_profiling(False)


res = {"bytes": N, "reps": REPS, "device": z.device_info()["arch"], "members": z.bgzip_members(N)}
n = C.c_uint64()
out = torch.empty(max(z.bgzip_bound(N), z.gzip_bound(N)), dtype=torch.uint8, device="cuda")
back = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
for kind in ("xorshift", "itext", "lowent4k"):
    t = torch.from_numpy(z.gen(kind, 12345, N)).cuda()
    torch.cuda.synchronize()
    z.trim()
    bgzip = lambda: L.zes_bgzip_dev(t.data_ptr(), N, out.data_ptr(), out.numel(), C.byref(n), None, 0)
    gzip = lambda: L.zes_gzip_dev(t.data_ptr(), N, out.data_ptr(), out.numel(), C.byref(n))
    row = {"bgzip_ms": round(median_ms(bgzip), 3), "bgzip_bytes": n.value, "pool_bytes": z.pool_bytes()}
    blob = out[: n.value].clone()
    assert L.zes_gunzip_dev(blob.data_ptr(), blob.numel(), back.data_ptr(), back.numel(), C.byref(n), 0) == 0
    assert n.value == N and torch.equal(back[:N], t) and z.last_gunzip_members() == res["members"]
    row["bgzip_kernels"] = profiled(bgzip)
    row["gzip_ms"] = round(median_ms(gzip), 3)
    row["gzip_bytes"] = n.value
    row["gzip_kernels"] = profiled(gzip)
    row["bgzip_over_gzip"] = round(row["bgzip_ms"] / row["gzip_ms"], 3)
    row["bgzip_GBps"] = round(N / row["bgzip_ms"] / 1e6, 2)
    ks = row["bgzip_kernels"]
    total = sum(v["ms"] for v in ks.values())
    row["bgzip_kernel_ms_total"] = round(total, 3)
    row["share_k_bgzf_pack"] = round(ks["k_bgzf_pack"]["ms"] / total, 4)
    row["share_k_crc32_seg"] = round(ks["k_crc32_seg"]["ms"] / total, 4)
    res[kind] = row
line = json.dumps(res)
with open(OUT, "w") as f:
    f.write(line + "\n")
print(line)
