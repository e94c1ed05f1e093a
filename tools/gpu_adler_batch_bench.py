"""The segmented Adler-32 kernel and ZES_F_CHECK_ADLER in the batch inflate form (not a pytest); prints one JSON line and
writes it to profiles/adler_batch_bench.json.

    python tools/gpu_adler_batch_bench.py [reps]

(a) kernel: zes_adler32_batch_dev over 1024 segments of 65280 bytes at mixed alignments (segment i starts i % 16 bytes
    behind a 16-byte boundary) against a loop of 1024 zes_adler32_dev calls on the same bytes: median wall time of `reps`
    rounds, each call synchronised; and k_adler_seg's own time from the library's events.
(b) against the existing kernel: k_adler_seg's time for one aligned 64 MiB segment against k_adler's on the same buffer,
    both from zes_last_kernel_times, rounds alternating.
(c) the flag: zes_inflate_batch_dev on 128 x 1 MiB (BASELINE.json configs[3]: generator i % 3, seed 12345 + i; streams
    made by zes_deflate_batch_dev) without the flag, with it, and a loop of 128 flagged zes_inflate_dev calls.
"""
import ctypes as C
import json
import os
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


def median(v):
    return sorted(v)[len(v) // 2]


def wall_ms(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return median(ts)


def kernel_ms(fn, name):
    """median of the kernel's own time over REPS profiled calls (the first one left out)"""
    z.set_profiling(True)
    try:
        ks = []
        for _ in range(REPS + 1):
            fn()
            ks.append(sum(ms for k, ms, _ in z.last_kernel_times() if k == name))
    finally:
        z.set_profiling(False)
    return median(ks[1:])


res = {"reps": REPS}

# ---- (a) 1024 segments of 65280 bytes, mixed alignments ----
CNT, SEG = 1024, 65280
host = z.gen("xorshift", 12345, CNT * (SEG + 32) + 64)
arena = torch.from_numpy(host).cuda()
assert arena.data_ptr() % 16 == 0
offs = [i * (SEG + 32) + i % 16 for i in range(CNT)]
c_off, c_len, c_out = (C.c_uint64 * CNT)(*offs), (C.c_uint64 * CNT)(*([SEG] * CNT)), (C.c_uint32 * CNT)()
one = C.c_uint32()


def batch():
    assert L.zes_adler32_batch_dev(arena.data_ptr(), c_off, c_len, c_out, CNT) == 0


def loop():
    for o in offs:
        assert L.zes_adler32_dev(arena.data_ptr() + o, SEG, C.byref(one)) == 0


batch()
assert all(c_out[i] == zlib.adler32(host[offs[i]:offs[i] + SEG].tobytes()) for i in (0, 1, 7, 15, CNT - 1))
a = {"segments": CNT, "segment_bytes": SEG, "batch_ms": round(wall_ms(batch), 4), "loop_ms": round(wall_ms(loop), 4)}
a["loop_over_batch"] = round(a["loop_ms"] / a["batch_ms"], 1)
a["k_adler_seg_ms"] = round(kernel_ms(batch, "k_adler_seg"), 4)
a["k_adler_seg_GBps"] = round(CNT * SEG / a["k_adler_seg_ms"] / 1e6, 1)
res["a_kernel"] = a

# ---- (b) one aligned 64 MiB segment: k_adler_seg against k_adler ----
N = 64 << 20
big = torch.from_numpy(z.gen("xorshift", 777, N)).cuda()
assert big.data_ptr() % 16 == 0
b_off, b_len, b_out = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(N), (C.c_uint32 * 1)()
z.set_profiling(True)
seg, single = [], []
for _ in range(REPS + 1):  # alternating
    assert L.zes_adler32_batch_dev(big.data_ptr(), b_off, b_len, b_out, 1) == 0
    seg.append(sum(ms for k, ms, _ in z.last_kernel_times() if k == "k_adler_seg"))
    assert L.zes_adler32_dev(big.data_ptr(), N, C.byref(one)) == 0
    single.append(sum(ms for k, ms, _ in z.last_kernel_times() if k == "k_adler"))
z.set_profiling(False)
assert b_out[0] == one.value
b = {"bytes": N, "k_adler_seg_ms": round(median(seg[1:]), 4), "k_adler_ms": round(median(single[1:]), 4)}
b["k_adler_seg_GBps"] = round(N / b["k_adler_seg_ms"] / 1e6, 1)
b["k_adler_GBps"] = round(N / b["k_adler_ms"] / 1e6, 1)
b["seg_over_single"] = round(b["k_adler_seg_ms"] / b["k_adler_ms"], 3)
res["b_one_segment"] = b
del big

# ---- (c) the flag on 128 x 1 MiB ----
NB, ONE = 128, 1 << 20
mix = ("xorshift", "itext", "lowent4k")
raws = np.concatenate([z.gen(mix[i % 3], 12345 + i, ONE) for i in range(NB)])
d_raw = torch.from_numpy(raws).cuda()
cap = z.deflate_bound(ONE)
slot = (cap + 15) // 16 * 16
d_comp = torch.zeros(NB * slot + 64, dtype=torch.uint8, device="cuda")
clen, st = z.deflate_batch_tensor(d_raw, [i * ONE for i in range(NB)], [ONE] * NB, d_comp, [i * slot for i in range(NB)], [cap] * NB)
assert not any(st)
d_back = torch.empty(NB * ONE + 64, dtype=torch.uint8, device="cuda")
arr = lambda v: (C.c_uint64 * NB)(*[int(x) for x in v])
i_off, i_len, o_off, o_cap = arr([i * slot for i in range(NB)]), arr(clen), arr([i * ONE for i in range(NB)]), arr([ONE] * NB)
o_len, o_st = (C.c_uint64 * NB)(), (C.c_int32 * NB)()
n = C.c_uint64()


def inflate_batch(flags):
    assert L.zes_inflate_batch_dev(d_comp.data_ptr(), i_off, i_len, d_back.data_ptr(), o_off, o_cap, o_len, o_st, NB, flags) == 0
    assert not any(o_st)


def inflate_loop():
    for i in range(NB):
        assert L.zes_inflate_dev(d_comp.data_ptr() + i * slot, clen[i], d_back.data_ptr() + i * ONE, ONE, C.byref(n), z.ZES_F_CHECK_ADLER) == 0


inflate_batch(z.ZES_F_CHECK_ADLER)
assert torch.equal(d_back[:NB * ONE], d_raw)
c = {"buffers": NB, "buffer_bytes": ONE, "batch_ms": round(wall_ms(lambda: inflate_batch(0)), 4),
     "batch_checked_ms": round(wall_ms(lambda: inflate_batch(z.ZES_F_CHECK_ADLER)), 4), "loop_checked_ms": round(wall_ms(inflate_loop), 4)}
c["checked_over_plain"] = round(c["batch_checked_ms"] / c["batch_ms"], 3)
c["loop_over_checked_batch"] = round(c["loop_checked_ms"] / c["batch_checked_ms"], 2)
c["k_adler_seg_ms"] = round(kernel_ms(lambda: inflate_batch(z.ZES_F_CHECK_ADLER), "k_adler_seg"), 4)
res["c_flag"] = c

line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "adler_batch_bench.json"), "w") as f:
    f.write(line + "\n")
