"""BGZF random access on the 64 MiB files of DESIGN.md §4b (not a pytest); prints one JSON line and writes it to
profiles/bgzf_read_bench.json.

    python tools/gpu_bgzf_read_bench.py [reps]

Files: text64 and random64 as tools/gpu_gzip_bench.py --bgzf builds them (65280-byte members, CPython level 6, the marker).
index   zes_bgzf_index_dev, the parallel finder (flags 0) against the serial walk (ZES_F_INDEX_WALK, the baseline): median
        wall time of `reps` calls after a warm-up, and the median of the kernel's time (k_bgzf_mark / k_gz_walk) from the
        library's own events (zes_last_kernel_times) over `reps` profiled calls
read    zes_bgzf_read_dev of 64 KiB, 1 MiB and 16 MiB from the middle of the file and of the whole file: median wall time,
        members decoded, against zes_gunzip_dev of the whole file (the only way to get at those bytes without an index)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpu_gzip_bench as gb  # noqa: E402  (the file builder, median_ms, the initialised library)

z, L, N, REPS = gb.z, gb.L, gb.N, gb.REPS
res = {"bytes": N, "reps": REPS}
n = C.c_uint64()
m = C.c_uint64()


def kernel_ms(fn, name):
    """Median over REPS profiled calls (after one warm-up) of the kernel's time."""
    z.set_profiling(True)
    ks = []
    for _ in range(REPS + 1):
        assert fn() == 0
        ks.append(sum(ms for k, ms, _ in z.last_kernel_times() if k == name))
    z.set_profiling(False)
    return sorted(ks[1:])[REPS // 2]


for name, kind in (("text64", "itext"), ("random64", "xorshift")):
    host = z.gen(kind, 12345, N)
    blob = gb.bgzf_file(host.tobytes())
    t = gb.dev(blob)
    coff, uoff = z.bgzf_index(blob)
    members = coff.size - 1
    row = {"file_bytes": len(blob), "members": members}
    gc, gu = np.empty_like(coff), np.empty_like(uoff)
    for label, flags, kernel in (("finder", 0, "k_bgzf_mark"), ("walk", z.ZES_F_INDEX_WALK, "k_gz_walk")):
        call = lambda: L.zes_bgzf_index_dev(t.data_ptr(), t.numel(), gc.ctypes.data, gu.ctypes.data, gc.size, C.byref(m), flags)  # noqa: E731
        row["index_%s_ms" % label] = round(gb.median_ms(call), 4)
        assert m.value == members and (gc == coff).all() and (gu == uoff).all()
        row["index_%s_kernel_ms" % label] = round(kernel_ms(call, kernel), 4)
    row["index_walk_over_finder"] = round(row["index_walk_ms"] / row["index_finder_ms"], 2)
    back = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    row["gunzip_whole_ms"] = round(gb.median_ms(lambda: L.zes_gunzip_dev(t.data_ptr(), t.numel(), back.data_ptr(), back.numel(), C.byref(n), 0)), 3)
    want = torch.from_numpy(host).cuda()
    for label, length in (("64k", 64 << 10), ("1m", 1 << 20), ("16m", 16 << 20), ("whole", N)):
        pos = 0 if length == N else N // 2 - length // 2 + 12345  # (the middle of the file, on no member's boundary)
        call = lambda: L.zes_bgzf_read_dev(t.data_ptr(), t.numel(), coff.ctypes.data, uoff.ctypes.data, members, pos, length, back.data_ptr(),  # noqa: E731
                                           back.numel(), C.byref(n), 0)
        row["read_%s_ms" % label] = round(gb.median_ms(call), 3)
        assert n.value == length and torch.equal(back[:length], want[pos:pos + length])
        row["read_%s_members" % label] = z.last_gunzip_members()
        row["gunzip_over_read_%s" % label] = round(row["gunzip_whole_ms"] / row["read_%s_ms" % label], 2)
    res[name] = row
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "bgzf_read_bench.json"), "w") as f:
    f.write(line + "\n")
