"""The gzip batch forms against the per-file loops they replace and against the work they cannot avoid (not a pytest); prints one
JSON line and writes it to profiles/gzip_batch_speed.json.

    python tools/gzip_batch_speed.py [runs]

Two workloads of 1024 files of 64 KiB of text (zes_gen "itext"), back to back in device memory: "zes" (the writer's input; the
reader's files are the writer's own) and "cpython" (the reader's files are gzip.compress level 6 of the same text; the writer's
input is the same text, so its row is a second measurement of the first).  Per direction, timed in the same run, alternating call by call after a warm-up,
medians of wall time over `runs` (default 10) with the spread (min, max):
batch_ms   zes_gzip_batch_dev / zes_gunzip_batch_dev of the 1024 files
loop_ms    the loop a caller has without it: zes_gzip_dev / zes_gunzip_dev per file, each into its own 16-byte aligned place
floor_ms   zes_deflate_batch_dev / zes_inflate_batch_dev (the bodies behind a 78 9C, as the batch stages them) plus one
           zes_crc32_batch_dev over the same data: the work the batch cannot avoid
Before anything is timed the batch's files are compared with the loop's byte for byte, and the outputs with the text.  Kernel
times of one profiled call per direction from zes_last_kernel_times.
"""
import ctypes as C
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

z = ge.load()
z.init(0)
L = z.lib()
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
COUNT, LEN = 1024, 64 << 10
up16 = lambda n: (int(n) + 15) & ~15
u64 = lambda v: np.array(v, dtype=np.uint64)
n64 = C.c_uint64()


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3)}


def timed(fns):
    """Every function RUNS times, alternating, after one warm-up each -> a list of times (ms) per function."""
    for f in fns:
        f()
    out = [[] for _ in fns]
    for _ in range(RUNS):
        for k, f in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return out


def kernels_of(f):
    z.set_profiling(True)
    f()
    k = {name: [round(ms, 4), n] for name, ms, n in z.last_kernel_times()}
    z.set_profiling(False)
    return k


plain = [z.gen("itext", 9000 + k, LEN) for k in range(COUNT)]
t = torch.from_numpy(np.concatenate(plain)).cuda()
p_off, p_len = u64(np.arange(COUNT) * LEN), u64([LEN] * COUNT)
res = {"runs": RUNS, "files": COUNT, "file_bytes": LEN}

# ---- the writer ----
bound = z.gzip_batch_bound(p_len)
w_cap = u64([up16(b) for b in bound])
w_off = u64(np.concatenate([[0], np.cumsum(w_cap)[:-1]]))
w_out = torch.zeros(int(w_cap.sum()), dtype=torch.uint8, device="cuda")
w_len, w_st = np.zeros(COUNT, dtype=np.uint64), np.zeros(COUNT, dtype=np.int32)
one_cap = up16(z.gzip_bound(LEN))
l_out = torch.zeros(COUNT * one_cap, dtype=torch.uint8, device="cuda")
l_len = [0] * COUNT
slot = up16(z.deflate_bound(LEN))
slots = torch.zeros(COUNT * slot, dtype=torch.uint8, device="cuda")
s_off, s_cap = u64(np.arange(COUNT) * slot), u64([slot] * COUNT)
s_len, s_st = np.zeros(COUNT, dtype=np.uint64), np.zeros(COUNT, dtype=np.int32)
crcs = np.zeros(COUNT, dtype=np.uint32)
torch.cuda.synchronize()


def gzip_batch():
    rc = L.zes_gzip_batch_dev(t.data_ptr(), p_off.ctypes.data, p_len.ctypes.data, COUNT, w_out.data_ptr(), w_off.ctypes.data, w_cap.ctypes.data,
                              w_len.ctypes.data, w_st.ctypes.data, 0)
    assert rc == 0 and not w_st.any(), rc


def gzip_loop():
    for k in range(COUNT):
        rc = L.zes_gzip_dev(t.data_ptr() + k * LEN, LEN, l_out.data_ptr() + k * one_cap, one_cap, C.byref(n64))
        assert rc == 0, (k, rc)
        l_len[k] = n64.value


def gzip_floor():
    u64p, i32p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    rc = L.zes_deflate_batch_dev(t.data_ptr(), p_off.ctypes.data_as(u64p), p_len.ctypes.data_as(u64p), slots.data_ptr(), s_off.ctypes.data_as(u64p),
                                 s_cap.ctypes.data_as(u64p), s_len.ctypes.data_as(u64p), s_st.ctypes.data_as(i32p), COUNT)
    assert rc == 0 and not s_st.any()
    rc = L.zes_crc32_batch_dev(t.data_ptr(), p_off.ctypes.data_as(u64p), p_len.ctypes.data_as(u64p), crcs.ctypes.data_as(u32p), COUNT)
    assert rc == 0


gzip_batch()
gzip_loop()
wh, lh = w_out.cpu().numpy(), l_out.cpu().numpy()
files = [wh[int(o):int(o) + int(n)].tobytes() for o, n in zip(w_off, w_len)]
assert all(f == lh[k * one_cap:k * one_cap + l_len[k]].tobytes() for k, f in enumerate(files)), "the batch's files are not the loop's"
assert all(gzip.decompress(f) == p.tobytes() for f, p in list(zip(files, plain))[::97])
for tag in ("zes", "cpython"):  # (the writer's input is the same text in both workloads: the second row is a second measurement of it)
    tb, tl, tf = timed([gzip_batch, gzip_loop, gzip_floor])
    row = {"out_bytes": int(w_len.sum()), "batch_ms": stats(tb), "loop_ms": stats(tl), "floor_ms": stats(tf), "kernels": kernels_of(gzip_batch)}
    row["loop_over_batch"] = round(row["loop_ms"]["median"] / row["batch_ms"]["median"], 2)
    row["batch_over_floor"] = round(row["batch_ms"]["median"] / row["floor_ms"]["median"], 2)
    res["gzip_" + tag] = row

# ---- the reader ----
for tag, gz in (("zes", files), ("cpython", [gzip.compress(p.tobytes(), 6, mtime=0) for p in plain])):
    g_len = u64([len(f) for f in gz])
    g_off = u64(np.concatenate([[0], np.cumsum(g_len)[:-1]]))
    g = torch.from_numpy(np.frombuffer(b"".join(gz), dtype=np.uint8).copy()).cuda()
    # the bodies behind 78 9C at 16-byte boundaries, as zes_inflate_batch_dev asks for its inputs
    z_len = u64([len(f) - 18 + 2 for f in gz])
    z_off = u64(np.concatenate([[0], np.cumsum([up16(n) + 64 for n in z_len])[:-1]]))
    zb = np.zeros(int(z_off[-1]) + up16(z_len[-1]) + 64, dtype=np.uint8)
    for f, o in zip(gz, z_off):
        zb[int(o):int(o) + 2] = (0x78, 0x9C)
        zb[int(o) + 2:int(o) + len(f) - 16] = np.frombuffer(f[10:-8], dtype=np.uint8)
    zt = torch.from_numpy(zb).cuda()
    r_out = torch.zeros(COUNT * LEN, dtype=torch.uint8, device="cuda")
    r_len, r_st = np.zeros(COUNT, dtype=np.uint64), np.zeros(COUNT, dtype=np.int32)
    torch.cuda.synchronize()

    def gunzip_batch():
        rc = L.zes_gunzip_batch_dev(g.data_ptr(), g_off.ctypes.data, g_len.ctypes.data, COUNT, r_out.data_ptr(), p_off.ctypes.data, p_len.ctypes.data,
                                    r_len.ctypes.data, r_st.ctypes.data, 0)
        assert rc == 0 and not r_st.any(), rc

    def gunzip_loop():
        for k in range(COUNT):
            rc = L.zes_gunzip_dev(g.data_ptr() + int(g_off[k]), int(g_len[k]), r_out.data_ptr() + k * LEN, LEN, C.byref(n64), 0)
            assert rc == 0 and n64.value == LEN, (k, rc)

    def gunzip_floor():
        u64p, i32p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        rc = L.zes_inflate_batch_dev(zt.data_ptr(), z_off.ctypes.data_as(u64p), z_len.ctypes.data_as(u64p), r_out.data_ptr(), p_off.ctypes.data_as(u64p),
                                     p_len.ctypes.data_as(u64p), r_len.ctypes.data_as(u64p), r_st.ctypes.data_as(i32p), COUNT, 0)
        assert rc == 0 and not r_st.any()
        rc = L.zes_crc32_batch_dev(r_out.data_ptr(), p_off.ctypes.data_as(u64p), p_len.ctypes.data_as(u64p), crcs.ctypes.data_as(u32p), COUNT)
        assert rc == 0

    r_out.zero_()
    gunzip_batch()
    assert z.last_gunzip_batch() == (COUNT, 0) and bool((r_out == t).all()), tag
    r_out.zero_()
    gunzip_loop()
    assert bool((r_out == t).all()), tag
    tb, tl, tf = timed([gunzip_batch, gunzip_loop, gunzip_floor])
    row = {"in_bytes": int(g_len.sum()), "batch_ms": stats(tb), "loop_ms": stats(tl), "floor_ms": stats(tf), "kernels": kernels_of(gunzip_batch)}
    row["loop_over_batch"] = round(row["loop_ms"]["median"] / row["batch_ms"]["median"], 2)
    row["batch_over_floor"] = round(row["batch_ms"]["median"] / row["floor_ms"]["median"], 2)
    res["gunzip_" + tag] = row
    del g, zt, r_out

line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "gzip_batch_speed.json"), "w") as f:
    f.write(line + "\n")
