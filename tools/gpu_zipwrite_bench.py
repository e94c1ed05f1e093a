"""ZIP archive writing against the per-entry loop it replaces and against the batch encoder alone (not a pytest); prints one
JSON line and writes it to profiles/zipwrite_bench.json.

    python tools/gpu_zipwrite_bench.py [reps]

For each of itext, xorshift and lowent4k: 1024 entries of 64 KiB from zes_gen seeds, back to back in device memory, names
"kind/0000.bin".  Timed, alternating call by call in one process after a warm-up, medians of wall time:
zipwrite_ms  zes_zipwrite_dev of the 1024 entries
loop_ms      the loop a caller has without it: per entry zes_deflate_raw_dev straight to the body's place in the archive (a
             capacity of len - 1, so a stream that is not shorter answers ZES_E_NOSPACE and the entry's bytes are copied there
             instead) and zes_crc32_dev.  The headers and the directory, which the caller would still have to upload, are not
             part of it: the figure favours the loop
batch_ms     zes_deflate_batch_dev alone on the same buffers into 16-byte aligned slots: the floor.  What zes_zipwrite_dev takes
             beyond it is the CRC-32 launch, the pack kernel, the directory and the group's round trips
Before anything is timed the archive is read back by zes_zip_read_dev and CPython's zipfile, and the loop's bodies and CRCs are
compared with the archive's.  Kernel times of one profiled zes_zipwrite_dev call from zes_last_kernel_times.
"""
import ctypes as C
import io
import json
import os
import sys
import time
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

z = ge.load()
z.init(0)
L = z.lib()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 9
COUNT, LEN = 1024, 64 << 10
NOSPACE = z.ZES_E_NOSPACE

res = {"reps": REPS, "entries": COUNT, "entry_bytes": LEN}
n64, crc = C.c_uint64(), C.c_uint32()
for kind in ("itext", "xorshift", "lowent4k"):
    plain = [z.gen(kind, 7000 + k, LEN) for k in range(COUNT)]
    names = [b"%s/%04d.bin" % (kind.encode(), k) for k in range(COUNT)]
    t = torch.from_numpy(np.concatenate(plain)).cuda()
    off = np.arange(COUNT, dtype=np.uint64) * np.uint64(LEN)
    ln = np.full(COUNT, LEN, dtype=np.uint64)
    blob = np.frombuffer(b"".join(names), dtype=np.uint8)
    nl = np.array([len(n) for n in names], dtype=np.uint16)
    cap = z.zip_bound(ln, nl)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    out2 = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    ent = np.zeros(COUNT, dtype=z.ZIP_ENTRY)
    bound = z.deflate_bound(LEN)
    slot = (bound + 15) & ~15
    slots = torch.zeros(COUNT * slot, dtype=torch.uint8, device="cuda")
    s_off = np.arange(COUNT, dtype=np.uint64) * np.uint64(slot)
    s_cap = np.full(COUNT, slot, dtype=np.uint64)
    s_len = np.zeros(COUNT, dtype=np.uint64)
    s_st = np.zeros(COUNT, dtype=np.int32)
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    p64 = lambda a: a.ctypes.data_as(u64p)
    torch.cuda.synchronize()

    def zipwrite():
        rc = L.zes_zipwrite_dev(t.data_ptr(), off.ctypes.data, ln.ctypes.data, blob.ctypes.data, nl.ctypes.data, COUNT, out.data_ptr(), cap, C.byref(n64),
                                ent.ctypes.data, 0)
        assert rc == 0, rc
        return n64.value

    size = zipwrite()
    body_at = [int(e["hdr_off"]) + 30 + int(e["name_len"]) for e in ent]
    crcs = [0] * COUNT

    def loop():
        for k in range(COUNT):
            rc = L.zes_deflate_raw_dev(t.data_ptr() + k * LEN, LEN, out2.data_ptr() + body_at[k], LEN - 1, C.byref(n64))
            if rc == NOSPACE:
                out2[body_at[k]:body_at[k] + LEN] = t[k * LEN:(k + 1) * LEN]
            else:
                assert rc == 0, (k, rc)
            rc = L.zes_crc32_dev(t.data_ptr() + k * LEN, LEN, C.byref(crc))
            assert rc == 0
            crcs[k] = crc.value
        torch.cuda.synchronize()

    def batch():
        rc = L.zes_deflate_batch_dev(t.data_ptr(), p64(off), p64(ln), slots.data_ptr(), p64(s_off), p64(s_cap), p64(s_len), s_st.ctypes.data_as(i32p), COUNT)
        assert rc == 0 and not s_st.any()

    # the result first: our own reader and CPython's zipfile extract it, and the loop makes the same bodies and CRCs
    arch = out[:size].cpu().numpy().tobytes()
    with zipfile.ZipFile(io.BytesIO(arch)) as zf:
        assert zf.testzip() is None and all(zf.read(zi) == p.tobytes() for zi, p in zip(zf.infolist(), plain)), kind
    got, goff, glen, gst = z.zip_read_tensor(out[:size], ent)
    host = got.cpu().numpy()
    assert not any(gst) and all((host[int(o):int(o) + LEN] == p).all() for o, p in zip(goff, plain)), kind
    loop()
    h2 = out2.cpu().numpy()
    a = np.frombuffer(arch, dtype=np.uint8)
    assert all((h2[b:b + int(e["csize"])] == a[b:b + int(e["csize"])]).all() and c == int(e["crc"]) for b, e, c in zip(body_at, ent, crcs)), kind
    batch()
    tz, tl, tb = [], [], []
    for _ in range(REPS):  # alternating, so that no side has the clocks or the pools to itself
        t0 = time.perf_counter()
        zipwrite()
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        batch()
        t3 = time.perf_counter()
        tz.append((t1 - t0) * 1e3)
        tl.append((t2 - t1) * 1e3)
        tb.append((t3 - t2) * 1e3)
    z.set_profiling(True)
    zipwrite()
    kernels = {k: [round(ms, 4), launches] for k, ms, launches in z.last_kernel_times()}
    z.set_profiling(False)
    med = lambda v: round(sorted(v)[len(v) // 2], 3)
    row = {"archive_bytes": size, "plain_bytes": COUNT * LEN, "stored": int(sum(1 for e in ent if int(e["method"]) == 0)), "zipwrite_ms": med(tz),
           "loop_ms": med(tl), "batch_ms": med(tb), "kernels": kernels}
    row["loop_over_zipwrite"] = round(row["loop_ms"] / row["zipwrite_ms"], 2)
    row["zipwrite_over_batch"] = round(row["zipwrite_ms"] / row["batch_ms"], 2)
    res[kind] = row
    del t, out, out2, slots
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "zipwrite_bench.json"), "w") as f:
    f.write(line + "\n")
