"""ZIP batch extraction against the per-entry loop it replaces (not a pytest); prints one JSON line and writes it to
profiles/zip_read_bench.json.

    python tools/gpu_zip_bench.py [reps]

Archives, built from zes_gen seeds with the builder of tests/_zip.py:
text1024   1024 entries of 64 KiB of itext, CPython level 6
own64      64 entries of 1 MiB of itext whose bodies are the library's own deflate_raw
mixed      256 entries of 4 KiB to 256 KiB: CPython level 1, 6 and 9, the library's own, and every fourth one stored (random bytes)
For each, with the file in device memory: the median wall time of zes_zip_read_dev over all entries after a warm-up, and, in
the same process and alternating with it call by call, of the baseline a caller has without it: per entry zes_inflate_raw_dev
then zes_crc32_dev of the result (a stored entry: zes_crc32_dev of its bytes in the file), every CRC compared.  Both sides'
bytes are compared with the inputs before anything is timed.  The host form, zes_zip_read_alloc with the file in the caller's
memory and an allocator that hands out parts of one array made beforehand, is timed the same way on its own (`host_ms`), its
bytes compared first.  Kernel times of one profiled zes_zip_read_dev call from zes_last_kernel_times.
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
import _zip  # noqa: E402

z = ge.load()
z.init(0)
L = z.lib()
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10


def own(data):
    return z.deflate_raw(np.frombuffer(data, dtype=np.uint8)).tobytes()


def archive(name):
    """(bytes, [plain bytes]) of one of the three archives."""
    entries = []
    if name == "text1024":
        for k in range(1024):
            entries.append(_zip.entry(b"text/%04d.txt" % k, z.gen("itext", 1000 + k, 64 << 10).tobytes(), level=6))
    elif name == "own64":
        for k in range(64):
            d = z.gen("itext", 3000 + k, 1 << 20).tobytes()
            entries.append(_zip.entry(b"own/%02d.bin" % k, d, body=own(d)))
    else:
        for k in range(256):
            n = (4 << 10) * (1 + (k * 37) % 64) + (k % 5)
            if k % 4 == 3:
                entries.append(_zip.entry(b"mixed/%03d.raw" % k, z.gen("xorshift", 5000 + k, n).tobytes(), method=0))
            else:
                d = z.gen("itext" if k % 3 else "lowent4k", 5000 + k, n).tobytes()
                entries.append(_zip.entry(b"mixed/%03d.txt" % k, d, body=own(d) if k % 8 == 0 else None, level=(1, 6, 9)[k % 3]))
    return _zip.build(entries), [e["data"] for e in entries]


res = {"reps": REPS}
n64, crc = C.c_uint64(), C.c_uint32()
for name in ("text1024", "own64", "mixed"):
    blob, plain = archive(name)
    t = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    ent, _ = z.zip_index_tensor(t)
    cnt = ent.size
    assert cnt == len(plain)
    usize = [int(e["usize"]) for e in ent]
    off = np.zeros(cnt, dtype=np.uint64)
    at = 0
    for k in range(cnt):
        off[k] = at
        at += (usize[k] + 15) & ~15
    out = torch.zeros(at + 64, dtype=torch.uint8, device="cuda")
    out_len = np.zeros(cnt, dtype=np.uint64)
    status = np.zeros(cnt, dtype=np.int32)
    data_off = [int(e["hdr_off"]) + 30 + int(e["name_len"]) + _zip.le16(blob, int(e["hdr_off"]) + 28) for e in ent]
    torch.cuda.synchronize()

    def batch():
        rc = L.zes_zip_read_dev(t.data_ptr(), t.numel(), ent.ctypes.data, cnt, None, cnt, out.data_ptr(), off.ctypes.data, out_len.ctypes.data,
                                status.ctypes.data, 0)
        assert rc == 0 and not status.any()
        return rc

    def loop():
        for k in range(cnt):
            e = ent[k]
            if int(e["method"]) == 0:
                rc = L.zes_crc32_dev(t.data_ptr() + data_off[k], usize[k], C.byref(crc))
            else:
                rc = L.zes_inflate_raw_dev(t.data_ptr(), data_off[k] + int(e["csize"]), data_off[k], out.data_ptr() + int(off[k]), (usize[k] + 15) & ~15,
                                           C.byref(n64), 0)
                assert rc == 0 and n64.value == usize[k], (k, rc, n64.value)
                rc = L.zes_crc32_dev(out.data_ptr() + int(off[k]), usize[k], C.byref(crc))
            assert rc == 0 and crc.value == int(e["crc"]), (k, rc)
        return 0

    def same_bytes(stored_too):
        host = out.cpu().numpy()
        return all(host[int(o):int(o) + n].tobytes() == p for o, n, p, e in zip(off, usize, plain, ent) if stored_too or int(e["method"]) == 8)

    # the bytes first, both sides (the loop leaves stored entries where they are)
    batch()
    assert same_bytes(True), name
    out.zero_()
    torch.cuda.synchronize()
    loop()
    assert same_bytes(False), name
    tb, tl = [], []
    for _ in range(REPS):  # alternating, so that neither side has the clocks or the pools to itself
        t0 = time.perf_counter()
        batch()
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        tb.append((t1 - t0) * 1e3)
        tl.append((t2 - t1) * 1e3)
    filea = np.frombuffer(blob, dtype=np.uint8)
    hout = np.zeros(at + 64, dtype=np.uint8)
    alloc = z.ALLOC_FN(lambda _user, i, _n: hout.ctypes.data + int(off[i]))

    def host():
        rc = L.zes_zip_read_alloc(filea.ctypes.data, filea.size, ent.ctypes.data, cnt, None, cnt, alloc, None, out_len.ctypes.data, status.ctypes.data, 0)
        assert rc == 0 and not status.any()
        return rc

    host()
    assert all(hout[int(o):int(o) + n].tobytes() == p for o, n, p in zip(off, usize, plain)), name
    th = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        host()
        th.append((time.perf_counter() - t0) * 1e3)
    z.set_profiling(True)
    batch()
    kernels = {k: [round(ms, 4), launches] for k, ms, launches in z.last_kernel_times()}
    z.set_profiling(False)
    row = {"file_bytes": len(blob), "entries": cnt, "plain_bytes": sum(usize), "stored": int(sum(1 for e in ent if int(e["method"]) == 0)),
           "tier": z.last_inflate_tier(), "zip_read_ms": round(sorted(tb)[REPS // 2], 3), "loop_ms": round(sorted(tl)[REPS // 2], 3),
           "host_ms": round(sorted(th)[REPS // 2], 3), "kernels": kernels}
    row["loop_over_zip_read"] = round(row["loop_ms"] / row["zip_read_ms"], 2)
    res[name] = row
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "zip_read_bench.json"), "w") as f:
    f.write(line + "\n")
