"""PNG batch decoding, timed (not a pytest); prints one JSON line and writes it to profiles/png_decode_speed.json.

    python tools/png_speed.py [reps]

Files, written with tests/_png.py's writer from seeded pixels (a gradient plus noise) and CPython's zlib at level 6:
batch      1024 images of 256 x 256 RGBA (128 different ones, eight times each), every row with the filter type that the
           minimum-sum-of-absolute-differences heuristic picks (the adaptive choice of libpng)
single     one image of 4096 x 4096 RGBA whose rows are all Paeth, Average or Up: no restart row, so one wave unfilters it —
           the stated worst case
With the files in device memory: the median wall time of zes_png_decode_dev over the batch after a warm-up (the call ends
in a synchronise), of the same files one call each, and of the single image; the bytes are compared with the writer's input
before anything is timed.  The per-kernel split of one profiled batch call comes from zes_last_kernel_times, and with it
k_png_unfilter's time against the inflate kernels' of the same call.
"""
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
import _png  # noqa: E402

z = ge.load()
z.init(0)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10


def picture(w, h, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = ((xx * (1 + seed % 3) + yy * 2)[:, :, None] + np.arange(4) * 50 + rs.randint(0, 8, size=(h, w, 4))).astype(np.uint8)
    a[:, :, 3] = 255
    return a.reshape(h, w * 4)


def candidates(rows, bpp):
    """The five filtered forms of every row at once: [type] -> (height, rowbytes)."""
    x = rows.astype(np.int32)
    b = np.vstack([np.zeros((1, x.shape[1]), dtype=np.int32), x[:-1]])
    a = np.hstack([np.zeros((x.shape[0], bpp), dtype=np.int32), x[:, :-bpp]])
    c = np.hstack([np.zeros((x.shape[0], bpp), dtype=np.int32), b[:, :-bpp]])
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return [((x - pred) & 255).astype(np.uint8) for pred in (0, a, b, (a + b) >> 1, paeth)]


def png(rows, w, h, allowed):
    """A PNG of the RGBA rows: per row the allowed filter type with the least sum of absolute (signed) filtered bytes."""
    cand = candidates(rows, 4)
    cost = np.stack([np.abs(cand[t].astype(np.int8).astype(np.int32)).sum(axis=1) if t in allowed else np.full(h, 1 << 40) for t in range(5)])
    pick = cost.argmin(axis=0)
    filtered = np.empty((h, 1 + w * 4), dtype=np.uint8)
    filtered[:, 0] = pick
    for t in range(5):
        filtered[pick == t, 1:] = cand[t][pick == t]
    zs = zlib.compress(filtered.tobytes(), 6)
    blob = _png.SIGNATURE + _png.ihdr(w, h, 6, 8) + b"".join(_png.chunk(b"IDAT", zs[k:k + 65536]) for k in range(0, len(zs), 65536)) + _png.chunk(b"IEND")
    return blob, [int(t) for t in np.bincount(pick, minlength=5)]


def median(ts):
    return round(sorted(ts)[len(ts) // 2], 3)


def timed(fn, reps):
    fn()  # warm-up at this shape
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


res = {"reps": REPS}
# ---- the batch ----
W = H = 256
pics = [picture(W, H, 100 + k) for k in range(128)]
made = [png(p, W, H, {0, 1, 2, 3, 4}) for p in pics]
print("batch files made", file=sys.stderr, flush=True)
blobs = [made[k % 128][0] for k in range(1024)]
ioff = np.cumsum([0] + [len(b) + 3 for b in blobs])[:-1].astype(np.uint64)
ilen = np.array([len(b) for b in blobs], dtype=np.uint64)
flat = np.zeros(int(ioff[-1]) + len(blobs[-1]), dtype=np.uint8)
for o, b in zip(ioff, blobs):
    flat[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
t = torch.from_numpy(flat).cuda()
size = W * H * 4
off = np.arange(1024, dtype=np.uint64) * np.uint64(size)
cap = np.full(1024, size, dtype=np.uint64)
out = torch.zeros(1024 * size, dtype=torch.uint8, device="cuda")


def batch():
    _, _, out_len, status, _ = z.png_decode_tensor(t, ioff, ilen, out=out, off=off, cap=cap)
    assert not any(status)


def one_by_one():
    for k in range(1024):
        _, _, _, status, _ = z.png_decode_tensor(t, ioff[k:k + 1], ilen[k:k + 1], out=out, off=off[k:k + 1], cap=cap[k:k + 1])
        assert status == [0]


batch()
host = out.cpu().numpy().reshape(1024, size)
assert all(host[k].tobytes() == pics[k % 128].tobytes() for k in range(1024)), "the batch's bytes differ from the writer's input"
tb = timed(batch, REPS)
tl = timed(one_by_one, max(3, REPS // 3))
z.set_profiling(True)
batch()
kernels = {k: [round(ms, 4), launches] for k, ms, launches in z.last_kernel_times()}
z.set_profiling(False)
inflate_ms = sum(v[0] for k, v in kernels.items() if k.startswith("k_inf"))
unf_ms = kernels["k_png_unfilter"][0]
filters = np.sum([made[k % 128][1] for k in range(1024)], axis=0)
res["batch"] = {"images": 1024, "width": W, "height": H, "file_bytes": int(ilen.sum()), "out_bytes": 1024 * size, "rows_by_filter_type": [int(x) for x in filters],
                "tier": z.last_inflate_tier(), "decode_ms": median(tb), "decode_ms_min_max": [round(min(tb), 3), round(max(tb), 3)],
                "out_gib_per_s": round(1024 * size / 2**30 / (median(tb) / 1e3), 2), "one_call_each_ms": median(tl),
                "one_call_each_over_batch": round(median(tl) / median(tb), 2), "kernels": kernels, "unfilter_ms": unf_ms, "inflate_kernels_ms": round(inflate_ms, 4),
                "unfilter_over_inflate": round(unf_ms / inflate_ms, 3) if inflate_ms else None}
del out, t, host
# ---- the single large image ----
W = H = 4096
pic = picture(W, H, 7)
blob, rows_by_type = png(pic, W, H, {2, 3, 4})
assert rows_by_type[0] == rows_by_type[1] == 0
t = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
size = W * H * 4
out = torch.zeros(size, dtype=torch.uint8, device="cuda")
one = (np.zeros(1, dtype=np.uint64), np.array([len(blob)], dtype=np.uint64), np.array([size], dtype=np.uint64))


def single():
    _, _, _, status, _ = z.png_decode_tensor(t, one[0], one[1], out=out, off=one[0], cap=one[2])
    assert status == [0]


single()
assert out.cpu().numpy().tobytes() == pic.tobytes(), "the single image's bytes differ from the writer's input"
ts = timed(single, max(3, REPS // 3))
z.set_profiling(True)
single()
kernels = {k: [round(ms, 4), launches] for k, ms, launches in z.last_kernel_times()}
z.set_profiling(False)
res["single"] = {"width": W, "height": H, "file_bytes": len(blob), "out_bytes": size, "rows_by_filter_type": rows_by_type, "tier": z.last_inflate_tier(),
                 "decode_ms": median(ts), "out_gib_per_s": round(size / 2**30 / (median(ts) / 1e3), 3), "kernels": kernels}
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "png_decode_speed.json"), "w") as f:
    f.write(line + "\n")
