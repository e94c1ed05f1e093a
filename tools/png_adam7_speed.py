"""Adam7-interlaced PNG batch decoding, timed (not a pytest); prints one JSON line and writes it to
profiles/png_adam7_speed.json.

    python tools/png_adam7_speed.py [reps]

1024 images of 256 x 256 RGBA (128 different ones, eight times each; tools/png_speed.py's pictures: a gradient plus noise),
CPython's zlib at level 6, every row with the filter type that the minimum-sum-of-absolute-differences heuristic picks:
interlaced   written by tests/_adam7.py: the heuristic per row of each of the seven passes
plain        the same pixels written by tests/_png.py: the yardstick, what the reader decoded before it took Adam7
With the files in device memory: the median wall time of zes_png_decode_dev over each batch after a warm-up (the call ends
in a synchronise), both under ZES_F_PNG_INTERLACED; the bytes are compared with the writer's input before anything is
timed.  The per-kernel split of one profiled call of each comes from zes_last_kernel_times, and with it k_png_deinterlace's
time, its GiB/s of output and its share of the kernels' time.
"""
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
import _adam7  # noqa: E402
import _png  # noqa: E402

z = ge.load()
z.init(0)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
W = H = 256
N, DISTINCT = 1024, 128
SIZE = W * H * 4


def picture(w, h, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = ((xx * (1 + seed % 3) + yy * 2)[:, :, None] + np.arange(4) * 50 + rs.randint(0, 8, size=(h, w, 4))).astype(np.uint8)
    a[:, :, 3] = 255
    return a.reshape(h, w * 4)


def plain_filters(raw):
    """The heuristic's choice for the rows of the whole image: _adam7.minsum's rule, the image as a single pass."""
    x = np.frombuffer(raw, dtype=np.uint8).reshape(H, W * 4).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 4:] = x[:, :-4]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, 4:] = b[:, :-4]
    preds = [np.zeros_like(x), a, b, (a + b) >> 1, _png._paeth_np(a, b, c)]
    cost = [np.abs(((x - p) & 255).astype(np.uint8).view(np.int8).astype(np.int32)).sum(axis=1) for p in preds]
    return [int(t) for t in np.argmin(np.stack(cost), axis=0)]


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


pics = [picture(W, H, 100 + k).tobytes() for k in range(DISTINCT)]
made = {"interlaced": [_adam7.write(W, H, 6, 8, p, _adam7.minsum(p, W, H, 6, 8)) for p in pics],
        "plain": [_png.write(W, H, 6, 8, p, plain_filters(p)) for p in pics]}
print("files made", file=sys.stderr, flush=True)
off = np.arange(N, dtype=np.uint64) * np.uint64(SIZE)
cap = np.full(N, SIZE, dtype=np.uint64)
res = {"reps": REPS, "images": N, "distinct": DISTINCT, "width": W, "height": H, "out_bytes": N * SIZE}
for name in ("plain", "interlaced"):
    blobs = [made[name][k % DISTINCT] for k in range(N)]
    ioff = np.cumsum([0] + [len(b) + 3 for b in blobs])[:-1].astype(np.uint64)
    ilen = np.array([len(b) for b in blobs], dtype=np.uint64)
    flat = np.zeros(int(ioff[-1]) + len(blobs[-1]), dtype=np.uint8)
    for o, b in zip(ioff, blobs):
        flat[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    t = torch.from_numpy(flat).cuda()
    out = torch.zeros(N * SIZE, dtype=torch.uint8, device="cuda")

    def batch():
        _, _, _, status, _ = z.png_decode_tensor(t, ioff, ilen, out=out, off=off, cap=cap, flags=z.ZES_F_PNG_INTERLACED)
        assert not any(status)

    batch()
    host = out.cpu().numpy().reshape(N, SIZE)
    assert all(host[k].tobytes() == pics[k % DISTINCT] for k in range(N)), "the %s batch's bytes differ from the writer's input" % name
    ts = timed(batch, REPS)
    z.set_profiling(True)
    batch()
    kernels = {k: [round(ms, 4), launches] for k, ms, launches in z.last_kernel_times()}
    z.set_profiling(False)
    res[name] = {"file_bytes": int(ilen.sum()), "tier": z.last_inflate_tier(), "decode_ms": median(ts), "decode_ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
                 "out_gib_per_s": round(N * SIZE / 2**30 / (median(ts) / 1e3), 2), "kernels": kernels, "kernels_ms": round(sum(v[0] for v in kernels.values()), 4),
                 "unfilter_ms": kernels["k_png_unfilter"][0]}
    del out, t, host
d = res["interlaced"]
dms = d["kernels"]["k_png_deinterlace"][0]
assert "k_png_deinterlace" not in res["plain"]["kernels"]
res["interlaced_over_plain"] = round(d["decode_ms"] / res["plain"]["decode_ms"], 3)
res["deinterlace"] = {"ms": dms, "out_gib_per_s": round(N * SIZE / 2**30 / (dms / 1e3), 1), "share_of_kernels": round(dms / d["kernels_ms"], 4),
                      "share_of_call": round(dms / d["decode_ms"], 4), "over_unfilter": round(dms / d["unfilter_ms"], 3)}
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "png_adam7_speed.json"), "w") as f:
    f.write(line + "\n")
