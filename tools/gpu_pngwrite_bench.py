"""PNG batch writing, timed (not a pytest); prints one JSON line and writes it to profiles/pngwrite_bench.json.

    python tools/gpu_pngwrite_bench.py [reps]

Images: tools/png_speed.py's content (a gradient plus noise, seeded).
batch      1024 images of 256 x 256 RGBA 8 (128 different ones, eight times each) in device memory, filter value 5: the median
           wall time of zes_pngwrite_dev over the batch after a warm-up (the call ends in a synchronise), and of the same
           images one call each, alternating in one process; the files are read back by zes_png_decode_dev and by PIL before
           anything is timed.  The per-kernel split of one profiled batch call comes from zes_last_kernel_times; with it
           k_png_filter's bytes moved (the scanlines read once and once more as the row above, the filtered bytes written)
           over its time, beside the 8 TB/s that DESIGN.md's rooflines use.
pil        PIL's time to write the same 1024 images to memory on the host's CPUs (compress_level 6, one thread): the
           outside baseline.
single     one image of 4096 x 4096 RGBA written under filter value 5 and under value 6, and zes_png_decode_dev's time for
           each file: what the restart rows at every 64th row buy the reader.
"""
import io
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

z = ge.load()
z.init(0)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
HBM_TB_S = 8.0  # DESIGN.md's roofline figure


def picture(w, h, seed):  # tools/png_speed.py's
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = ((xx * (1 + seed % 3) + yy * 2)[:, :, None] + np.arange(4) * 50 + rs.randint(0, 8, size=(h, w, 4))).astype(np.uint8)
    a[:, :, 3] = 255
    return a.reshape(h, w * 4)


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


def records(n, w, h, filt):
    rec = np.zeros(n, dtype=z.PNGW_IMAGE)
    rec["width"], rec["height"], rec["depth"], rec["colour"], rec["filter"] = w, h, 8, 6, filt
    return rec


res = {"reps": REPS, "design_hbm_tb_per_s": HBM_TB_S}
# ---- the batch ----
W = H = 256
N = 1024
size = W * H * 4
pics = [picture(W, H, 100 + k) for k in range(128)]
flat = np.concatenate([pics[k % 128].reshape(-1) for k in range(N)])
t = torch.from_numpy(flat).cuda()
rec = records(N, W, H, 5)
ioff = np.arange(N, dtype=np.uint64) * np.uint64(size)
ilen = np.full(N, size, dtype=np.uint64)
bound = z.png_bound(rec[:1])[0]
step = (bound + 15) // 16 * 16
off = np.arange(N, dtype=np.uint64) * np.uint64(step)
cap = np.full(N, step, dtype=np.uint64)
out = torch.zeros(N * step, dtype=torch.uint8, device="cuda")
lens = []


def batch():
    _, _, out_len, status = z.png_encode_tensor(t, ioff, ilen, rec, out=out, off=off, cap=cap)
    assert not any(status)
    lens[:] = out_len


def one_by_one():
    for k in range(N):
        _, _, _, status = z.png_encode_tensor(t, ioff[k:k + 1], ilen[k:k + 1], rec[k:k + 1], out=out, off=off[k:k + 1], cap=cap[k:k + 1])
        assert status == [0]


batch()
# the files, read back: by the project's reader on the device, and the first 128 by PIL
back = torch.zeros(N * size, dtype=torch.uint8, device="cuda")
_, _, blen, bstatus, _ = z.png_decode_tensor(out, off, np.array(lens, dtype=np.uint64), out=back, off=ioff, cap=ilen)
assert not any(bstatus) and bool((back == t).all()), "the written files do not decode to the images"
host = out.cpu().numpy()
files = [host[int(off[k]):int(off[k]) + lens[k]].tobytes() for k in range(N)]
try:
    from PIL import Image

    for k in range(128):
        with Image.open(io.BytesIO(files[k])) as p:
            assert p.mode == "RGBA" and p.tobytes() == pics[k].tobytes()
except ImportError:
    Image = None
del back
tb, tl = [], []
for _ in range(2):  # alternating
    tb += timed(batch, REPS)
    tl += timed(one_by_one, max(2, REPS // 5))
z.set_profiling(True)
batch()
kernels = {k: [round(ms, 4), launches] for k, ms, launches in z.last_kernel_times()}
z.set_profiling(False)
filter_ms = kernels["k_png_filter"][0]
moved = N * (2 * size + H * (1 + W * 4))
longest = max(kernels, key=lambda k: kernels[k][0])
encode_ms = round(sum(v[0] for k, v in kernels.items() if k not in ("k_png_filter", "k_png_pack", "k_crc32_seg", "k_crc32_put", "k_adler_seg")), 4)
res["batch"] = {"images": N, "width": W, "height": H, "in_bytes": N * size, "file_bytes": int(sum(lens)), "filter": 5, "encode_ms": median(tb),
                "encode_ms_min_max": [round(min(tb), 3), round(max(tb), 3)], "in_gib_per_s": round(N * size / 2**30 / (median(tb) / 1e3), 2),
                "one_call_each_ms": median(tl), "one_call_each_over_batch": round(median(tl) / median(tb), 2), "kernels": kernels,
                "filter_ms": filter_ms, "filter_bytes_moved": moved, "filter_tb_per_s": round(moved / (filter_ms / 1e3) / 1e12, 3),
                "filter_share_of_hbm_figure": round(moved / (filter_ms / 1e3) / 1e12 / HBM_TB_S, 4), "encoder_kernels_ms": encode_ms,
                "longest_kernel": longest, "batch_faster_than_loop": median(tb) < median(tl), "filter_is_not_the_longest_kernel": longest != "k_png_filter"}
# ---- PIL on the host's CPUs ----
if Image is not None:
    def pil():
        for k in range(N):
            Image.frombuffer("RGBA", (W, H), pics[k % 128], "raw", "RGBA", 0, 1).save(io.BytesIO(), format="PNG", compress_level=6)

    tp = timed(pil, 2)
    res["pil"] = {"version": getattr(sys.modules.get("PIL"), "__version__", None), "threads": 1, "compress_level": 6, "encode_ms": median(tp),
                  "over_batch": round(median(tp) / median(tb), 1)}
del out, t, host, files
# ---- the single large image: what value 5's restart rows buy the reader ----
W = H = 4096
size = W * H * 4
pic = picture(W, H, 7)
t = torch.from_numpy(pic.reshape(-1).copy()).cuda()
one = (np.zeros(1, dtype=np.uint64), np.array([size], dtype=np.uint64))
back = torch.zeros(size, dtype=torch.uint8, device="cuda")
res["single"] = {"width": W, "height": H, "in_bytes": size}
for filt in (5, 6):
    rec1 = records(1, W, H, filt)
    cap1 = np.array([z.png_bound(rec1)[0]], dtype=np.uint64)
    out = torch.zeros(int(cap1[0]), dtype=torch.uint8, device="cuda")
    n = [0]

    def write():
        _, _, out_len, status = z.png_encode_tensor(t, one[0], one[1], rec1, out=out, off=one[0], cap=cap1)
        assert status == [0]
        n[0] = out_len[0]

    def read():
        _, _, _, status, _ = z.png_decode_tensor(out, one[0], np.array(n, dtype=np.uint64), out=back, off=one[0], cap=one[1])
        assert status == [0]

    tw = timed(write, max(3, REPS // 3))
    read()
    assert bool((back == t).all()), "the single image does not decode to itself"
    tr = timed(read, max(3, REPS // 3))
    z.set_profiling(True)
    read()
    unf = {k: round(ms, 4) for k, ms, _ in z.last_kernel_times()}.get("k_png_unfilter")
    z.set_profiling(False)
    res["single"]["filter_%d" % filt] = {"file_bytes": int(n[0]), "encode_ms": median(tw), "decode_ms": median(tr), "unfilter_ms": unf}
    del out
res["single"]["decode_6_over_5"] = round(res["single"]["filter_6"]["decode_ms"] / res["single"]["filter_5"]["decode_ms"], 2)
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "pngwrite_bench.json"), "w") as f:
    f.write(line + "\n")
