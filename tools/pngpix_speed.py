"""PNG files to RGBA8 pixels in one batch, timed (not a pytest); prints one JSON line and writes it to
profiles/pngpix_speed.json.

    python tools/pngpix_speed.py [reps]

Four workloads of 1024 images of 256 x 256 (32 different ones, 32 times each), written with tests/_png.py's chunk writer from
seeded pixels (a gradient plus noise) and CPython's zlib at level 6:
rgba8      8-bit RGBA, every row with the filter type that the minimum-sum-of-absolute-differences heuristic picks (the batch
           of tools/png_speed.py)
palette8   8-bit palette indices with a 256-entry PLTE and a 256-byte tRNS, filter None
grey1      1-bit grey, filter None
rgba16     16-bit RGBA, the heuristic's filters
With the files in device memory, per workload: the pixels of zes_pngpix_dev are compared with the numpy rule of
tests/_pngpix.py first; then the median wall time of 10 calls (each ends in a synchronise) after a warm-up at the same shape,
of zes_pngpix_dev and of zes_png_decode_dev on the same files, the two alternating in one loop; the per-kernel split of one
profiled call of each from zes_last_kernel_times; and k_png_expand's time against its traffic — the scanline bytes read plus
4 * width * height bytes written per image — at the HBM rate a streaming kernel reaches on this part (6.3 TB/s).
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
import _pngpix  # noqa: E402

z = ge.load()
z.init(0)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
W = H = 256
COUNT, DIFFERENT = 1024, 32
HBM_BYTES_PER_S = 6.3e12  # what a streaming kernel reaches (a float4 copy): the yardstick for k_png_expand's traffic


def picture(seed, channels, bits):
    """height x (width * channels) samples: a gradient plus noise, in 0 .. 2^bits - 1."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    a = (xx * (1 + seed % 3) + yy * 2)[:, :, None] + np.arange(channels) * 50 + rs.randint(0, 8, size=(H, W, channels))
    if bits == 16:
        a = a * 37 + rs.randint(0, 256, size=(H, W, channels))
    return (a & ((1 << bits) - 1)).reshape(H, W * channels)


def adaptive(rows, bpp):
    """The filtered scanlines, every row by the type with the least sum of absolute (signed) filtered bytes."""
    x = rows.astype(np.int32)
    b = np.vstack([np.zeros((1, x.shape[1]), dtype=np.int32), x[:-1]])
    a = np.hstack([np.zeros((x.shape[0], bpp), dtype=np.int32), x[:, :-bpp]])
    c = np.hstack([np.zeros((x.shape[0], bpp), dtype=np.int32), b[:, :-bpp]])
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = [((x - pred) & 255).astype(np.uint8) for pred in (0, a, b, (a + b) >> 1, paeth)]
    pick = np.stack([np.abs(f.astype(np.int8).astype(np.int32)).sum(axis=1) for f in cand]).argmin(axis=0)
    out = np.empty((x.shape[0], 1 + x.shape[1]), dtype=np.uint8)
    out[:, 0] = pick
    for t in range(5):
        out[pick == t, 1:] = cand[t][pick == t]
    return out


def unfiltered(rows):
    return np.hstack([np.zeros((rows.shape[0], 1), dtype=np.uint8), rows])


def png(filtered, colour, depth, chunks=()):
    zs = zlib.compress(filtered.tobytes(), 6)
    return (_png.SIGNATURE + _png.ihdr(W, H, colour, depth) + b"".join(chunks) + b"".join(_png.chunk(b"IDAT", zs[k:k + 65536]) for k in range(0, len(zs), 65536)) +
            _png.chunk(b"IEND"))


def make(kind, seed):
    """(file, scanline bytes, colour, depth, plte, trns) of one image."""
    rs = np.random.RandomState(9000 + seed)
    if kind == "rgba8":
        rows = picture(seed, 4, 8).astype(np.uint8)
        return png(adaptive(rows, 4), 6, 8), rows.tobytes(), 6, 8, b"", b""
    if kind == "rgba16":
        s = picture(seed, 4, 16)
        rows = np.stack([s >> 8, s & 255], axis=2).astype(np.uint8).reshape(H, W * 8)
        return png(adaptive(rows, 8), 6, 16), rows.tobytes(), 6, 16, b"", b""
    if kind == "palette8":
        rows = picture(seed, 1, 8).astype(np.uint8)
        plte, trns = rs.randint(0, 256, size=768, dtype=np.uint8).tobytes(), rs.randint(0, 256, size=256, dtype=np.uint8).tobytes()
        return png(unfiltered(rows), 3, 8, [_png.chunk(b"PLTE", plte), _png.chunk(b"tRNS", trns)]), rows.tobytes(), 3, 8, plte, trns
    assert kind == "grey1"
    rows = np.packbits((picture(seed, 1, 8) >> 3) & 1, axis=1).astype(np.uint8)
    return png(unfiltered(rows), 0, 1), rows.tobytes(), 0, 1, b"", b""


def median(ts):
    return round(sorted(ts)[len(ts) // 2], 3)


def kernels_of(call):
    z.set_profiling(True)
    call()
    k = {name: [round(ms, 4), launches] for name, ms, launches in z.last_kernel_times()}
    z.set_profiling(False)
    return k


def workload(kind):
    made = [make(kind, 100 + k) for k in range(DIFFERENT)]
    print(kind, "files made", file=sys.stderr, flush=True)
    blobs = [made[k % DIFFERENT][0] for k in range(COUNT)]
    ioff = np.cumsum([0] + [len(b) + 3 for b in blobs])[:-1].astype(np.uint64)
    ilen = np.array([len(b) for b in blobs], dtype=np.uint64)
    flat = np.zeros(int(ioff[-1]) + len(blobs[-1]), dtype=np.uint8)
    for o, b in zip(ioff, blobs):
        flat[int(o):int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    t = torch.from_numpy(flat).cuda()
    lines = len(made[0][1])
    psize = W * H * 4
    poff, pcap = np.arange(COUNT, dtype=np.uint64) * np.uint64(psize), np.full(COUNT, psize, dtype=np.uint64)
    loff, lcap = np.arange(COUNT, dtype=np.uint64) * np.uint64(lines), np.full(COUNT, lines, dtype=np.uint64)
    pix = torch.zeros(COUNT * psize, dtype=torch.uint8, device="cuda")
    raw = torch.zeros(COUNT * lines, dtype=torch.uint8, device="cuda")

    def pixels():
        status = z.png_pixels_tensor(t, ioff, ilen, out=pix, off=poff, cap=pcap)[3]
        assert not any(status)

    def scanlines():
        status = z.png_decode_tensor(t, ioff, ilen, out=raw, off=loff, cap=lcap)[3]
        assert not any(status)

    # the bytes first
    pixels()
    host = pix.cpu().numpy().reshape(COUNT, psize)
    want = [_pngpix.rule(m[1], W, H, m[2], m[3], m[4], m[5]).reshape(-1) for m in made]
    assert all((host[k] == want[k % DIFFERENT]).all() for k in range(COUNT)), "%s: the pixels differ from the rule" % kind
    del host
    scanlines()  # warm-up of the other form at this shape
    tp, td = [], []
    for _ in range(REPS):  # the two forms in turn
        for fn, ts in ((pixels, tp), (scanlines, td)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    kp, kd = kernels_of(pixels), kernels_of(scanlines)
    share = lambda k, pred: round(sum(v[0] for name, v in k.items() if pred(name)), 4)
    total = share(kp, lambda n: True)
    expand_ms, unf_ms, inf_ms = kp["k_png_expand"][0], kp["k_png_unfilter"][0], share(kp, lambda n: n.startswith("k_inf"))
    traffic = COUNT * (lines + psize)
    floor_ms = traffic / HBM_BYTES_PER_S * 1e3
    return {"images": COUNT, "width": W, "height": H, "file_bytes": int(ilen.sum()), "scanline_bytes": COUNT * lines, "pixel_bytes": COUNT * psize,
            "tier": z.last_inflate_tier(), "pixels_ms": median(tp), "pixels_ms_min_max": [round(min(tp), 3), round(max(tp), 3)],
            "decode_ms": median(td), "decode_ms_min_max": [round(min(td), 3), round(max(td), 3)], "pixels_minus_decode_ms": round(median(tp) - median(td), 3),
            "kernels_pixels": kp, "kernels_decode": kd, "kernel_ms_total": total, "expand_ms": expand_ms, "unfilter_ms": unf_ms,
            "unfilter_ms_in_decode_call": kd["k_png_unfilter"][0], "inflate_kernels_ms": inf_ms,
            "expand_share_of_call": round(expand_ms / median(tp), 4), "unfilter_share_of_call": round(unf_ms / median(tp), 4),
            "inflate_share_of_call": round(inf_ms / median(tp), 4), "expand_over_unfilter": round(expand_ms / unf_ms, 3),
            "expand_traffic_bytes": traffic, "expand_traffic_floor_ms": round(floor_ms, 4), "expand_tb_per_s": round(traffic / (expand_ms / 1e3) / 1e12, 3),
            "expand_share_of_hbm_rate": round(floor_ms / expand_ms, 3)}


res = {"reps": REPS, "hbm_bytes_per_s": HBM_BYTES_PER_S}
for kind in ("rgba8", "palette8", "grey1", "rgba16"):
    res[kind] = workload(kind)
    torch.cuda.empty_cache()
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "pngpix_speed.json"), "w") as f:
    f.write(line + "\n")
