"""One large TIFF image read on the device, timed (not a pytest); prints one JSON line and writes it to
profiles/tiff_speed.json.

    python tools/tiff_speed.py [reps]

The image: 4096 x 4096 RGBA8 whose bytes are zes_gen's text-like content, written by tests/_tiff.py's writer as 256 tiles of
256 x 256, Compression 8 (CPython's zlib, level 6), Predictor 2, the file in device memory.  After a warm-up at the same shape,
the median wall time of `reps` calls (each ends in a synchronise), the calls of the legs alternating in one loop:
whole      zes_tiff_read_dev on the whole image (the pixels are compared with the input first)
rect       a 512 x 512 rectangle that straddles four tiles
loop       the same 256 tile streams through a loop of zes_inflate_dev, one call per tile: what the library offered before
           (it stops at the predicted tile bytes: no predictor, no placing)
png6/png5  the same pixels as a PNG file through zes_pngpix_dev, the file written by zes_pngwrite with the adaptive filter (6,
           rows chain from top to bottom: one wave unfilters the image) and with the banded default (5, restart rows every 64)
and, from one profiled call each (zes_last_kernel_times), the per-kernel split; k_tiff_place's time against the bytes it
moves (the decoded tiles read, the image written) beside a device-to-device copy of the image (read + written) timed here.
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
import _tiff as T  # noqa: E402

z = ge.load()
z.init(0)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
W = H = 4096
TILE = 256


def median(ts):
    return round(sorted(ts)[len(ts) // 2], 3)


def kernels_of(call):
    z.set_profiling(True)
    call()
    k = [[name, round(ms, 4), launches] for name, ms, launches in z.last_kernel_times()]
    z.set_profiling(False)
    return k


px = z.gen("itext", 77, W * H * 4).reshape(H, W, 4)
pg = T.page(px, ("tiles", TILE, TILE), 8, 2)
streams = [zlib.compress(raw, 6) for raw in T.segments_of(pg, "II")]
f = T.write([T.page(px, ("tiles", TILE, TILE), 8, 2, compress=lambda k, raw: streams[k])], "II")
print("file made: %d bytes, %d tiles" % (len(f), len(streams)), file=sys.stderr, flush=True)
t = torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda()
index = z.tiff_index_tensor(t)
out = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
small = torch.zeros(512 * 512 * 4, dtype=torch.uint8, device="cuda")
RECT = (TILE, 2 * TILE, 512, 512)  # over the corner that four tiles share
assert len(T.touched(T.rule(f)[0], RECT)) == 4


def whole():
    assert z.tiff_read_tensor(t, index, None, out=out)[2] == 0


def rect():
    assert z.tiff_read_tensor(t, index, RECT, out=small)[2] == 0


# the tile streams once more, each at a 16-byte boundary, for the loop of single calls
soff = np.cumsum([0] + [(len(s) + 15) // 16 * 16 + 64 for s in streams])
sbuf = np.zeros(int(soff[-1]), dtype=np.uint8)
for o, s in zip(soff, streams):
    sbuf[int(o):int(o) + len(s)] = np.frombuffer(s, dtype=np.uint8)
st = torch.from_numpy(sbuf).cuda()
tiles_out = torch.zeros(W * H * 4 + 64, dtype=torch.uint8, device="cuda")
E = TILE * TILE * 4


def loop():
    for k, s in enumerate(streams):
        got = z.inflate_tensor(st[int(soff[k]):int(soff[k]) + len(s)], tiles_out[k * E:(k + 1) * E])
        assert got.numel() == E


whole()
host = out.cpu().numpy().reshape(H, W, 4)
assert (host == px).all(), "the pixels differ from the input"
rect()
x, y, w, h = RECT
assert (small.cpu().numpy().reshape(h, w, 4) == px[y:y + h, x:x + w]).all(), "the rectangle differs from the input"
del host

# the same pixels as PNG files
rows = px.reshape(H, W * 4)
pngs = {}
for name, flt in (("png6", z.PNG_FILTER_ADAPTIVE), ("png5", z.PNG_FILTER_BANDED)):
    blob = z.png_encode(rows, width=W, colour=6, depth=8, filter=flt)
    pngs[name] = (torch.from_numpy(np.ascontiguousarray(blob)).cuda(), len(blob))
    print(name, "written: %d bytes" % len(blob), file=sys.stderr, flush=True)
pix = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")


def png(name):
    d, n = pngs[name]
    status = z.png_pixels_tensor(d, [0], [n], out=pix, off=[0], cap=[W * H * 4])[3]
    assert not any(status)


png("png6")
assert (pix.cpu().numpy().reshape(H, W, 4) == px).all(), "the PNG's pixels differ from the input"

legs = {"whole": whole, "rect": rect, "loop": loop, "png6": lambda: png("png6"), "png5": lambda: png("png5")}
for fn in legs.values():  # warm-up at the same shapes
    fn()
times = {k: [] for k in legs}
for _ in range(REPS):
    for k, fn in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) * 1e3)

# a device-to-device copy of the image
dst = torch.empty_like(out)
copies = []
for _ in range(REPS + 2):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    dst.copy_(out)
    b.record()
    torch.cuda.synchronize()
    copies.append(a.elapsed_time(b))
copy_ms = median(copies[2:])

kern = {k: kernels_of(fn) for k, fn in legs.items() if k != "loop"}
place_ms = [ms for name, ms, _ in kern["whole"] if name == "k_tiff_place"][0]
moved = 2 * W * H * 4
res = {"reps": REPS, "width": W, "height": H, "tile": TILE, "file_bytes": len(f), "png6_bytes": pngs["png6"][1], "png5_bytes": pngs["png5"][1],
       "rect": list(RECT), "rect_tiles": len(T.touched(T.rule(f)[0], RECT)), "tier": z.last_inflate_tier()}
for k in legs:
    res[k + "_ms"] = median(times[k])
    res[k + "_ms_min_max"] = [round(min(times[k]), 3), round(max(times[k]), 3)]
res["whole_gib_per_s"] = round(W * H * 4 / (res["whole_ms"] / 1e3) / 2**30, 2)
res["kernels"] = kern
res["place_ms"] = round(place_ms, 4)
res["place_bytes_moved"] = moved
res["place_tb_per_s"] = round(moved / (place_ms / 1e3) / 1e12, 3)
res["copy_ms"] = copy_ms
res["copy_tb_per_s"] = round(moved / (copy_ms / 1e3) / 1e12, 3)
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "tiff_speed.json"), "w") as fh:
    fh.write(line + "\n")
