"""One large TIFF image written on the device, timed (not a pytest); prints one JSON line and writes it to
profiles/tiffwrite_speed.json.

    python tools/tiffwrite_speed.py [reps]

The image: 4096 x 4096 RGBA8 whose bytes are zes_gen's text-like content, in device memory; written as 256 tiles of 256 x 256,
Compression 8, Predictor 2.  After a warm-up at the same shape, the median wall time of `reps` calls (each ends in a
synchronise), the calls of the legs alternating in one loop:
write      zes_tiffwrite_dev on the image (the file is read back by zes_tiff_read_dev and compared with the input first)
loop       the tiles, cut and differenced beforehand (tests/_tiff.py's segments_of), through a loop of zes_deflate_dev, one
           call per tile: what the library offered before
batch      zes_deflate_batch_dev alone over the same cut tiles: the encoder's share of the write call
and, from one profiled write call (zes_last_kernel_times), the per-kernel split, k_tiff_cut's and k_tiff_pack's share of the
call's kernel time, and k_tiff_cut's time against the bytes it moves (the image read, the slots written) beside a
device-to-device copy of the image (read + written) timed here.
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
import _tiff as T  # noqa: E402

z = ge.load()
z.init(0)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
W = H = 4096
TILE = 256
E = TILE * TILE * 4


def median(ts):
    return round(sorted(ts)[len(ts) // 2], 3)


px = z.gen("itext", 77, W * H * 4).reshape(H, W, 4)
rec = z.tiff_image(W, H, 8, 4, tile=(TILE, TILE), compression=8, predictor=2)
img = torch.from_numpy(px.reshape(-1).copy()).cuda()
bound, nseg = z.tiff_bound(rec)
room = torch.zeros(bound, dtype=torch.uint8, device="cuda")
state = {}


def write():
    state["file"] = z.tiff_write_tensor(img, rec, out=room)


# the cut tiles, each at a 16-byte boundary, for the two encoder-only legs
tiles = T.segments_of(T.page(px, ("tiles", TILE, TILE), 8, 2), "II")
assert len(tiles) == nseg == 256 and all(len(t) == E for t in tiles)
cut = torch.from_numpy(np.frombuffer(b"".join(tiles), dtype=np.uint8).copy()).cuda()
slot = (z.deflate_bound(E) + 15) // 16 * 16
slots = torch.zeros(slot * nseg + 64, dtype=torch.uint8, device="cuda")
in_off, in_len = [k * E for k in range(nseg)], [E] * nseg
out_off, out_cap = [k * slot for k in range(nseg)], [slot] * nseg


def loop():
    for k in range(nseg):
        z.deflate_tensor(cut[k * E:(k + 1) * E], out=slots[k * slot:(k + 1) * slot])


def batch():
    out_len, status = z.deflate_batch_tensor(cut, in_off, in_len, slots, out_off, out_cap)
    assert not any(status)


write()
f, seg_off, seg_len = state["file"]
back, st, rc = z.tiff_read_tensor(f, z.tiff_index_tensor(f))
assert rc == 0 and (back.cpu().numpy().reshape(H, W, 4) == px).all(), "the written file does not read back to the input"
file_bytes = int(f.numel())
print("file written: %d bytes of a bound of %d" % (file_bytes, bound), file=sys.stderr, flush=True)

legs = {"write": write, "loop": loop, "batch": batch}
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
dst = torch.empty_like(img)
copies = []
for _ in range(REPS + 2):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    dst.copy_(img)
    b.record()
    torch.cuda.synchronize()
    copies.append(a.elapsed_time(b))
copy_ms = median(copies[2:])

z.set_profiling(True)
write()
kern = [[name, round(ms, 4), launches] for name, ms, launches in z.last_kernel_times()]
z.set_profiling(False)
total_ms = sum(ms for _, ms, _ in kern)
cut_ms = [ms for name, ms, _ in kern if name == "k_tiff_cut"][0]
pack_ms = [ms for name, ms, _ in kern if name == "k_tiff_pack"][0]
moved = 2 * W * H * 4
res = {"reps": REPS, "width": W, "height": H, "tile": TILE, "segments": nseg, "file_bytes": file_bytes, "bound": bound}
for k in legs:
    res[k + "_ms"] = median(times[k])
    res[k + "_ms_min_max"] = [round(min(times[k]), 3), round(max(times[k]), 3)]
res["write_gib_per_s"] = round(W * H * 4 / (res["write_ms"] / 1e3) / 2**30, 2)
res["write_over_loop"] = round(res["write_ms"] / res["loop_ms"], 4)
res["write_over_batch"] = round(res["write_ms"] / res["batch_ms"], 4)
res["kernels"] = kern
res["kernel_ms"] = round(total_ms, 4)
res["cut_ms"] = round(cut_ms, 4)
res["pack_ms"] = round(pack_ms, 4)
res["cut_share"] = round(cut_ms / total_ms, 4)
res["pack_share"] = round(pack_ms / total_ms, 4)
res["cut_bytes_moved"] = moved
res["cut_tb_per_s"] = round(moved / (cut_ms / 1e3) / 1e12, 3)
res["copy_ms"] = copy_ms
res["copy_tb_per_s"] = round(moved / (copy_ms / 1e3) / 1e12, 3)
line = json.dumps(res)
print(line)
with open(os.path.join(ROOT, "profiles", "tiffwrite_speed.json"), "w") as fh:
    fh.write(line + "\n")
