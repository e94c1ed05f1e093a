"""The host-pointer batch forms, timed (not a pytest): the calls that take the caller's memory up, run the device batch and
bring the results down.  Prints one JSON line (and writes it to the path behind --out).

    python tools/gpu_host_forms_bench.py [reps] [--out FILE]

256 buffers of 64 KiB of itext from zes_gen seeds, and 256 images of 128 x 128 RGBA (a gradient plus noise, seeded); every
input is made once, every result is compared with the inputs before anything is timed, and each figure is the median wall
time in ms of `reps` calls through the package after a warm-up:
deflate_batch     zes_deflate_batch          inflate_batch    zes_inflate_batch_alloc of deflate_batch's streams
zip_write         zes_zipwrite               zip_read         zes_zip_read_alloc of zip_write's archive
png_encode_batch  zes_pngwrite               png_decode_batch zes_png_decode_alloc of png_encode_batch's files
The other tools time the device forms (and tools/gpu_zip_bench.py zes_zip_read_alloc on larger archives).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before the library: tests/conftest.py says why)

import __graft_entry__ as ge  # noqa: E402

z = ge.load()
z.init(0)
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
COUNT, LEN, SIDE = 256, 64 << 10, 128


def median_ms(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 3)


def picture(seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    a = ((xx * (1 + seed % 3) + yy * 2)[:, :, None] + np.arange(4) * 50 + rs.randint(0, 8, size=(SIDE, SIDE, 4))).astype(np.uint8)
    return a.reshape(SIDE, SIDE * 4)


plain = [z.gen("itext", 8000 + k, LEN) for k in range(COUNT)]
entries = [(b"text/%04d.bin" % k, p) for k, p in enumerate(plain)]
pics = [dict(rows=picture(300 + k), width=SIDE, colour=6, depth=8) for k in range(COUNT)]

streams = z.deflate_batch(plain)
assert all((a == b).all() for a, b in zip(z.inflate_batch(streams), plain))
archive, index = z.zip_write(entries)
assert all((a == b).all() for a, b in zip(z.zip_read(archive, index), plain))
files = z.png_encode_batch(pics)
assert all(rows.tobytes() == p["rows"].tobytes() for (_, rows), p in zip(z.png_decode_batch(files), pics))

res = {"reps": REPS, "buffers": COUNT, "buffer_bytes": LEN, "images": COUNT, "image": "%d x %d RGBA 8" % (SIDE, SIDE),
       "deflate_batch_ms": median_ms(lambda: z.deflate_batch(plain)), "inflate_batch_ms": median_ms(lambda: z.inflate_batch(streams)),
       "zip_write_ms": median_ms(lambda: z.zip_write(entries)), "zip_read_ms": median_ms(lambda: z.zip_read(archive, index)),
       "png_encode_batch_ms": median_ms(lambda: z.png_encode_batch(pics)), "png_decode_batch_ms": median_ms(lambda: z.png_decode_batch(files))}
line = json.dumps(res)
print(line)
if OUT:
    with open(OUT, "w") as f:
        f.write(line + "\n")
