"""bench.py --dump-outputs: what the timed path computed goes to DIR/<name>.npy as float32 / float64 — streams whole up to
DUMP_SAMPLE bytes, longer ones as the same seeded sample on every run, each with its length and CRC-32 over all of it —
and within 64 MB for the two 64 MiB streams of the flagship step."""
import os
import sys
import zlib

import numpy as np

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_short_streams_and_lengths_are_written_whole(tmp_path):
    a = np.arange(1000, dtype=np.uint32).astype(np.uint8)
    written = bench.dump_outputs(str(tmp_path), {"deflate": a, "deflate_lengths": [600, 400]})
    got = _load(tmp_path)
    assert set(got) == {"deflate", "deflate_length", "deflate_crc32", "deflate_lengths"}
    assert got["deflate"].dtype == np.float32 and (got["deflate"] == a).all()
    assert got["deflate_length"].dtype == np.float64 and list(got["deflate_length"]) == [1000]
    assert got["deflate_crc32"].dtype == np.float64 and got["deflate_crc32"][0] == zlib.crc32(a.tobytes())
    assert got["deflate_lengths"].dtype == np.float64 and list(got["deflate_lengths"]) == [600, 400]
    assert written["deflate.npy"] == 4000


def test_long_streams_are_a_fixed_seeded_sample_within_64_mb(tmp_path):
    n = 64 << 20
    rng = np.random.default_rng(7)
    big = [rng.integers(0, 256, n + k, dtype=np.uint8) for k in (0, 1234)]
    written = bench.dump_outputs(str(tmp_path / "a"), {"deflate": big[1], "inflate": big[0]})
    bench.dump_outputs(str(tmp_path / "b"), {"deflate": big[1], "inflate": big[0]})
    assert sum(written.values()) <= 64 * 10**6
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(b) and all((a[k] == b[k]).all() for k in a)
    for name, src in (("deflate", big[1]), ("inflate", big[0])):
        idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, src.size, bench.DUMP_SAMPLE))
        assert a[name].dtype == np.float32 and a[name].size == bench.DUMP_SAMPLE
        assert (a[name] == src[idx]).all()
        assert a[name + "_length"][0] == src.size and a[name + "_crc32"][0] == zlib.crc32(src)
