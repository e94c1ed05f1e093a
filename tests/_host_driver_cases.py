"""The one-buffer drivers' launches: a case per entry point that encodes one buffer (host deflate, raw deflate, a block
range, the join of two ranges, gzip, the pipelined host deflate), and a runner that records what a call came to — status,
the result against the oracle, and the launches per profiled name (zes_last_kernel_times).
tests/test_gpu_pipelined_deflate.py compares the records with tests/golden/host_driver_launches.json.

    python -m tests._host_driver_cases      writes tests/golden/host_driver_launches.json (ZES_LIB selects the library)

The pipelined call collects its kernels' times piece by piece: its report is its last piece's (two bytes of input).
"""
import functools
import json
import os
import struct
import sys
import zlib as pz

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_driver_launches.json")
if os.path.join(ROOT, "tests") not in sys.path:  # (python -m tests._host_driver_cases)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle  # noqa: E402

BLOCK = 131072
PIPE_PIECE = 256 * BLOCK  # zes_api.hip
PIPE_MIN = PIPE_PIECE + PIPE_PIECE // 2
SMALL = 300000

CASES = ["deflate", "deflate_raw", "deflate_range_tensor final", "deflate_range_tensor not final", "deflate_join_tensors", "gzip",
         "deflate pipelined"]


def _pkg():
    import torch  # noqa: F401  (before the library: tests/conftest.py says why)

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    return ge.load()


@functools.lru_cache(maxsize=None)
def small():
    """(300 000 bytes of itext, oracle.deflate of them, oracle.deflate_raw of them)."""
    a = _pkg().gen("itext", 801, SMALL)
    return a, _oracle.deflate(a).tobytes(), _oracle.deflate_raw(a).tobytes()


@functools.lru_cache(maxsize=None)
def long_input():
    """(2 * PIPE_PIECE + 2 bytes of lowent4k — three pieces, the last one two bytes —, oracle.deflate of them)."""
    a = _pkg().gen("lowent4k", 802, 2 * PIPE_PIECE + 2)
    return a, _oracle.deflate(a).tobytes()


def _call(z, fn):
    try:
        return 0, fn()
    except z.ZlibEsError as e:
        return e.code, None


def _record(z, status, **what):
    rec = {"status": status, "launches": {name: n for name, _, n in z.last_kernel_times()}}
    rec.update(what)
    return rec


def _range(z, gpu, lo, hi):
    import torch

    a = small()[0]
    t = torch.from_numpy(a).to(gpu)
    status, got = _call(z, lambda: z.deflate_range_tensor(t, lo, hi, final=(hi == a.size)))
    rec = _record(z, status)
    want, want_bits = _oracle.deflate_range(a, lo, hi - lo, hi == a.size)
    p, bits, ad = got
    rec.update(bits=bits, bytes_equal=bits == want_bits and p.cpu().numpy().tobytes() == want.tobytes(),
               adler_equal=ad == pz.adler32(a[lo:hi].tobytes()))
    return rec


def _join(z, gpu):
    import torch

    a, want, _ = small()
    t = torch.from_numpy(a).to(gpu)
    cuts = (0, 2 * BLOCK, a.size)
    parts = [z.deflate_range_tensor(t, lo, hi, final=(hi == a.size)) for lo, hi in zip(cuts, cuts[1:])]
    pieces = [p.clone() for p, _, _ in parts]
    status, got = _call(z, lambda: z.deflate_join_tensors(pieces, [b for _, b, _ in parts], [ad for _, _, ad in parts],
                                                          [hi - lo for lo, hi in zip(cuts, cuts[1:])]))
    return _record(z, status, out_len=int(got.numel()), bytes_equal=got.cpu().numpy().tobytes() == want)


def run_case(z, gpu, name):
    """A case's record; profiling is on for the call and off again behind it."""
    a, want, want_raw = small()
    z.set_profiling(True)
    try:
        if name == "deflate":
            status, got = _call(z, lambda: z.deflate(a))
            return _record(z, status, out_len=int(got.size), bytes_equal=got.tobytes() == want)
        if name == "deflate_raw":
            status, got = _call(z, lambda: z.deflate_raw(a))
            return _record(z, status, out_len=int(got.size), bytes_equal=got.tobytes() == want_raw)
        if name == "deflate_range_tensor final":
            return _range(z, gpu, 2 * BLOCK, a.size)
        if name == "deflate_range_tensor not final":
            return _range(z, gpu, 0, 2 * BLOCK)
        if name == "deflate_join_tensors":
            return _join(z, gpu)
        if name == "gzip":
            status, got = _call(z, lambda: z.gzip(a))
            expect = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF]) + want_raw + struct.pack("<II", pz.crc32(a.tobytes()), a.size)
            return _record(z, status, out_len=int(got.size), bytes_equal=got.tobytes() == expect)
        if name == "deflate pipelined":
            big, want_big = long_input()
            assert "ZES_NO_PIPELINE" not in os.environ
            status, got = _call(z, lambda: z.deflate(big))
            return _record(z, status, out_len=int(got.size), bytes_equal=got.tobytes() == want_big)
        raise KeyError(name)
    finally:
        z.set_profiling(False)


def main():
    import torch

    z = _pkg()
    assert torch.cuda.is_available(), "the launches are recorded on a GPU"
    z.init(0)
    gpu = torch.device("cuda:0")
    rec = {}
    for name in CASES:
        first, second = run_case(z, gpu, name), run_case(z, gpu, name)
        assert first == second, "%s: the second run differs from the first: %r / %r" % (name, first, second)
        rec[name] = first
        print(name, first, file=sys.stderr)
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
