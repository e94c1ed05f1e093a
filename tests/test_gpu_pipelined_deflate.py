"""The pipelined host deflate (deflate_host_pipelined: every zes_deflate of PIPE_MIN = 48 MiB and more) at its seams, and the
launches of the one-buffer deflate drivers.

The pipelined deflate has no piece-size switch: a piece is 256 blocks (32 MiB), so the smallest shapes that reach a seam
are tens of MiB.  Inputs are the library's own generators'.  That the pipelined path ran is shown by its own trace
(ZES_PIPE_DBG=1, five stamps per piece) in a child process.

The launches (tests/_host_driver_cases.py against tests/golden/host_driver_launches.json) were recorded from the commit in
front of the drivers' fold into deflate_one and the host conveyor (NOTES.md says which): status, the oracle's bytes, and
the launch count of every profiled kernel, each case twice in a row with the second record equal to the first.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _host_driver_cases as K
import _range_cases as rc
from test_gpu_pipelined_seams import GUARD, NOSPACE, PIPE_VARS, POISON, ROOT, inflate_into, pipe_env, same

pytestmark = pytest.mark.gpu

BLOCK = K.BLOCK
PIPE_PIECE, PIPE_MIN = K.PIPE_PIECE, K.PIPE_MIN

SEAMS = {  # name: (kind, seed, bytes)
    "pipe_min": ("xorshift", 811, PIPE_MIN),                    # the first pipelined size: pieces of 32 + 16 MiB
    "two_bytes_last": ("xorshift", 812, 2 * PIPE_PIECE + 2),    # three pieces, the last one two bytes; upload 2 carries no bytes
    "lowent_short_windows": ("lowent4k", 813, 2 * PIPE_PIECE + BLOCK + 2),  # compressed windows of ~1 MiB a piece
}


def deflate_into(z, a, cap):
    """zes_deflate into a poisoned buffer of cap + GUARD bytes -> (rc, out_len, buffer)"""
    buf = np.full(cap + GUARD, POISON, dtype=np.uint8)
    n = C.c_uint64()
    rcode = z.lib().zes_deflate(a.ctypes.data, a.size, buf.ctypes.data, cap, C.byref(n))
    return rcode, n.value, buf


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_sizes_at_the_seams(z, gpu, name):
    kind, seed, n = SEAMS[name]
    a = z.gen(kind, seed, n)
    bound = z.deflate_bound(n)
    with pipe_env():
        rcode, got, buf = deflate_into(z, a, bound)
    assert rcode == 0 and 6 < got <= bound and bool((buf[bound:] == POISON).all())
    stream = buf[:got].copy()
    with pipe_env(off=True):
        rcode, got1, buf1 = deflate_into(z, a, bound)
    assert rcode == 0 and got1 == got and same(buf1[:got1], stream), name
    assert bool((buf1[bound:] == POISON).all())
    assert int.from_bytes(stream[-4:].tobytes(), "big") == zlib.adler32(a.tobytes())
    with pipe_env():
        # a capacity of exactly the result (below the bound: counted first, one copy at the end)
        rcode, got2, buf2 = deflate_into(z, a, got)
        assert rcode == 0 and got2 == got and same(buf2[:got], stream) and bool((buf2[got:] == POISON).all()), name
        # one byte short: the exact size, and nothing behind the capacity
        rcode, got3, buf3 = deflate_into(z, a, got - 1)
        assert rcode == NOSPACE and got3 == got and bool((buf3[got - 1:] == POISON).all()), name
        # and back
        rcode, back_len, back = inflate_into(z, stream, n)
        assert rcode == 0 and back_len == n and same(back[:n], a) and bool((back[n:] == POISON).all()), name


CHILD = r"""
import ctypes as C, os, sys
import numpy as np
L = C.CDLL(sys.argv[1])
L.zes_deflate.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
L.zes_deflate_bound.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
L.zes_gen.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
n_long, n_short = int(sys.argv[2]), int(sys.argv[3])
a = np.empty(n_long, dtype=np.uint8)
assert L.zes_gen(a.ctypes.data, n_long, 0, 821) == 0
cap = C.c_uint64()
L.zes_deflate_bound(n_long, C.byref(cap))
out = np.zeros(cap.value, dtype=np.uint8)
got = C.c_uint64()
assert L.zes_init(0) == 0
for mark, n, off in (("pipelined", n_long, False), ("one-pass", n_long, True), ("below", n_short, False)):
    sys.stderr.write("mark: %s\n" % mark)
    sys.stderr.flush()
    os.environ.pop("ZES_NO_PIPELINE", None)
    if off:
        os.environ["ZES_NO_PIPELINE"] = "1"
    rcode = L.zes_deflate(a.ctypes.data, n, out.ctypes.data, cap.value, C.byref(got))
    sys.stderr.write("done: %d %d %d\n" % (rcode, got.value, int(np.bitwise_xor.reduce(out[:got.value]))))
    sys.stderr.flush()
L.zes_shutdown()
"""


def test_the_pipelined_path_runs(z, gpu):
    """One child process, ZES_PIPE_DBG=1: the 2 * PIPE_PIECE + 2 call stamps `launched` and `up done` for pieces 0, 1, 2; the
    same call under ZES_NO_PIPELINE=1 and a call of PIPE_MIN - 1 bytes stamp nothing."""
    n_long, n_short = 2 * PIPE_PIECE + 2, PIPE_MIN - 1
    env = {k: v for k, v in os.environ.items() if k not in PIPE_VARS}
    env.update(ZES_PIPE_DBG="1")
    lib = os.path.abspath(os.environ.get("ZES_LIB") or os.path.join(ROOT, "zlib.es_amd", "libzes_hip.so"))
    p = subprocess.run([sys.executable, "-c", CHILD, lib, str(n_long), str(n_short)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stderr.splitlines() if ln.startswith(("mark:", "done:")) or ln.lstrip().startswith("pipe ")]
    at1, at2 = lines.index("mark: one-pass"), lines.index("mark: below")
    first, second, third = lines[:at1], lines[at1:at2], lines[at2:]
    assert first[-1].startswith("done: 0 ") and second[-1] == first[-1] and third[-1].startswith("done: 0 "), lines
    stamps = [ln.split() for ln in first if ln.lstrip().startswith("pipe ")]  # pipe <what...> <k> <ms> ms
    pieces = lambda what: sorted(int(w[-3]) for w in stamps if " ".join(w[1:-3]) == what)
    assert pieces("launched") == [0, 1, 2] and pieces("up done") == [0, 1, 2], lines
    assert pieces("kernels done") == [0, 1, 2] and pieces("all down") == [3] and pieces("down issued"), lines
    assert not [ln for ln in second + third if ln.lstrip().startswith("pipe ")], lines


def test_state_left_behind(z, oracle, gpu):
    """On one context, twice round: a pipelined deflate, a one-pass host deflate, a device deflate and a block range, a
    pipelined inflate, the pipelined deflate again.  The upload events, the page-locked result slot (read directly and
    deferred) and the side threads (shared by both pipelines) must not carry anything over."""
    import torch

    kind, seed, n = SEAMS["pipe_min"]
    a = z.gen(kind, seed, n)
    small = z.gen("itext", 822, 300000)
    want_small = oracle.deflate(small)
    b = rc.deflate_input(z, "lowent4k")
    want_b = oracle.deflate(b)
    t = torch.from_numpy(b).to(gpu)
    lo, hi = BLOCK, 2 * BLOCK
    want_p, want_bits = oracle.deflate_range(b, lo, hi - lo, False)
    first = None
    for _ in range(2):
        with pipe_env():
            stream = z.deflate(a)
            if first is None:
                first = stream.copy()
                assert int.from_bytes(first[-4:].tobytes(), "big") == zlib.adler32(a.tobytes())
            assert same(stream, first)
            assert same(z.deflate(small), want_small)
            assert same(z.deflate_tensor(t).cpu().numpy(), want_b)
            p, bits, ad = z.deflate_range_tensor(t, lo, hi, final=False)
            assert bits == want_bits and same(p.cpu().numpy(), want_p) and ad == oracle.adler32(b[lo:hi])
            rcode, got, buf = inflate_into(z, first, n)
            assert rcode == 0 and got == n and same(buf[:n], a) and z.last_inflate_tier() == 1
            assert same(z.deflate(a), first)


@pytest.fixture(scope="module")
def golden():
    with open(K.GOLDEN) as f:
        return json.load(f)


def test_golden_file_has_every_case(golden):
    assert sorted(golden) == sorted(K.CASES)


@pytest.mark.parametrize("name", K.CASES)
def test_launches(z, gpu, golden, name):
    first = K.run_case(z, gpu, name)
    second = K.run_case(z, gpu, name)
    print(name, first)
    # whatever was recorded: the call succeeded and gave the oracle's bytes
    assert first["status"] == 0 and first["bytes_equal"] and first.get("adler_equal", True), first
    assert first["launches"], first
    assert first == golden[name], (name, first, golden[name])
    assert second == first, (name, "second run", second, first)
