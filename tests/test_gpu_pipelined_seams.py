"""The pipelined host inflate (inflate_host_pipelined: every zes_inflate / zes_inflate_alloc of 8 MiB of stream and more)
with many small pieces: ZES_PIPE_PIECE_MB / ZES_PIPE_FIRST_MB, read per call, cut the smallest streams that enter the
path into nine and more pieces.  Valid streams, capacities, the allocating forms, damaged and truncated streams
(positions and oracle outcomes: tests/_range_cases.py), and what a call that ended mid-stream leaves behind.

That the pipelined path ran is shown by its own trace: the call does not record its launches for
zes_last_kernel_times, so a child process runs it with ZES_DEBUG_PIPE=1 and the test reads its "zes pipe:" line.
"""
import contextlib
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _range_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xC3
GUARD = 4096
NOSPACE = -16
PIPE_VARS = ("ZES_PIPE_PIECE_MB", "ZES_PIPE_FIRST_MB", "ZES_NO_PIPELINE")


@contextlib.contextmanager
def pipe_env(piece_mb=None, first_mb=None, off=False):
    """The three variables are read by every call: set around one."""
    want = {"ZES_PIPE_PIECE_MB": piece_mb, "ZES_PIPE_FIRST_MB": first_mb, "ZES_NO_PIPELINE": 1 if off else None}
    old = {k: os.environ.get(k) for k in PIPE_VARS}
    try:
        for k, v in want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def inputs(z, oracle, gpu):
    """name -> (plain bytes, oracle.deflate of them), made once."""
    out = {}
    for name, (kind, seed, n, c) in rc.PIPE_INPUTS.items():
        a = z.gen(kind, seed, n)
        comp = oracle.deflate(a)
        assert len(comp) == c and c >= 8 << 20
        out[name] = (a, comp)
    return out


def inflate_into(z, comp, cap):
    """zes_inflate into a poisoned buffer of cap + GUARD bytes -> (rc, out_len, buffer)"""
    buf = np.full(cap + GUARD, POISON, dtype=np.uint8)
    n = C.c_uint64()
    rcode = z.lib().zes_inflate(comp.ctypes.data, len(comp), buf.ctypes.data, cap, C.byref(n), 0)
    return rcode, n.value, buf


def inflate_alloc(z, comp, flags):
    """zes_inflate_alloc -> (rc, out_len, [(index, array) per allocator call])"""
    asked = []

    def alloc(_user, index, n):
        asked.append((int(index), np.full(max(int(n), 1), POISON, dtype=np.uint8)))
        return asked[-1][1].ctypes.data

    n = C.c_uint64()
    rcode = z.lib().zes_inflate_alloc(comp.ctypes.data, len(comp), z.ALLOC_FN(alloc), None, C.byref(n), flags)
    return rcode, n.value, asked


def same(got, want):
    return got.size == want.size and bool((got == want).all())


CHILD = r"""
import ctypes as C, os, sys
import numpy as np
L = C.CDLL(sys.argv[1])
L.zes_inflate.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32]
comp = np.fromfile(sys.argv[2], dtype=np.uint8)
n = int(sys.argv[3])
out = np.zeros(n, dtype=np.uint8)
got = C.c_uint64()
assert L.zes_init(0) == 0
for mark, off in (("pipelined", False), ("one-pass", True)):
    sys.stderr.write("mark: %s\n" % mark)
    sys.stderr.flush()
    if off:
        os.environ["ZES_NO_PIPELINE"] = "1"
    rcode = L.zes_inflate(comp.ctypes.data, comp.size, out.ctypes.data, n, C.byref(got), 0)
    sys.stderr.write("done: %d %d %d\n" % (rcode, got.value, int(np.bitwise_xor.reduce(out))))
    sys.stderr.flush()
L.zes_shutdown()
"""


@pytest.mark.parametrize("name,first_mb", (("xorshift9", 0), ("itext24", 1)))
def test_the_pipelined_path_runs(z, gpu, inputs, tmp_path, name, first_mb):
    """One child process, ZES_DEBUG_PIPE=1 and 1 MiB pieces: the pipelined call traces np >= 9 pieces and the whole output;
    the same call under ZES_NO_PIPELINE=1 traces nothing."""
    a, comp = inputs[name]
    path = tmp_path / "stream.bin"
    comp.tofile(str(path))
    env = {k: v for k, v in os.environ.items() if k not in PIPE_VARS}
    env.update(ZES_DEBUG_PIPE="1", ZES_PIPE_PIECE_MB="1", ZES_PIPE_FIRST_MB=str(first_mb))
    lib = os.path.join(ROOT, "zlib.es_amd", "libzes_hip.so")
    p = subprocess.run([sys.executable, "-c", CHILD, lib, str(path), str(len(a))], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stderr.splitlines() if ln.startswith(("mark:", "done:", "zes pipe:"))]
    at = lines.index("mark: one-pass")
    first, second = lines[:at], lines[at:]
    x = int(np.bitwise_xor.reduce(a))
    assert first[-1] == "done: 0 %d %d" % (len(a), x) and second[-1] == "done: 0 %d %d" % (len(a), x), lines
    loop = [ln for ln in first if ln.startswith("zes pipe: loop done")]
    assert len(loop) == 1, lines
    words = loop[0].replace(",", " ").split()
    np_, total = int(words[words.index("np") + 1]), int(words[words.index("total") + 1])
    assert np_ >= 9 and total == len(a), loop
    assert not [ln for ln in second if ln.startswith("zes pipe:")], lines


@pytest.mark.parametrize("name", ("xorshift9", "itext24"))
@pytest.mark.parametrize("first_mb", (0, 1))
@pytest.mark.parametrize("piece_mb", (1, 2))
def test_valid_streams(z, gpu, inputs, name, first_mb, piece_mb):
    a, comp = inputs[name]
    n = len(a)
    with pipe_env(piece_mb, first_mb):
        rcode, got, buf = inflate_into(z, comp, n)
        assert rcode == 0 and got == n and z.last_inflate_tier() == 1
        assert same(buf[:n], a) and bool((buf[n:] == POISON).all())
        rcode, got, buf = inflate_into(z, comp, n - 1)
        assert rcode == NOSPACE and got == n
        assert bool((buf[n - 1:] == POISON).all())
        # bytes behind the stream are ignored (src/inflate.ts:22-37 stops at BFINAL)
        longer = np.concatenate([comp, np.random.default_rng(n).integers(0, 256, 1 << 20, dtype=np.uint8)])
        rcode, got, buf = inflate_into(z, longer, n)
        assert rcode == 0 and got == n and same(buf[:n], a) and bool((buf[n:] == POISON).all())
        # the allocating form: asked once, for the exact size
        rcode, got, asked = inflate_alloc(z, comp, 0)
        assert rcode == 0 and got == n and [(i, x.size) for i, x in asked] == [(0, n)]
        assert same(asked[0][1], a)
        # ... and with an early upper estimate: the last array handed out holds the result as a prefix
        rcode, got, asked = inflate_alloc(z, comp, z.ZES_F_ALLOC_BOUND)
        assert rcode == 0 and got == n and 1 <= len(asked) <= 2
        assert asked[0][0] == z.ZES_ALLOC_EARLY and asked[0][1].size >= (n if len(asked) == 1 else 1)
        assert all(i == 0 and x.size == n for i, x in asked[1:])
        last = asked[-1][1]
        assert same(last[:n], a) and bool((last[n:] == POISON).all())


@pytest.mark.parametrize("case", rc.PIPE_DAMAGE, ids=["%s-%s" % (d[0], d[1]) for d in rc.PIPE_DAMAGE])
def test_damaged_streams(z, oracle, gpu, inputs, case):
    """Each damaged or truncated stream: oracle.inflate's bytes or its error code, pipelined in 1 MiB pieces and on the
    one-pass path alike."""
    name, dname, how, recorded = case
    a, comp = inputs[name]
    bad = rc.damaged(comp, how)
    want, want_bytes = rc.outcome(oracle, bad)
    assert want == recorded
    cap = len(a) + rc.BLOCK
    for off in (False, True):
        with pipe_env(1, 0, off=off):
            rcode, got, buf = inflate_into(z, bad, cap)
        if want[0] == "err":
            assert rcode == want[1], (dname, off, rcode, got)
        else:
            assert rcode == 0 and got == want[1], (dname, off, rcode, got)
            assert same(buf[:got], want_bytes), (dname, off)
        assert bool((buf[cap:] == POISON).all()), (dname, off)


def test_state_left_behind(z, oracle, gpu, inputs):
    """On one context, twice round: a valid pipelined call, one that ends mid-stream with the next piece enqueued, a short
    stream of another encoder, a valid pipelined call with more blocks, a one-buffer device call.  The device's block
    counter and the two result slots of the pieces must not carry over."""
    import torch

    a9, c9 = inputs["xorshift9"]
    a24, c24 = inputs["itext24"]
    broken = [d for d in rc.PIPE_DAMAGE if d[:2] == ("xorshift9", "middle_break")][0]
    bad = rc.damaged(c9, broken[2])
    want_bad, _ = rc.outcome(oracle, bad)
    assert want_bad == broken[3] and want_bad[0] == "err"
    plain = z.gen("itext", 604, 250000)
    other = np.frombuffer(zlib.compress(plain.tobytes(), 6), dtype=np.uint8).copy()
    assert 50000 <= len(other) <= 100000
    s = rc.range_stream(z, oracle, "itext")
    t = torch.from_numpy(s.comp).to(gpu)
    for _ in range(2):
        with pipe_env(1, 0):
            rcode, got, buf = inflate_into(z, c9, len(a9))
            assert rcode == 0 and got == len(a9) and same(buf[:got], a9) and z.last_inflate_tier() == 1
            rcode, got, buf = inflate_into(z, bad, len(a9) + rc.BLOCK)
            assert rcode == want_bad[1]
            rcode, got, buf = inflate_into(z, other, len(plain))
            assert rcode == 0 and got == len(plain) and same(buf[:got], plain)
            rcode, got, buf = inflate_into(z, c24, len(a24))
            assert rcode == 0 and got == len(a24) and same(buf[:got], a24) and z.last_inflate_tier() == 1
            out = torch.full((s.n + 16,), POISON, dtype=torch.uint8, device=gpu)
            back = z.inflate_tensor(t, out)
            assert back.numel() == s.n and same(back.cpu().numpy(), s.a) and z.last_inflate_tier() == 1
