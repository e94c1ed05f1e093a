"""The segment-parallel inflate tier's routes: streams of another encoder built to reach each of them, and a runner that
records what a call came to — status, tier, output length, whether the bytes are the input's, and the launches per
profiled name (zes_last_kernel_times).  tests/test_gpu_t2_routes.py compares the records with tests/golden/t2_routes.json.

    python -m tests._t2_routes > tests/golden/t2_routes.json     record every case (ZES_LIB selects the library)
    python -m tests._t2_routes pieces                            the `pieces` case alone, run twice (needs ZES_SEG_PIECE_MB=1
                                                                 from the start of the process: the library reads it once)

Every stream is Python zlib's, from the library's own generators; STREAM_BYTES holds the sizes they must have (another
zlib build writes other streams, and the recorded launches would not be theirs).
"""
import functools
import json
import os
import subprocess
import sys
import zlib as pz

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "t2_routes.json")
MIB = 1 << 20
PIECES_TIMEOUT = 120  # seconds, the child process of the `pieces` case

# compressed bytes of every stream
STREAM_BYTES = {"clean": 101869, "flushes": 351885, "fixed": 434409, "tiny blocks": 403410, "thinned": 1156688, "one long block": 10738,
                "mixed": 339267}
# the cases in the order they run; `pieces` last, in a process of its own
CASES = ["clean", "flushes", "fixed", "tiny blocks", "thinned", "one long block", "mixed", "wave only", "too small", "batch", "pieces"]
BATCH = ["clean", "thinned", "flushes", "fixed"]


def _pkg():
    import torch  # noqa: F401  (before the library: tests/conftest.py says why)

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    return ge.load()


def _deflate(plain, level=6, mem_level=8, strategy=pz.Z_DEFAULT_STRATEGY, flush_at=()):
    co = pz.compressobj(level, pz.DEFLATED, 15, mem_level, strategy)
    out, at = [], 0
    for cut in flush_at:
        out += [co.compress(plain[at:cut]), co.flush(pz.Z_SYNC_FLUSH)]
        at = cut
    out += [co.compress(plain[at:]), co.flush()]
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def stream(name):
    """(zlib stream, plain bytes) of a case's input."""
    z = _pkg()
    itext = lambda n: z.gen("itext", 91, n).tobytes()
    if name == "clean":
        plain = itext(MIB)[:300000]
        comp = _deflate(plain)
    elif name == "flushes":
        plain = itext(MIB)
        comp = _deflate(plain, flush_at=[k * MIB // 5 for k in range(1, 6)])  # (the fifth at the end: the final block is an empty fixed one)
    elif name == "fixed":
        plain = itext(MIB)
        comp = _deflate(plain, strategy=pz.Z_FIXED)
    elif name == "tiny blocks":
        plain = itext(MIB)
        comp = _deflate(plain, mem_level=1)
    elif name == "thinned":
        plain = itext(2 * MIB)
        comp = _deflate(plain, level=1, mem_level=1)
    elif name == "one long block":
        plain = z.gen("lowent4k", 92, MIB).tobytes()
        comp = _deflate(plain)
    elif name == "mixed":
        t = itext(MIB)
        plain = t[:200000] + z.gen("xorshift", 93, MIB).tobytes()[:200000] + t[200000:400000]
        comp = _deflate(plain)
    elif name == "pieces":
        plain = itext(4 * MIB)
        comp = _deflate(plain)
    else:
        raise KeyError(name)
    if name in STREAM_BYTES:
        assert len(comp) == STREAM_BYTES[name], "%s: %d compressed bytes, the case was written for %d" % (name, len(comp), STREAM_BYTES[name])
    return comp, plain


def _launches(z):
    return {name: n for name, _, n in z.last_kernel_times()}


def _one(z, gpu, name, cap=None, env=None):
    """One stream through the one-buffer device call."""
    import torch

    comp, plain = stream(name)
    d = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).to(gpu)
    out = torch.zeros(len(plain) if cap is None else cap, dtype=torch.uint8, device=gpu)
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        try:
            got = z.inflate_tensor(d, out)
            status, n, same = 0, got.numel(), bytes(got.cpu().numpy()) == plain
        except z.ZlibEsError as e:
            status, n, same = e.code, getattr(e, "need", 0), None
    finally:
        for k in env or {}:
            os.environ.pop(k, None)
    return {"status": status, "tier": z.last_inflate_tier(), "out_len": n, "bytes_equal": same, "launches": _launches(z)}


def _batch(z, gpu):
    """BATCH's streams in one device call."""
    import torch

    pairs = [stream(name) for name in BATCH]
    up = lambda n: (n + 15) // 16 * 16
    in_off, out_off, a, b = [], [], 0, 0
    for comp, plain in pairs:
        in_off.append(a)
        out_off.append(b)
        a += up(len(comp))
        b += up(len(plain))
    arena = np.zeros(a, dtype=np.uint8)
    for off, (comp, _) in zip(in_off, pairs):
        arena[off: off + len(comp)] = np.frombuffer(comp, dtype=np.uint8)
    out = torch.zeros(b, dtype=torch.uint8, device=gpu)
    olen, st = z.inflate_batch_tensor(torch.from_numpy(arena).to(gpu), in_off, [len(c) for c, _ in pairs], out, out_off, [len(p) for _, p in pairs])
    tier, launches = z.last_inflate_tier(), _launches(z)
    host = out.cpu().numpy()
    same = [bytes(host[off: off + n]) == plain if s == 0 else None for off, n, s, (_, plain) in zip(out_off, olen, st, pairs)]
    return {"status": [int(s) for s in st], "tier": tier, "out_len": [int(n) for n in olen], "bytes_equal": same, "launches": launches}


def run_case(z, gpu, name):
    """A case's record; profiling is on for the call and off again behind it."""
    z.set_profiling(True)
    try:
        if name == "batch":
            return _batch(z, gpu)
        if name == "wave only":
            return _one(z, gpu, "clean", env={"ZES_NO_SEG_PAR": "1"})
        if name == "too small":
            return _one(z, gpu, "flushes", cap=1024)
        return _one(z, gpu, name)
    finally:
        z.set_profiling(False)


def run_pieces_child():
    """[first record, second record] of the `pieces` case from a process that has ZES_SEG_PIECE_MB=1 from its start."""
    env = dict(os.environ, ZES_SEG_PIECE_MB="1")
    p = subprocess.run([sys.executable, "-m", "tests._t2_routes", "pieces"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=PIECES_TIMEOUT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(p.stdout.splitlines()[-1])


def _device(z):
    import torch

    assert torch.cuda.is_available(), "the routes are recorded on a GPU"
    z.init(0)
    return torch.device("cuda:0")


def main(argv):
    z = _pkg()
    gpu = _device(z)
    if argv[1:] == ["pieces"]:
        assert os.environ.get("ZES_SEG_PIECE_MB") == "1"
        print(json.dumps([run_case(z, gpu, "pieces"), run_case(z, gpu, "pieces")]))
        return 0
    rec = {}
    for name in CASES:
        first, second = run_pieces_child() if name == "pieces" else (run_case(z, gpu, name), run_case(z, gpu, name))
        assert first == second, "%s: the second run differs from the first: %r / %r" % (name, first, second)
        rec[name] = first
        print(name, first, file=sys.stderr)
    print(json.dumps(rec, indent=1, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
