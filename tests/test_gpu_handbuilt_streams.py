"""Every inflate tier on hand-built DEFLATE streams no encoder in the suite makes (tests/_handbuilt_cases.py):
distances 32507..32768 at block, segment and piece starts, rare legal shapes, the reference's quirks inside large
streams, and T1 impostors.  RFC-valid streams are held against zlib (the CPU tests hold the oracle to the same),
quirks and impostors against the oracle: bytes or error code.  DESIGN.md §4: the tiers change speed, never a result."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _deflate_writer as W
import _handbuilt_cases as H
from conftest import ROOT

pytestmark = pytest.mark.gpu

B = 131072


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy()).to(gpu)


def expect(oracle, blob):
    """The reference's result on a zlib-wrapped stream: ("out", bytes) or ("err", code)."""
    try:
        return ("out", oracle.inflate(blob).tobytes())
    except oracle.OracleError as e:
        return ("err", e.code)


def run(fn):
    try:
        return ("out", bytes(fn()))
    except Exception as e:  # noqa: BLE001 — ZlibEsError carries .code
        if not hasattr(e, "code"):
            raise
        return ("err", e.code)


def all_entries(z, gpu, raw, want, valid, tier=None, batch=True):
    """Every entry point on one raw stream; want = ("out", bytes) or ("err", code).  valid: RFC-valid (zlib's
    end of stream is checked, gunzip too).  tier: the tier the one-buffer call must take (None: not pinned;
    a set: any of them; a negative number: anything but its absolute value)."""
    import torch

    blob = W.zlib_wrap(raw)
    tiers = {}
    for flags in (0, z.ZES_F_NO_FASTPATH, z.ZES_F_PIECES):
        got = run(lambda: z.inflate(blob, flags).tobytes())
        assert got == want, ("inflate", flags, got[0], want[0], got[1] if got[0] == "err" else len(got[1]))
        tiers[flags] = z.last_inflate_tier()
    t0 = tiers[0]
    if isinstance(tier, int) and tier > 0:
        assert t0 == tier, ("tier", t0, tier)
    elif isinstance(tier, int) and tier < 0:
        assert t0 != -tier, ("tier", t0, tier)
    elif isinstance(tier, set):
        assert t0 in tier, ("tier", t0, tier)
    # the device form at an odd offset of its tensor, at exact capacity and one byte short
    d = dev(b"\x00" * 3 + blob, gpu)[3:]
    if want[0] == "out":
        n = len(want[1])
        o = torch.empty(max(n, 1), dtype=torch.uint8, device=gpu)
        back = z.inflate_tensor(d, o)
        assert back.numel() == n and bytes(back.cpu().numpy()) == want[1]
        if n:
            with pytest.raises(z.ZlibEsError) as ei:
                z.inflate_tensor(d, torch.empty(n - 1, dtype=torch.uint8, device=gpu))
            assert ei.value.code == z.ZES_E_NOSPACE and ei.value.need == n
    else:
        o = torch.empty(8 << 20, dtype=torch.uint8, device=gpu)  # room for everything in front of the error
        assert run(lambda: z.inflate_tensor(d, o).cpu().numpy()) == want
    # where the raw stream ends
    if valid:
        dz = zlib.decompressobj(-15)
        dz.decompress(raw + b"TRAILING")
        end = len(raw) + 8 - len(dz.unused_data)
        out, used = z.inflate_raw_used(b"\x05" * 5 + raw + b"TRAILING", 5)
        assert out.tobytes() == want[1] and used == end, (used, end)
        gz = W.gzip_wrap(raw[:end], want[1])
        assert z.gunzip(gz).tobytes() == want[1]
    # a batch of two: k_inf_chain walks the chains, not the host
    if batch:
        other = zlib.compress(H.text(70000, 9), 6)
        res = z.inflate_batch([blob, other])
        got = ("err", res[0].code) if isinstance(res[0], Exception) else ("out", res[0].tobytes())
        assert got == want, ("batch", got[0], want[0])
        assert res[1].tobytes() == H.text(70000, 9)
    return tiers


# ---------------------------------------------------------------------------------------------
# A. valid shapes
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_stream():
    s = H.far_distance_stream()
    return s.raw(), bytes(s.plain)


def test_far_distances_across_blocks_and_segments(z, gpu, far_stream):
    raw, plain = far_stream
    assert zlib.decompress(raw, -15) == plain
    all_entries(z, gpu, raw, ("out", plain), True, tier=2)


def test_far_distances_across_pieces_in_child(z, gpu):
    """ZES_SEG_PIECE_MB=1: the stream goes through T2 in pieces of 1 MiB; every hand-built block starts with a match
    at distance 32768, so later pieces start on one and read the oldest byte of the window the piece carries in
    front (ob.hist / hist): in the block decoder's translate step, in the window composition, and — with
    ZES_NO_SEG_PAR=1 — in the wave decoder's ring."""
    script = r"""
import os, sys, zlib
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import __graft_entry__ as ge
import _handbuilt_cases as H
import _deflate_writer as W
z = ge.load()
z.init(0)
for seed in (5, 6):
    s = H.far_distance_stream(seed=seed)
    raw, plain = s.raw(), bytes(s.plain)
    for wave in (False, True):  # the block decoder, then everything through the wave decoder (ZES_NO_SEG_PAR)
        if wave:
            os.environ["ZES_NO_SEG_PAR"] = "1"
        try:
            out = z.inflate(W.zlib_wrap(raw))
        finally:
            os.environ.pop("ZES_NO_SEG_PAR", None)
        assert out.tobytes() == plain, ("output", seed, wave)
        assert z.last_inflate_tier() == 2, z.last_inflate_tier()
    out, used = z.inflate_raw_used(raw + b"TAIL", 0)
    assert out.tobytes() == plain and used == len(raw), ("raw_used", seed, used, len(raw))
    d = torch.from_numpy(__import__("numpy").frombuffer(W.zlib_wrap(raw), dtype="uint8").copy()).cuda()
    o = torch.empty(len(plain), dtype=torch.uint8, device="cuda")
    back = z.inflate_tensor(d, o)
    assert back.numel() == len(plain) and bytes(back.cpu().numpy()) == plain, ("tensor", seed)
print("pieces ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, ZES_SEG_PIECE_MB="1")
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "pieces ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


SHAPES = [name for name, _ in H.shape_cases()]


@pytest.mark.parametrize("name", SHAPES)
def test_rare_legal_shapes(z, gpu, name):
    s = dict(H.shape_cases())[name]
    raw, plain = s.raw(), bytes(s.plain)
    assert zlib.decompress(raw, -15) == plain
    # >= 32 KiB compressed: T2 must take it (a stream of stored blocks only would not be; none of these is)
    all_entries(z, gpu, raw, ("out", plain), True, tier=2)


def test_bfinal_on_a_middle_block(z, gpu, oracle):
    raw, plain = H.bfinal_middle()
    assert expect(oracle, W.zlib_wrap(raw)) == ("out", plain)
    all_entries(z, gpu, raw, ("out", plain), True)


@pytest.mark.parametrize("n", [(1 << 27) - 1, 1 << 27, (1 << 27) + 1])
def test_one_block_of_2_to_the_27_bytes(z, gpu, n):
    """One dynamic block around PAR_MAX_OUT; through gunzip too (the CRC power table beyond 64 MiB)."""
    import torch

    raw = H.big_run_block(n)
    want = np.full(n, ord("Z"), dtype=np.uint8)
    out = z.inflate(W.zlib_wrap(raw))
    assert out.size == n and np.array_equal(out, want)
    gz = W.gzip_wrap(raw, want.tobytes())
    got = z.gunzip(gz)
    assert got.size == n and np.array_equal(got, want)
    o = torch.empty(n + 64, dtype=torch.uint8, device=gpu)
    back = z.gunzip_tensor(dev(gz, gpu), o)
    assert back.numel() == n and bool((back == ord("Z")).all())


# ---------------------------------------------------------------------------------------------
# B. quirks, in four places
# ---------------------------------------------------------------------------------------------
QUIRKS = [(c[0], where) for c in H.quirk_cases() for where in ("alone", "first", "last", "middle") if c[3] or where in ("alone", "first")]


@pytest.mark.parametrize("name,where", QUIRKS)
def test_quirk_blocks(z, gpu, oracle, name, where):
    fn, claim = {c[0]: (c[1], c[2]) for c in H.quirk_cases()}[name]
    raw = H.quirk_stream(fn, where)
    want = expect(oracle, W.zlib_wrap(raw))
    if where == "alone":
        assert want == (("err", claim) if isinstance(claim, int) else ("out", claim))
    all_entries(z, gpu, raw, want, False, batch=where in ("alone", "middle"))


# ---------------------------------------------------------------------------------------------
# C. T1 impostors
# ---------------------------------------------------------------------------------------------
IMPOSTORS = [c[0] for c in H.impostor_cases()]


@pytest.mark.parametrize("name", IMPOSTORS)
def test_t1_impostors(z, gpu, oracle, name):
    raw, t1_ok = {c[0]: (c[1], c[2]) for c in H.impostor_cases()}[name]
    want = expect(oracle, W.zlib_wrap(raw))
    d = zlib.decompressobj(-15)
    assert want == ("out", d.decompress(raw))
    tier = 1 if t1_ok else (-1 if t1_ok is False else None)
    all_entries(z, gpu, raw, want, d.unused_data == b"", tier=tier)


# ---------------------------------------------------------------------------------------------
# E. back to back on one context
# ---------------------------------------------------------------------------------------------
def test_back_to_back_on_one_context(z, gpu, oracle):
    import torch

    a = z.gen("itext", 77, 5 * B + 123)
    ref = oracle.deflate(a).tobytes()
    imp = {c[0]: c[1] for c in H.impostor_cases()}
    impostor = W.zlib_wrap(imp["matches into the previous block"])
    text = H.text(3 << 20, 78)
    foreign = zlib.compress(text, 6)
    truncated = foreign[: len(foreign) // 2]
    q = {c[0]: c[1] for c in H.quirk_cases()}
    quirk = W.zlib_wrap(H.quirk_stream(q["fixed dist code 30"], "middle"))
    seq = [(ref, 1), (impostor, -1), (foreign, 2), (truncated, None), (quirk, -1), (ref, 1)]
    wants = [expect(oracle, blob) for blob, _ in seq]
    assert wants[0] == ("out", a.tobytes()) and wants[2] == ("out", text) and wants[3][0] == "err"
    for rnd in range(2):
        for (blob, tier), want in zip(seq, wants):
            got = run(lambda: z.inflate(blob).tobytes())
            assert got == want
            t = z.last_inflate_tier()
            if tier is not None:
                assert (t == tier) if tier > 0 else (t != -tier), (t, tier)
            d = dev(blob, gpu)
            o = torch.empty(len(want[1]) if want[0] == "out" else 8 << 20, dtype=torch.uint8, device=gpu)
            n = C.c_uint64()
            rc = z.lib().zes_inflate_dev(d.data_ptr(), d.numel(), o.data_ptr(), o.numel(), C.byref(n), 0)
            if want[0] == "out":
                assert rc == 0 and n.value == len(want[1]) and bytes(o[: n.value].cpu().numpy()) == want[1]
            else:
                assert rc == want[1]
        # the batch form: k_inf_chain over the same sequence in one call
        res = z.inflate_batch([blob for blob, _ in seq])
        for r, want in zip(res, wants):
            got = ("err", r.code) if isinstance(r, Exception) else ("out", r.tobytes())
            assert got == want
