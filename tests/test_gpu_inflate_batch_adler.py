"""ZES_F_CHECK_ADLER in the batch forms: zes_inflate_batch_dev and zes_inflate_batch_alloc check every stream's Adler-32
trailer against its result with one segmented launch (k_adler_seg).  The batch is tests/_verify_cases.py's: a stream for
every inflate tier and path, intact and with its trailer damaged or cut, and buffers that fail for another reason.
Expected bytes come from the inputs, expected error codes of damaged bodies from the oracle."""
import ctypes as C
import os
import subprocess
import sys
import zlib as pz

import numpy as np
import pytest

import _verify_cases as vc
from conftest import ROOT

pytestmark = pytest.mark.gpu


def arena(sizes):
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos += (int(n) + 15) // 16 * 16
    return offs, max(pos, 16)


def run_dev(z, gpu, cases, flags):
    """the batch through zes_inflate_batch_dev -> (out_len[], status[], outputs as host bytes per case, launches)"""
    import torch

    in_off, tin = arena([c.stream.size for c in cases])
    h_in = np.zeros(tin + 64, dtype=np.uint8)
    for c, o in zip(cases, in_off):
        h_in[o:o + c.stream.size] = c.stream
    caps = [c.cap if c.cap is not None else (1 << 16 if isinstance(c.raw, int) else max(len(c.raw), 16)) for c in cases]
    out_off, tout = arena(caps)
    d_out = torch.zeros(tout, dtype=torch.uint8, device=gpu)
    z.set_profiling(True)
    try:
        olen, st = z.inflate_batch_tensor(torch.from_numpy(h_in).to(gpu), in_off, [c.stream.size for c in cases], d_out, out_off, caps, flags)
        launches = {k: n for k, ms, n in z.last_kernel_times()}
    finally:
        z.set_profiling(False)
    host = d_out.cpu().numpy()
    return olen, st, [host[o:o + min(n, cap)].tobytes() for o, n, cap in zip(out_off, olen, caps)], launches


def check(cases, flagged, olen, st, outs):
    for c, n, s, got in zip(cases, olen, st, outs):
        ws, wn, wb = vc.expected(c, flagged)
        assert s == ws, (c.label, flagged, s, ws)
        if wn is not None:
            assert n == wn, (c.label, flagged, n, wn)
        if wb is not None:  # (a failed check leaves the decoded bytes written, and their length)
            assert got == wb, (c.label, flagged)


@pytest.fixture(scope="module")
def full(z, oracle):
    return vc.full_batch(z, oracle)


def test_the_reference_made_stream_takes_the_block_parallel_tier(z, gpu, full):
    import torch

    t1 = full[0]
    assert t1.label == "T1 intact"
    back = z.inflate_tensor(torch.from_numpy(t1.stream.copy()).to(gpu), torch.empty(len(t1.raw), dtype=torch.uint8, device=gpu))
    assert z.last_inflate_tier() == 1 and back.cpu().numpy().tobytes() == t1.raw


def test_device_batch_with_the_flag(z, gpu, full):
    """Every status, length and output: ZES_E_CHECKSUM for a damaged or cut trailer, the body's own status first."""
    olen, st, outs, launches = run_dev(z, gpu, full, z.ZES_F_CHECK_ADLER)
    check(full, True, olen, st, outs)
    assert launches.get("k_adler_seg") == 1, launches  # one launch over all outputs


def test_device_batch_without_the_flag(z, gpu, full):
    """The trailer is ignored, as before: every trailer variant is ZES_OK; and nothing of the check runs."""
    olen, st, outs, launches = run_dev(z, gpu, full, 0)
    check(full, False, olen, st, outs)
    assert "k_adler_seg" not in launches, launches


@pytest.mark.parametrize("flagged", [True, False])
def test_few_short_streams_take_the_per_buffer_serial_wavefront(z, gpu, oracle, flagged):
    cases = vc.small_batch(z, oracle)
    assert len(cases) < 16  # SERIAL_BATCH_MIN_JOBS of zes_api.hip
    olen, st, outs, launches = run_dev(z, gpu, cases, z.ZES_F_CHECK_ADLER if flagged else 0)
    check(cases, flagged, olen, st, outs)
    assert z.last_inflate_tier() in (3, 4)  # (inflate_slow: the serial wavefront, the exact tier for what it declines)
    assert launches.get("k_adler_seg") == (1 if flagged else None), launches


def test_a_batch_whose_trailers_are_all_cut_launches_nothing(z, gpu, oracle):
    cases = [c for c in vc.small_batch(z, oracle) if "cut" in c.label]
    olen, st, outs, launches = run_dev(z, gpu, cases, z.ZES_F_CHECK_ADLER)
    check(cases, True, olen, st, outs)
    assert "k_adler_seg" not in launches, launches


def host_cases(z, oracle):
    """the batch of the host form: no capacities there; and 1 MiB of zeros, which outgrows the first guess of 4c"""
    cases = [c for c in vc.full_batch(z, oracle) if c.cap is None]
    zeros = bytes(1 << 20)
    stream = pz.compress(zeros)
    assert max(4 * len(stream), 1 << 16) < len(zeros)  # (inflate_batch_alloc_one's first guess)
    v = vc.variants("zeros", stream, zeros)
    return cases + v[:2]  # intact, trailer bit


def run_host(z, cases, flags):
    """zes_inflate_batch_alloc with an allocator that counts its calls -> (out_len[], status[], results, calls per index)"""
    cnt = len(cases)
    got, calls = {}, [0] * cnt

    def alloc(_user, index, n):
        calls[index] += 1
        got[index] = np.empty(max(int(n), 1), dtype=np.uint8)
        return got[index].ctypes.data

    arrs = [np.ascontiguousarray(c.stream) for c in cases]
    ptrs = (C.c_void_p * cnt)(*[a.ctypes.data for a in arrs])
    lens = (C.c_uint64 * cnt)(*[a.size for a in arrs])
    out_len, status = (C.c_uint64 * cnt)(), (C.c_int32 * cnt)()
    rc = z.lib().zes_inflate_batch_alloc(ptrs, lens, z.ALLOC_FN(alloc), None, out_len, status, cnt, flags)
    assert rc == 0
    return list(out_len), list(status), [got[i][:out_len[i]].tobytes() if i in got else None for i in range(cnt)], calls


@pytest.mark.parametrize("flagged", [True, False])
def test_host_batch(z, gpu, oracle, flagged):
    """A buffer that fails gets no memory request, every other buffer one; the zeros succeed in the second attempt."""
    cases = host_cases(z, oracle)
    olen, st, outs, calls = run_host(z, cases, z.ZES_F_CHECK_ADLER if flagged else 0)
    for c, n, s, got, k in zip(cases, olen, st, outs, calls):
        ws, wn, wb = vc.expected(c, flagged)
        assert s == ws, (c.label, flagged, s, ws)
        assert k == (1 if ws == 0 else 0), (c.label, flagged, k)
        if wn is not None:
            assert n == wn, (c.label, n, wn)
        if ws == 0:
            assert got == wb, c.label
    # the wrapper: an array or a ZlibEsError per buffer
    res = z.inflate_batch([c.stream for c in cases], z.ZES_F_CHECK_ADLER if flagged else 0)
    for c, r in zip(cases, res):
        ws, wn, wb = vc.expected(c, flagged)
        assert (r.code if isinstance(r, z.ZlibEsError) else 0) == ws, c.label
        if ws == 0:
            assert r.tobytes() == wb, c.label


PY = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch
torch.cuda.init()
import __graft_entry__ as ge
import _oracle
import _verify_cases as vc
z = ge.load()
assert z.init_devices(2) == 2
cases = [c for c in vc.full_batch(z, _oracle) if c.cap is None]
for flags in (z.ZES_F_CHECK_ADLER, 0):
    res = z.inflate_batch([c.stream for c in cases], flags)
    for c, r in zip(cases, res):
        ws, wn, wb = vc.expected(c, flags != 0)
        assert (r.code if isinstance(r, z.ZlibEsError) else 0) == ws, (c.label, flags)
        if ws == 0:
            assert r.tobytes() == wb, (c.label, flags)
print("checked batch over two contexts passed")
'''


def test_host_batch_over_two_contexts(gpu):
    env = dict(os.environ, ZES_OVERSUBSCRIBE="1", ZES_TEST_DEVICES="2")
    out = subprocess.run([sys.executable, "-c", PY % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "checked batch over two contexts passed" in out.stdout
