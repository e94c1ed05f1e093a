"""Batches at the capacity edges of a context's page-locked area (PinnedArea in zlib.es_amd/csrc/zes_api.hip): deflate
batches one buffer past the results k_layout writes into the area (16384) and past 1 MiB of results, a second group of
the block-parallel tier (4096 buffers per group) and a second group of the segment-parallel tier (512 per group).  Every
result is checked against the oracle or the input."""
import struct
import zlib as pz

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GZ_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"  # what zes_gzip writes: FLG 0, MTIME 0, XFL 0, OS 255


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def arena(sizes):
    """16-byte aligned offsets for buffers of these sizes -> (offsets, total)"""
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos += (int(n) + 15) // 16 * 16
    return offs, max(pos, 16)


def packed(bufs):
    offs, total = arena([b.size for b in bufs])
    a = np.zeros(total, dtype=np.uint8)
    for b, o in zip(bufs, offs):
        a[o:o + b.size] = b
    return a, offs


def expect(oracle, fn, data):
    """the oracle's result, or the code of its error"""
    try:
        return fn(data)
    except oracle.OracleError as e:
        return e.code


def _deflate_edge(z, oracle, gpu, nlive):
    import torch

    contents = [z.gen(k, 40 + i, n) for i, (k, n) in enumerate((("itext", 2), ("xorshift", 17), ("lowent4k", 33), ("itext", 64),
                                                                ("xorshift", 64)))]
    contents.append(np.zeros(48, dtype=np.uint8))
    refused = [np.zeros(0, dtype=np.uint8), np.full(1, 7, dtype=np.uint8)]  # the reference throws on 0 and 1 bytes
    kinds = [i % len(contents) for i in range(nlive)]
    kinds[nlive // 2:nlive // 2] = [len(contents), len(contents) + 1]  # (not part of the device pass: nlive buffers are)
    allc = contents + refused
    want = [expect(oracle, oracle.deflate, c) for c in allc]
    bufs = [allc[k] for k in kinds]
    h_in, in_off = packed(bufs)
    caps = [z.deflate_bound(b.size) for b in bufs]
    out_off, total = arena(caps)
    d_out = torch.empty(total, dtype=torch.uint8, device=gpu)
    olen, st = z.deflate_batch_tensor(dev(h_in, gpu), in_off, [b.size for b in bufs], d_out, out_off, caps)
    kinds, olen, st, out_off = np.array(kinds), np.array(olen), np.array(st), np.array(out_off)
    for c, w in enumerate(want):
        sel = np.flatnonzero(kinds == c)
        if isinstance(w, int):
            assert (st[sel] == w).all(), c
            continue
        assert (st[sel] == 0).all() and (olen[sel] == w.size).all(), c
        idx = torch.from_numpy(out_off[sel]).to(gpu)[:, None] + torch.arange(w.size, device=gpu)[None, :]
        assert bool((d_out[idx] == dev(w, gpu)[None, :]).all()), c
    # the same context afterwards: one buffer through the block-parallel tier (its host chain reads the area), and gzip
    raw = z.gen("itext", 4242, 300000)
    back = z.inflate_tensor(dev(oracle.deflate(raw), gpu), torch.empty(raw.size, dtype=torch.uint8, device=gpu))
    assert z.last_inflate_tier() == 1 and np.array_equal(back.cpu().numpy(), raw)
    gz = z.gzip_tensor(dev(raw, gpu)).cpu().numpy().tobytes()
    assert gz == GZ_HEADER + oracle.deflate_raw(raw).tobytes() + struct.pack("<II", pz.crc32(raw.tobytes()), raw.size)


@pytest.mark.parametrize("nlive", [16385, 65537])
def test_deflate_batch_past_the_area(z, oracle, gpu, nlive):
    """16385 small buffers: one more than k_layout writes into the area; 65537: more than 1 MiB of results.  A few
    contents of 0-64 bytes, each output equal to the oracle's; then inflate and gzip of one buffer on the same context."""
    import torch

    try:
        _deflate_edge(z, oracle, gpu, nlive)
    finally:
        z.trim()  # (the batch's device scratch is sized per block: tens of GiB for 65537 blocks)
        torch.cuda.empty_cache()


def test_inflate_batch_second_block_parallel_group(z, oracle, gpu):
    """4100 reference streams: the block-parallel tier takes them in two groups.  The second one also holds a buffer
    that is no deflate stream, one whose first block is BTYPE 3 and one damaged in the middle."""
    import torch

    raws = [z.gen(("itext", "lowent4k", "xorshift")[i % 3], 500 + i, 100 + 61 * i) for i in range(12)]
    comps = [oracle.deflate(r) for r in raws]
    kinds = [i % len(raws) for i in range(4100)]
    long_raw = z.gen("itext", 600, 20000)
    damaged = oracle.deflate(long_raw)
    damaged[damaged.size // 2] ^= 0x55
    extra = [np.frombuffer(b"\x77\x9c" + bytes(98), dtype=np.uint8),  # not deflate (src/zlib.ts:13-16)
             np.frombuffer(b"\x78\x9c\x07" + bytes(97), dtype=np.uint8),  # BTYPE 3
             damaged]
    want = [expect(oracle, oracle.inflate, e) for e in extra]
    assert want[0] == -1 and want[1] == -2
    bufs = [comps[k] for k in kinds] + extra
    caps = [raws[k].size for k in kinds] + [64, 64, 1 << 20 if isinstance(want[2], int) else max(want[2].size, 16)]
    h_in, in_off = packed(bufs)
    out_off, total = arena(caps)
    d_out = torch.zeros(total, dtype=torch.uint8, device=gpu)
    olen, st = z.inflate_batch_tensor(dev(h_in, gpu), in_off, [b.size for b in bufs], d_out, out_off, caps)
    host = d_out.cpu().numpy()
    for i, k in enumerate(kinds):
        r = raws[k]
        assert st[i] == 0 and olen[i] == r.size, i
        assert np.array_equal(host[out_off[i]:out_off[i] + r.size], r), i
    n = len(kinds)
    assert st[n] == -1 and st[n + 1] == -2
    if isinstance(want[2], int):
        assert st[n + 2] == want[2]
    else:
        assert st[n + 2] == 0 and np.array_equal(host[out_off[n + 2]:out_off[n + 2] + olen[n + 2]], want[2])


def test_inflate_batch_second_segment_parallel_group(z, gpu):
    """520 streams of CPython's zlib: the segment-parallel tier takes them in two groups.  Every 16th stream is made of
    fixed blocks only, which the block decoder declines: the wave decoder gets them through the list of live items."""
    import torch

    raws, comps = [], []
    for i in range(520):
        raw = z.gen("itext", 3000 + i, 100000 + 997 * (i % 40))
        co = pz.compressobj(6, pz.DEFLATED, 15, 8, pz.Z_FIXED) if i % 16 == 5 else pz.compressobj((6, 1, 9)[i % 3])
        raws.append(raw)
        comps.append(np.frombuffer(co.compress(raw.tobytes()) + co.flush(), dtype=np.uint8))
    h_in, in_off = packed(comps)
    caps = [r.size for r in raws]
    out_off, total = arena(caps)
    d_out = torch.zeros(total, dtype=torch.uint8, device=gpu)
    z.set_profiling(True)
    try:
        olen, st = z.inflate_batch_tensor(dev(h_in, gpu), in_off, [c.size for c in comps], d_out, out_off, caps)
        launches = {k: n for k, ms, n in z.last_kernel_times()}
    finally:
        z.set_profiling(False)
    assert launches.get("k_inf_ranksort") == 2, launches  # (one candidate sort per group of several buffers)
    host = d_out.cpu().numpy()
    for i, r in enumerate(raws):
        assert st[i] == 0 and olen[i] == r.size, i
        assert np.array_equal(host[out_off[i]:out_off[i] + r.size], r), i
