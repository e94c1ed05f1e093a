"""The gzip batch forms on the MI355X (zes_gzip_batch*, zes_gunzip_batch*; include/zes.h).  The writer: bit-exact with the file
that tests/_gzip_batch.py's builder assembles around z.gzip's own body or the stored form, at odd places between sentinels, in
groups, with launches that do not grow with the files.  The reader: the batched route finishes every good single member in a
fixed set of launches; every other file gets exactly what zes_gunzip_dev gives for it alone, which the same call under
ZES_F_GZIP_SERIAL and the single-file form both say."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import _gzip_batch as G
import _gzip_batch_poison  # noqa: F401  (adds the batch forms' entries to the poison catalogue, tests/_poison_cases.py)

pytestmark = pytest.mark.gpu

SENT = 0xA5
ERR_CAP = 1008  # the room of a file that is expected to fail: its output, were it good, would fit


def ptr(a):
    return a.ctypes.data if a.size else None


def dev_batch(z, gpu, which, blobs, caps, in_at=1, out_at=5, gap=0, flags=0, null_out=False):
    """zes_gzip_batch_dev / zes_gunzip_batch_dev: the inputs back to back behind in_at bytes of a 16-byte aligned tensor, the
    outputs' ranges butted against each other (gap bytes between them) from byte out_at of a tensor filled with the sentinel.
    -> (status, out_len, the output tensor on the host, the ranges' offsets)."""
    import torch

    cnt = len(blobs)
    blob = b"".join(blobs)
    t = torch.zeros(in_at + len(blob) + 1, dtype=torch.uint8, device=gpu)
    if blob:
        t[in_at:in_at + len(blob)] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(gpu)
    ioff = np.cumsum([0] + [len(b) for b in blobs], dtype=np.uint64)[:cnt]
    ilen = np.array([len(b) for b in blobs], dtype=np.uint64)
    ocap = np.array(caps, dtype=np.uint64)
    ooff = np.cumsum([0] + [int(c) + gap for c in caps], dtype=np.uint64)[:cnt]
    out = torch.full((out_at + int(sum(caps)) + gap * cnt + 40,), SENT, dtype=torch.uint8, device=gpu)
    assert t.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    out_len = np.full(max(cnt, 1), 77, dtype=np.uint64)
    status = np.full(max(cnt, 1), 77, dtype=np.int32)
    torch.cuda.synchronize()
    fn = z.lib().zes_gzip_batch_dev if which == "gzip" else z.lib().zes_gunzip_batch_dev
    rc = fn(t.data_ptr() + in_at, ptr(ioff), ptr(ilen), cnt, None if null_out else out.data_ptr() + out_at, ptr(ooff), ptr(ocap), out_len.ctypes.data,
            status.ctypes.data, flags)
    assert rc == 0, rc
    return [int(s) for s in status[:cnt]], [int(n) for n in out_len[:cnt]], out.cpu().numpy(), [out_at + int(o) for o in ooff]


def untouched(host, offs, lens):
    """Every byte outside the ranges [offs[i], offs[i] + lens[i]) is still the sentinel."""
    mask = np.ones(host.size, dtype=bool)
    for o, n in zip(offs, lens):
        mask[o:o + n] = False
    return bool((host[mask] == SENT).all())


def launches(z):
    return {name: n for name, _, n in z.last_kernel_times()}


@pytest.fixture(scope="module")
def writer(z, gpu):
    """[(name, data, file, kind)]: the writer's case list with the builder's files around z.gzip's own bodies."""
    raw = lambda d: z.gzip(np.frombuffer(d, dtype=np.uint8))[10:-8]
    out = []
    for name, data in G.writer_cases(z):
        f, kind = G.expect(data, raw)
        assert f == G.expect(data)[0], name  # (the CPU oracle's body is the same)
        out.append((name, data, f, kind))
    return out


@pytest.fixture(scope="module")
def mixed(z, gpu):
    """[(name, file, cap, good)]: the reader's good files and the per-file route's, interleaved."""
    good = [(n, f, len(p), True) for n, f, p in G.good_files(z)]
    bad = [(n, f, len(v) + d if v is not None else ERR_CAP, False) for n, f, v, d in G.serial_files(z)]
    out = []
    for k in range(max(len(good), len(bad))):
        out += good[k:k + 1] + bad[k:k + 1]
    return out


def alone(z, gpu, blob, cap, in_at=3):
    """zes_gunzip_dev on one file -> (status, out_len, the bytes at ZES_OK)."""
    import torch

    t = torch.zeros(in_at + len(blob) + 1, dtype=torch.uint8, device=gpu)
    if blob:
        t[in_at:in_at + len(blob)] = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(gpu)
    out = torch.full(((cap + 15) // 16 * 16 + 16,), SENT, dtype=torch.uint8, device=gpu)
    n = C.c_uint64(77)
    torch.cuda.synchronize()
    rc = z.lib().zes_gunzip_dev(t.data_ptr() + in_at, len(blob), out.data_ptr(), cap, C.byref(n), 0)
    return rc, n.value, out.cpu().numpy()[:n.value].tobytes() if rc == 0 else None


def test_writer_exact_bytes(z, gpu, writer):
    kinds = {kind for _, _, _, kind in writer} | {"two blocks" for _, d, _, kind in writer if kind != "stream" and len(d) > 65535}
    assert kinds == {"stream", "longer", "refused", "two blocks"}
    status, out_len, host, offs = dev_batch(z, gpu, "gzip", [d for _, d, _, _ in writer], [G.bound(len(d)) for _, d, _, _ in writer])
    for (name, data, want, kind), st, n, o in zip(writer, status, out_len, offs):
        got = host[o:o + n].tobytes()
        assert (st, n) == (0, len(want)), (name, st, n, len(want))
        assert got == want, "%s (%s): first difference at byte %d of %d" % (name, kind, next(i for i in range(n) if got[i] != want[i]), n)
        assert gzip.decompress(got) == data and struct.unpack("<I", got[-8:-4])[0] == zlib.crc32(data), name
        if kind == "stream":
            assert got == z.gzip(np.frombuffer(data, dtype=np.uint8)).tobytes(), name
    assert untouched(host, offs, out_len)
    # the same inputs give the same bytes
    again = dev_batch(z, gpu, "gzip", [d for _, d, _, _ in writer], [G.bound(len(d)) for _, d, _, _ in writer])
    assert again[:2] == (status, out_len) and (again[2] == host).all()


def test_writer_placement(z, gpu, writer):
    data = [d for _, d, _, _ in writer]
    want = [f for _, _, f, _ in writer]
    for in_at in (1, 7):
        # every range exactly its file: the files meet at whatever byte they end
        status, out_len, host, offs = dev_batch(z, gpu, "gzip", data, [len(f) for f in want], in_at=in_at, out_at=in_at + 2)
        assert status == [0] * len(want) and out_len == [len(f) for f in want] and len({o % 16 for o in offs}) >= 8
        assert [host[o:o + n].tobytes() for o, n in zip(offs, out_len)] == want and untouched(host, offs, out_len)
    # one byte short: the size needed, and the range untouched; its neighbours are written
    short = (3, 5, 8, 14)  # text 17 (stored), text 65536 (stream), text 300000 (stream), random 65536 (two blocks)
    caps = [len(f) - (1 if i in short else 0) for i, f in enumerate(want)]
    status, out_len, host, offs = dev_batch(z, gpu, "gzip", data, caps, in_at=7, out_at=3)
    assert status == [G.NOSPACE if i in short else 0 for i in range(len(want))] and out_len == [len(f) for f in want]
    ok = [i for i in range(len(want)) if i not in short]
    assert [host[offs[i]:offs[i] + out_len[i]].tobytes() for i in ok] == [want[i] for i in ok]
    assert untouched(host, [offs[i] for i in ok], [out_len[i] for i in ok])
    # every capacity 0: a sizing pass, with and without an output
    for null_out in (False, True):
        status, out_len, host, offs = dev_batch(z, gpu, "gzip", data, [0] * len(want), null_out=null_out)
        assert status == [G.NOSPACE] * len(want) and out_len == [len(f) for f in want] and (host == SENT).all()


def test_writer_groups(z, gpu, writer):
    files = dict((n, f) for n, _, f, _ in writer)
    nine = G.nine(z)
    data = [d for _, d in nine]
    want = [files[n] for n, _ in nine]
    z.set_profiling(True)
    try:
        status, out_len, host, offs = dev_batch(z, gpu, "gzip", data, [len(f) for f in want], flags=z.ZES_F_PIECES)
        n = launches(z)
        assert status == [0] * 9 and [host[o:o + k].tobytes() for o, k in zip(offs, out_len)] == want and untouched(host, offs, out_len)
        assert n.get("k_gz_pack") == 3 and n.get("k_crc32_seg") == 3, n  # a launch per group, none per file
        status, out_len, host, offs = dev_batch(z, gpu, "gzip", data, [len(f) for f in want])
        n = launches(z)
        assert [host[o:o + k].tobytes() for o, k in zip(offs, out_len)] == want
        assert n.get("k_gz_pack") == 1 and n.get("k_crc32_seg") == 1 and max(n.values()) < 9, n
        # 64 files and 2: the same kernels the same number of times
        two = [d for _, d, _, kind in writer if kind == "stream"][:2]
        seen = []
        for mult in (1, 32):
            status, out_len, host, offs = dev_batch(z, gpu, "gzip", two * mult, [G.bound(len(d)) for d in two] * mult)
            assert status == [0] * (2 * mult)
            seen.append(launches(z))
        assert seen[0] == seen[1] and seen[0].get("k_gz_pack") == 1, seen
    finally:
        z.set_profiling(False)


def test_reader_batched_route(z, gpu):
    good = G.good_files(z)
    files, plains = [f for _, f, _ in good], [p for _, _, p in good]
    places = set()
    z.set_profiling(True)
    try:
        for in_at, out_at, gap in ((1, 5, 0), (16, 16, 0), (7, 0, 3)):
            caps = [len(p) for p in plains]
            if out_at == 16:  # every range at a 16-byte boundary
                caps = [(len(p) + 15) // 16 * 16 for p in plains]
            status, out_len, host, offs = dev_batch(z, gpu, "gunzip", files, caps, in_at=in_at, out_at=out_at, gap=gap)
            assert status == [0] * len(good) and out_len == [len(p) for p in plains], (status, out_len)
            assert [host[o:o + n].tobytes() for o, n in zip(offs, out_len)] == plains and untouched(host, offs, out_len)
            assert z.last_gunzip_batch() == (len(good), 0)
            n = launches(z)
            assert n.get("k_gz_heads") == 1 and n.get("k_crc32_seg") == 1 and max(n.values()) < len(good), n  # none per file
            places |= {(o % 16 == 0, k % 16 == 0) for o, k in zip(offs, out_len) if k}
        assert places == {(a, b) for a in (False, True) for b in (False, True)}  # aligned and odd places, sizes that are and are not whole groups
        # 2 files and 64: the same set of launches
        two = [files[1], files[3]]  # CPython's level 6 and z.gzip's two blocks: both decoder tiers
        seen = []
        for mult in (1, 32):
            status, out_len, host, offs = dev_batch(z, gpu, "gunzip", two * mult, [len(plains[1]), len(plains[3])] * mult)
            assert status == [0] * (2 * mult) and z.last_gunzip_batch() == (2 * mult, 0)
            assert host[offs[-1]:offs[-1] + out_len[-1]].tobytes() == plains[3]
            seen.append(launches(z))
        print(seen)
        assert set(seen[0]) == set(seen[1]) and max(seen[1].values()) < 64, seen  # no new kernel, and none launched per file
        assert all(seen[0].get(k) == seen[1].get(k) for k in ("k_gz_heads", "k_gz_gather", "k_crc32_seg")) and seen[1]["k_gz_heads"] == 1, seen
    finally:
        z.set_profiling(False)


def test_reader_per_file_route(z, gpu, mixed):
    files, caps = [f for _, f, _, _ in mixed], [c for _, _, c, _ in mixed]
    ngood = sum(1 for m in mixed if m[3])
    got = dev_batch(z, gpu, "gunzip", files, caps, in_at=1, out_at=5)
    assert z.last_gunzip_batch() == (ngood, len(mixed) - ngood)
    serial = dev_batch(z, gpu, "gunzip", files, caps, in_at=1, out_at=5, flags=z.ZES_F_GZIP_SERIAL)
    assert z.last_gunzip_batch() == (0, len(mixed))
    assert got[:2] == serial[:2] and got[3] == serial[3], (got[:2], serial[:2])
    status, out_len, host, offs = got
    statuses = {}
    for (name, f, cap, good), st, n, o in zip(mixed, status, out_len, offs):
        rc1, n1, bytes1 = alone(z, gpu, f, cap)
        print(name, st, n, "| alone:", rc1, n1)
        assert (st, n) == (rc1, n1), (name, st, n, rc1, n1)
        if st == 0:
            assert host[o:o + n].tobytes() == bytes1 == serial[2][o:o + n].tobytes(), name
        assert good == (st == 0 and name not in [x[0] for x in G.serial_files(z)]), name
        statuses[name] = st
    assert untouched(host, offs, caps) and untouched(serial[2], offs, caps)
    for name, want in _gzip_batch_poison.STATED.items():
        assert statuses[name] == want, (name, statuses[name], want)
    assert statuses["out_cap one short"] == G.NOSPACE and statuses["ISIZE 0xFFFFFFF0"] == G.E_CHECKSUM
    assert all(statuses[n] != 0 for n in ("10 bytes", "17 bytes", "cut inside the header", "cut inside the body", "cut inside the trailer", "one flipped body bit",
                                          "ISIZE one more"))


def test_lying_isize_costs_nothing(z, gpu):
    """A 40-byte file whose trailer claims 0xFFFFFFF0 bytes, in the alloc form.  The bound: the per-file route's scratch follows the
    file's 40 bytes and fixed minimum sizes, never ISIZE — the 64 KiB that the route's output scratch starts with, and the member's staging
    and the serial decoder's tables at their smallest sizes, a few KiB a pool over the library's some fifty pools: 4 MiB over a
    good 40-byte file's growth covers those whatever the case is, and a scratch sized by any lie above it is caught."""
    lying = next(f for n, f, _, _ in G.serial_files(z) if n.startswith("40 bytes"))
    good, plain = G.forty_good(z)
    z.trim()
    before = z.pool_bytes()
    assert z.gunzip_batch([good])[0].tobytes() == plain and z.last_gunzip_batch() == (1, 0)
    grew_good = z.pool_bytes() - before
    z.trim()
    assert z.pool_bytes() == before
    got = z.gunzip_batch([lying])[0]
    grew_lying = z.pool_bytes() - before
    print("pool growth: a good 40-byte file %d bytes, the lying one %d bytes" % (grew_good, grew_lying))
    assert isinstance(got, z.ZlibEsError) and got.code == G.E_CHECKSUM and z.last_gunzip_batch() == (0, 1)
    assert grew_lying <= grew_good + (4 << 20)
    z.trim()


def test_host_forms_and_tensors(z, gpu, writer, mixed):
    import torch

    # the writer: the host form and the tensor form give the device form's files
    data, want = [d for _, d, _, _ in writer], [f for _, _, f, _ in writer]
    assert [x.tobytes() for x in z.gzip_batch(data)] == want
    assert [x.tobytes() for x in z.gzip_batch(data, z.ZES_F_PIECES)] == want
    blob = np.frombuffer(b"".join(data), dtype=np.uint8)
    t = torch.from_numpy(np.concatenate([np.zeros(3, dtype=np.uint8), blob])).to(gpu)[3:]
    ioff = np.cumsum([0] + [len(d) for d in data])[:-1]
    out, off, out_len, status = z.gzip_batch_tensor(t, ioff, [len(d) for d in data])
    host = out.cpu().numpy()
    assert status == [0] * len(want) and [host[int(o):int(o) + n].tobytes() for o, n in zip(off, out_len)] == want
    sized = z.gzip_batch_tensor(t, ioff, [len(d) for d in data], off=np.zeros(len(data), dtype=np.uint64), cap=np.zeros(len(data), dtype=np.uint64))
    assert sized[0] is None and sized[2] == [len(f) for f in want] and sized[3] == [G.NOSPACE] * len(want)
    # the reader: per file what the device form says (a capacity is the device form's alone)
    files = [f for _, f, _, _ in mixed]
    dstat, dlen, dhost, doffs = dev_batch(z, gpu, "gunzip", files, [c + 1 if n == "out_cap one short" else c for n, _, c, _ in mixed])
    calls = []
    keep = {}

    def alloc(_u, i, n):
        calls.append((i, n))
        keep[i] = np.empty(max(int(n), 1), dtype=np.uint8)
        return keep[i].ctypes.data

    ptrs = (C.c_void_p * len(files))(*[np.frombuffer(f, dtype=np.uint8).ctypes.data if f else None for f in files])
    held = [np.frombuffer(f, dtype=np.uint8) for f in files]  # noqa: F841  (the pointers' memory)
    ln = np.array([len(f) for f in files], dtype=np.uint64)
    out_len = np.zeros(len(files), dtype=np.uint64)
    status = np.zeros(len(files), dtype=np.int32)
    assert z.lib().zes_gunzip_batch_alloc(ptrs, ln.ctypes.data, len(files), z.ALLOC_FN(alloc), None, out_len.ctypes.data, status.ctypes.data, 0) == 0
    assert [int(s) for s in status] == dstat and [int(n) for n in out_len] == [n if s == 0 else 0 for s, n in zip(dstat, dlen)]
    assert calls == [(i, dlen[i]) for i in range(len(files)) if dstat[i] == 0]  # once per file at ZES_OK, in order, never for a failed one
    for i, o in enumerate(doffs):
        if dstat[i] == 0:
            assert keep[i][:dlen[i]].tobytes() == dhost[o:o + dlen[i]].tobytes(), mixed[i][0]
    ngood = sum(1 for m in mixed if m[3]) + 1  # (without a capacity "out_cap one short" is one more good file)
    assert z.last_gunzip_batch() == (ngood, len(mixed) - ngood)
    got = z.gunzip_batch(files, z.ZES_F_GZIP_SERIAL)
    assert z.last_gunzip_batch() == (0, len(mixed))
    assert [x.code if isinstance(x, Exception) else 0 for x in got] == dstat
    assert all(isinstance(x, Exception) or x.tobytes() == keep[i][:dlen[i]].tobytes() for i, x in enumerate(got))
    # the tensor form with its own sizing pass and placement
    fblob = np.frombuffer(b"".join(files), dtype=np.uint8)
    ft = torch.from_numpy(np.concatenate([np.zeros(5, dtype=np.uint8), fblob])).to(gpu)[5:]
    foff = np.cumsum([0] + [len(f) for f in files])[:-1]
    out, off, tlen, tstat = z.gunzip_batch_tensor(ft, foff, [len(f) for f in files])
    assert tstat == dstat and tlen == [n if s == 0 else 0 for s, n in zip(dstat, dlen)]
    host = out.cpu().numpy()
    assert all(host[int(o):int(o) + n].tobytes() == keep[i][:n].tobytes() for i, (o, n) in enumerate(zip(off, tlen)) if tstat[i] == 0)


def test_poisoned_scratch_and_trim(z, gpu, writer, mixed):
    files = dict((n, f) for n, _, f, _ in writer)
    nine = G.nine(z)
    data, want = [d for _, d in nine], [files[n] for n, _ in nine]
    gfiles, caps = [f for _, f, _, _ in mixed], [c for _, _, c, _ in mixed]
    first = dev_batch(z, gpu, "gunzip", gfiles, caps)
    for word in (0xFFFFFFFF, 0):
        z.stage_poison(word)
        status, out_len, host, offs = dev_batch(z, gpu, "gzip", data, [len(f) for f in want], flags=z.ZES_F_PIECES)
        assert status == [0] * 9 and [host[o:o + n].tobytes() for o, n in zip(offs, out_len)] == want
        z.stage_poison(word)
        assert [x.tobytes() for x in z.gzip_batch(data)] == want
        z.stage_poison(word)
        again = dev_batch(z, gpu, "gunzip", gfiles, caps)
        assert again[:2] == first[:2]
        assert all(again[2][o:o + n].tobytes() == first[2][o:o + n].tobytes() for s, n, o in zip(again[0], again[1], again[3]) if s == 0)
        z.stage_poison(word)
        host_got = z.gunzip_batch(gfiles)
        assert [x.code if isinstance(x, Exception) else 0 for x in host_got] == [s if s != G.NOSPACE else 0 for s in first[0]]
    z.trim()
    before = z.pool_bytes()
    dev_batch(z, gpu, "gzip", data, [len(f) for f in want])
    dev_batch(z, gpu, "gunzip", gfiles, caps)
    assert z.pool_bytes() > before
    z.trim()
    assert z.pool_bytes() == before
