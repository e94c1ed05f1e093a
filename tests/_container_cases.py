"""The checksum / gzip / BGZF / ZIP / PNG layer's launches: a case per seam of the layer, each at the smallest shape that reaches it, and
a runner that records what a call came to — status, result, and the launches per profiled name (zes_last_kernel_times).
tests/test_gpu_container_launches.py compares the records with tests/golden/container_launches.json.

    python -m tests._container_cases      writes tests/golden/container_launches.json (ZES_LIB selects the library)

The launch counts are kept for this layer's kernels (LAYER); of a call's inflate and deflate kernels only the set of names.
Every input of the checksum, gzip and BGZF cases is the library's own (its generators, its encoders); the ZIP archives are
those of tests/_zip.py and tests/_zipwrite.py (CPython's bodies, the oracle's expected archive), built on the host, and the
PNG files those of tests/_png.py.
"""
import functools
import gzip as pygzip
import hashlib
import json
import os
import sys
import zlib as pz

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "container_launches.json")
if os.path.join(ROOT, "tests") not in sys.path:  # (python -m tests._container_cases)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import _png  # noqa: E402
import _zip  # noqa: E402
import _zipwrite  # noqa: E402

LAYER = ("k_crc32", "k_crc32_seg", "k_adler", "k_adler_seg", "k_gz_walk", "k_gz_gather", "k_bgzf_mark", "k_bgzf_pack", "k_zip_stage", "k_zip_pack",
         "k_png_walk", "k_png_unfilter", "k_png_filter", "k_png_pack", "k_crc32_put")
CHUNK = 65280  # ZES_BGZF_CHUNK

# (alignment, length) of the checksum cases' buffers: a start inside a 16-byte piece, a tail behind the last 16-byte boundary,
# one and two 64 KiB work items, a buffer of no bytes between two others and one in last place
SEGMENTS = [(15, 0), (15, 1), (0, 0), (15, 17), (0, 65536), (1, 65537), (7, 131075), (0, 0)]

CASES = ["crc32 batch", "adler32 batch", "crc32 batch, every length 0", "adler32 batch, every length 0", "crc32 batch, count 0",
         "adler32 batch, count 0", "gunzip_tensor bgzf", "gunzip bgzf", "gunzip two members", "bgzip_tensor", "bgzip_tensor pieces",
         "bgzf_index_tensor", "bgzf_index_tensor walk", "bgzf_read_tensor", "bgzf_read", "inflate_batch_tensor checked",
         "inflate_batch checked",
         "zip_read_tensor standard", "zip_read standard", "zip_read_tensor failures", "zip_read failures", "zip_read_tensor stored only",
         "zip_read_tensor one rejected", "zip_read_tensor count 0", "zipwrite_tensor nine pieces", "zipwrite_tensor refused only", "zipwrite nine",
         "bgzip_tensor 1 byte", "bgzf_read_tensor body damaged", "bgzf_read_tensor crc damaged", "gunzip_tensor bgzf crc damaged",
         "png_decode_tensor three", "png_decode three"]


def _pkg():
    import torch  # noqa: F401  (before the library: tests/conftest.py says why)

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    return ge.load()


def _itext(n, seed=7):
    return _pkg().gen("itext", seed, n)


@functools.lru_cache(maxsize=None)
def arena():
    """(bytes, off[], len[]) of the checksum cases."""
    off, length, pos = [], [], 0
    for align, n in SEGMENTS:
        off.append(pos + align)
        length.append(n)
        pos += (align + n + 15) // 16 * 16 + 16
    return _itext(pos), off, length


@functools.lru_cache(maxsize=None)
def bgzf_file(n):
    """(the library's bgzip of n bytes, the bytes)."""
    plain = _itext(n, 11)
    blob = _pkg().bgzip(plain)
    assert pygzip.decompress(blob.tobytes()) == plain.tobytes()
    return blob, plain.tobytes()


@functools.lru_cache(maxsize=None)
def bgzf_damaged(what):
    """The 70000-byte file with one bit flipped: the first of member 0's body, its first block's BFINAL ("body": the stream no
    longer ends where the member says), or one of member 1's CRC-32 ("crc")."""
    blob, plain = bgzf_file(70000)
    coff = _pkg().bgzf_index(blob)[0].tolist()
    bad = blob.copy()
    bad[coff[0] + 18 if what == "body" else coff[2] - 8] ^= 1
    return bad, plain


@functools.lru_cache(maxsize=None)
def zip_archive(which):
    """(the standard or the failure archive of tests/_zip.py, per entry (the expected status or statuses, the plain bytes))."""
    if which == "standard":
        blob, plain, _ = _zip.standard()
        return np.frombuffer(blob, dtype=np.uint8).copy(), [(0, p) for p in plain]
    blob, plan = _zip.failures()
    return np.frombuffer(blob, dtype=np.uint8).copy(), [(want, data) for _, want, data in plan]


def zipwrite_entries(z, which):
    if which == "nine":
        return _zipwrite.nine(z)
    c = dict(_zipwrite.cases(z))
    return [(n, c[n]) for n in (b"refused/%d" % n for n in _zipwrite.THROW_LENGTHS)]


@functools.lru_cache(maxsize=None)
def checked_streams():
    """Three zlib streams of a few KiB and their bytes: a good one, one with a wrong trailer, one cut inside its trailer."""
    z = _pkg()
    plains = [_itext(n, 20 + k) for k, n in enumerate((3000, 5000, 4000))]
    streams = [z.deflate(p).copy() for p in plains]
    streams[1][-1] ^= 1
    streams[2] = streams[2][:-2].copy()
    return streams, [p.tobytes() for p in plains]


def _dev(a, gpu, lead=0):
    """`a` on the device, `lead` bytes behind a 16-byte boundary."""
    import torch

    t = torch.zeros(lead + a.size, dtype=torch.uint8, device=gpu)
    assert t.data_ptr() % 16 == 0
    t[lead:] = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t[lead:]


def _call(z, fn):
    """status, what fn returns (None with a status), the NOSPACE size."""
    try:
        return 0, fn(), 0
    except z.ZlibEsError as e:
        return e.code, None, getattr(e, "need", 0)


def _record(z, status, **what):
    names = {name: n for name, _, n in z.last_kernel_times()}
    rec = {"status": status, "launches": {k: v for k, v in names.items() if k in LAYER}, "others": sorted(k for k in names if k not in LAYER)}
    rec.update(what)
    return rec


def _checksums(z, gpu, which, lengths=None, count=None):
    data, off, length = arena()
    if lengths is not None:
        length = lengths
    off, length = off[:count], length[:count]
    fn, ref = (z.crc32_batch_tensor, pz.crc32) if which == "crc32" else (z.adler32_batch_tensor, pz.adler32)
    status, got, _ = _call(z, lambda: fn(_dev(data, gpu), off, length))
    want = [ref(data[o:o + n].tobytes()) for o, n in zip(off, length)]
    return _record(z, status, values=got, values_equal=got == want)


def _gunzip(z, gpu, blob, plain, on_device):
    import torch

    if on_device:
        out = torch.zeros(len(plain), dtype=torch.uint8, device=gpu)
        status, got, _ = _call(z, lambda: z.gunzip_tensor(_dev(blob, gpu), out).cpu().numpy())
    else:
        status, got, _ = _call(z, lambda: z.gunzip(blob))
    return _record(z, status, out_len=None if got is None else int(got.size), bytes_equal=None if got is None else got.tobytes() == plain,
                   members=z.last_gunzip_members())


def _zip_read(z, gpu, which, on_device, sel=None):
    """`expected`: every entry's status is one that tests/_zip.py expects of it; `bytes_equal`: None for an entry with a status."""
    blob, rows = zip_archive(which)
    index = z.zip_index(blob)
    rows = rows if sel is None else [rows[k] for k in sel]
    if on_device:
        status, got, _ = _call(z, lambda: z.zip_read_tensor(_dev(blob, gpu, lead=1), index, sel=sel))
        out, off, out_len, st = got
        host = out.cpu().numpy()
        datas = [host[int(o):int(o) + n].tobytes() for o, n in zip(off, out_len)]
    else:
        status, res, _ = _call(z, lambda: z.zip_read(blob, index, sel=sel))
        st = [r.code if isinstance(r, z.ZlibEsError) else 0 for r in res]
        datas = [b"" if s else r.tobytes() for r, s in zip(res, st)]
    expected = [s == w or (isinstance(w, tuple) and s in w) for s, (w, _) in zip(st, rows)]
    return _record(z, status, statuses=st, expected=expected, bytes_equal=[d == p if s == 0 else None for d, s, (_, p) in zip(datas, st, rows)])


def _zip_write(z, gpu, which, on_device, flags=0):
    entries = zipwrite_entries(z, which)
    if on_device:
        lens = [len(d) for _, d in entries]
        arena_ = np.frombuffer(b"".join(d for _, d in entries), dtype=np.uint8).copy()
        status, got, _ = _call(z, lambda: z.zip_write_tensor(_dev(arena_, gpu, lead=3), np.cumsum([0] + lens)[:-1], lens, [n for n, _ in entries],
                                                             flags=flags))
        blob = got[0].cpu().numpy().tobytes()
    else:
        status, got, _ = _call(z, lambda: z.zip_write(entries, flags))
        blob = got[0].tobytes()
    sha = hashlib.sha256(blob).hexdigest()
    return _record(z, status, out_len=len(blob), sha256=sha, sha256_expected=sha == hashlib.sha256(_zipwrite.expect(entries)).hexdigest(),
                   methods=[int(e["method"]) for e in got[1][0]])


def _bgzip(z, gpu, n, flags):
    plain = _itext(n, 11)
    status, got, _ = _call(z, lambda: z.bgzip_tensor(_dev(plain, gpu), flags=flags, index=True))
    blob = got[0].cpu().numpy().tobytes()
    return _record(z, status, out_len=len(blob), sha256=hashlib.sha256(blob).hexdigest(), member_off=[int(v) for v in got[1]],
                   bytes_equal=pygzip.decompress(blob) == plain.tobytes())


def _index(z, gpu, flags):
    blob, _ = bgzf_file(4 * CHUNK + 1)
    status, got, _ = _call(z, lambda: z.bgzf_index_tensor(_dev(blob, gpu), flags))
    same = [a.tolist() for a in got] == [a.tolist() for a in z.bgzf_index(blob)]
    return _record(z, status, coff=got[0].tolist(), uoff=got[1].tolist(), same_as_host_index=same)


def _read(z, gpu, on_device, damage=None):
    import torch

    blob, plain = bgzf_file(70000)
    index = z.bgzf_index(blob)
    if damage:
        blob, _ = bgzf_damaged(damage)
    pos, length = 30000, CHUNK + 2000 - 30000  # the middle of member 0 to the middle of member 1
    if on_device:
        out = torch.zeros(3 + length, dtype=torch.uint8, device=gpu)[3:]
        assert out.data_ptr() % 16 == 3
        status, got, _ = _call(z, lambda: z.bgzf_read_tensor(_dev(blob, gpu), index, pos, length, out).cpu().numpy())
    else:
        status, got, _ = _call(z, lambda: z.bgzf_read(blob, index, pos, length))
    if got is None:
        return _record(z, status, out_len=None, bytes_equal=None, members=z.last_gunzip_members())
    return _record(z, status, out_len=int(got.size), bytes_equal=got.tobytes() == plain[pos:pos + length], members=z.last_gunzip_members())


def _checked(z, gpu, on_device):
    import torch

    streams, plains = checked_streams()
    if not on_device:
        res = z.inflate_batch(streams, z.ZES_F_CHECK_ADLER)
        st = [r.code if isinstance(r, z.ZlibEsError) else 0 for r in res]
        return _record(z, 0, statuses=st, bytes_equal=[r.tobytes() == p if s == 0 else None for r, s, p in zip(res, st, plains)])
    up = lambda n: (n + 15) // 16 * 16
    in_off, out_off = np.cumsum([0] + [up(s.size) for s in streams]).tolist(), np.cumsum([0] + [up(len(p)) for p in plains]).tolist()
    h_in = np.zeros(in_off[-1] + 64, dtype=np.uint8)
    for s, o in zip(streams, in_off):
        h_in[o:o + s.size] = s
    out = torch.zeros(out_off[-1], dtype=torch.uint8, device=gpu)
    status, got, _ = _call(z, lambda: z.inflate_batch_tensor(_dev(h_in, gpu), in_off[:-1], [s.size for s in streams], out, out_off[:-1],
                                                             [len(p) for p in plains], z.ZES_F_CHECK_ADLER))
    host = out.cpu().numpy()
    olen, st = got
    return _record(z, status, statuses=[int(s) for s in st], out_len=[int(n) for n in olen],
                   bytes_equal=[host[o:o + len(p)].tobytes() == p for o, p in zip(out_off, plains)])


@functools.lru_cache(maxsize=None)
def png_three():
    """Three small files of tests/_png.py: a good one, one whose zlib stream has a flipped Adler-32, another good one."""
    a, b = _png.neighbours()
    bad = [c for c in _png.damage() if c.name == "flipped Adler-32"]
    assert len(bad) == 1 and bad[0].status == _png.ZES_E_CHECKSUM
    return [a, bad[0], b]


def _png_decode(z, gpu, on_device):
    import torch

    cases = png_three()
    if on_device:
        blobs = [np.frombuffer(c.blob, dtype=np.uint8) for c in cases]
        in_off = np.cumsum([0] + [b.size + 3 for b in blobs])[:-1].tolist()  # (the second and third file off the 16-byte boundaries)
        flat = np.zeros(in_off[-1] + blobs[-1].size, dtype=np.uint8)
        for o, b in zip(in_off, blobs):
            flat[o:o + b.size] = b
        off = np.cumsum([0] + [len(c.want) + 5 for c in cases])[:-1].tolist()
        out = torch.zeros(off[-1] + len(cases[-1].want), dtype=torch.uint8, device=gpu)
        status, got, _ = _call(z, lambda: z.png_decode_tensor(_dev(flat, gpu, lead=1), in_off, [b.size for b in blobs], out=out, off=off))
        host = got[0].cpu().numpy()
        out_len, st = got[2], got[3]
        datas = [host[o:o + n].tobytes() for o, n in zip(off, out_len)]
    else:
        status, res, _ = _call(z, lambda: z.png_decode_batch([c.blob for c in cases]))
        st = [r.code if isinstance(r, z.ZlibEsError) else 0 for r in res]
        datas = [b"" if s else r[1].tobytes() for r, s in zip(res, st)]
        out_len = [len(d) for d in datas]
    return _record(z, status, statuses=st, out_len=out_len, bytes_equal=[d == c.want if s == 0 else None for d, s, c in zip(datas, st, cases)])


def run_case(z, gpu, name):
    """A case's record; profiling is on for the call and off again behind it."""
    z.set_profiling(True)
    try:
        if name.split()[0] in ("png_decode_tensor", "png_decode"):
            return _png_decode(z, gpu, name.startswith("png_decode_tensor"))
        if name.split()[0] in ("zip_read_tensor", "zip_read"):
            on_device = name.startswith("zip_read_tensor")
            if name.endswith("stored only"):
                return _zip_read(z, gpu, "standard", on_device, sel=[k for k, e in enumerate(z.zip_index(zip_archive("standard")[0])[0]) if e["method"] == 0])
            if name.endswith("one rejected"):
                return _zip_read(z, gpu, "failures", on_device, sel=[[what for what, _, _ in _zip.failures()[1]].index("local signature damaged")])
            if name.endswith("count 0"):
                return _zip_read(z, gpu, "standard", on_device, sel=[])
            return _zip_read(z, gpu, name.split()[1], on_device)
        if name.endswith("batch"):
            return _checksums(z, gpu, name.split()[0])
        if name.endswith("every length 0"):
            return _checksums(z, gpu, name.split()[0], lengths=[0] * len(SEGMENTS))
        if name.endswith("count 0"):
            return _checksums(z, gpu, name.split()[0], count=0)
        if name in ("gunzip_tensor bgzf", "gunzip bgzf"):
            return _gunzip(z, gpu, *bgzf_file(70000), on_device=name.startswith("gunzip_tensor"))
        if name == "gunzip two members":
            a, b = _itext(3000, 31), _itext(70000, 32)
            return _gunzip(z, gpu, np.concatenate([z.gzip(a), z.gzip(b)]), a.tobytes() + b.tobytes(), on_device=False)
        if name == "bgzip_tensor":
            return _bgzip(z, gpu, 70000, 0)
        if name == "bgzip_tensor pieces":
            return _bgzip(z, gpu, 4 * CHUNK + 1, z.ZES_F_PIECES)  # five members: two groups of ENC_GROUP_PIECES
        if name.startswith("bgzf_index_tensor"):
            return _index(z, gpu, z.ZES_F_INDEX_WALK if name.endswith("walk") else 0)
        if name in ("bgzf_read_tensor", "bgzf_read"):
            return _read(z, gpu, name == "bgzf_read_tensor")
        if name in ("inflate_batch_tensor checked", "inflate_batch checked"):
            return _checked(z, gpu, name.startswith("inflate_batch_tensor"))
        if name == "zipwrite_tensor nine pieces":
            return _zip_write(z, gpu, "nine", True, z.ZES_F_PIECES)
        if name == "zipwrite_tensor refused only":
            return _zip_write(z, gpu, "refused", True)
        if name == "zipwrite nine":
            return _zip_write(z, gpu, "nine", False)
        if name == "bgzip_tensor 1 byte":
            # behind a call whose report is empty: where the encoder refuses a whole group, the report of the call in front
            # is kept as this call's own (NOTES.md), and the record would depend on what ran before
            z.crc32_batch_tensor(_dev(_itext(16), gpu), [], [])
            return _bgzip(z, gpu, 1, 0)
        if name.startswith("bgzf_read_tensor") and name.endswith("damaged"):
            return _read(z, gpu, True, damage=name.split()[1])
        if name == "gunzip_tensor bgzf crc damaged":
            return _gunzip(z, gpu, *bgzf_damaged("crc"), on_device=True)
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
