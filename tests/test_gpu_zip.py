"""The ZIP reader on the MI355X (zes_zip_index_dev, zes_zip_read_dev, zes_zip_read_alloc): hand-built archives at the smallest
shapes that matter — headers, names and bodies at every residue mod 16 (the fixture asserts it), names on either side of one workgroup pass (256 bytes), bodies on either side of one 64 KiB
piece — and one archive in which every kind of damage stands beside good entries.  Expected bytes
are the builder's inputs; expected statuses are the table of tests/_zip.py, checked there against the restated rule."""
import ctypes as C
import io
import zipfile

import numpy as np
import pytest

import _zip
import _zip_poison  # noqa: F401  (adds the ZIP entries to the poison catalogue, tests/_poison_cases.py)

pytestmark = pytest.mark.gpu


def dev(a, gpu, at=0):
    """The bytes on the device, starting `at` bytes into a 16-byte aligned tensor."""
    import torch

    t = torch.zeros(at + len(a), dtype=torch.uint8, device=gpu)
    t[at:] = torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy()).to(gpu)
    return t[at:]


@pytest.fixture(scope="module")
def standard(z, gpu):
    blob, plain, own = _zip.standard(lambda d: z.deflate_raw(np.frombuffer(d, dtype=np.uint8)).tobytes())
    ent, names = z.zip_index(blob)
    assert ent.size == len(plain) == 18 and sum(own) == 3 and len(blob) < 3 << 20
    # headers, the directory's names and bodies at every residue mod 16 over the tensor offsets the tests use
    assert _zip.OFFSETS == (0, 1, 7) and all(r == set(range(16)) for r in _zip.residues(blob))
    assert {1, 255, 256, 257, 1000} <= {int(e["name_len"]) for e in ent}
    assert min(int(e["csize"]) for e in ent) == 0 and max(int(e["csize"]) for e in ent) > 65536
    return blob, plain, own, ent


@pytest.fixture(scope="module")
def failure(z, gpu):
    blob, plan = _zip.failures()
    ent, _ = z.zip_index(blob)
    assert ent.size == len(plan)
    return blob, plan, ent


def offsets(ent, sel):
    """Unaligned, non-overlapping places for the selected entries: a gap of 1 to 13 bytes in front of each."""
    off, at = [], 0
    for i, k in enumerate(sel):
        at += 1 + (5 * i) % 13
        off.append(at)
        at += int(ent[k]["usize"])
    return off, at + 40


def dev_read(z, gpu, t, ent, sel=None, explicit=True, flags=0):
    """zes_zip_read_dev into a tensor filled with 0xA5 -> (statuses, out_len, off, the whole output on the host)."""
    import torch

    picked = list(range(ent.size)) if sel is None else list(sel)
    off, room = offsets(ent, picked)
    out = torch.full((room,), 0xA5, dtype=torch.uint8, device=gpu)
    s = np.ascontiguousarray(picked, dtype=np.uint32) if (explicit or sel is not None) else None
    got, off2, out_len, status = z.zip_read_tensor(t, ent, sel=s, out=out, off=off, flags=flags)
    return status, out_len, off, got.cpu().numpy()


def check(what, ent, picked, want, status, out_len, off, host, expect=None):
    """Every entry's status (expect[k], default 0), the bytes of those that check out, and 0xA5 everywhere outside the ranges."""
    untouched = np.ones(host.size, dtype=bool)
    for i, k in enumerate(picked):
        exp = 0 if expect is None else expect[k]
        assert status[i] == exp or (isinstance(exp, tuple) and status[i] in exp), (what, i, k, status[i], exp)
        assert out_len[i] == (int(ent[k]["usize"]) if status[i] == 0 else 0), (what, i, k)
        untouched[off[i]:off[i] + int(ent[k]["usize"])] = False
        if status[i] == 0:
            assert host[off[i]:off[i] + out_len[i]].tobytes() == want[k], (what, i, k)
    assert (host[untouched] == 0xA5).all(), what


def test_device_form_at_every_alignment(z, gpu, standard):
    blob, plain, own, ent = standard
    everyone = list(range(ent.size))
    for at in (0, 1, 7):
        t = dev(blob, gpu, at)
        check("sel NULL, file at %d" % at, ent, everyone, plain, *dev_read(z, gpu, t, ent, explicit=False))
    t = dev(blob, gpu, 7)
    for what, sel in (("reversed", everyone[::-1]), ("one entry", [11]), ("one stored entry", [16]), ("duplicates", [12, 3, 12, 16, 16, 0, 13, 0])):
        check(what, ent, sel, plain, *dev_read(z, gpu, t, ent, sel=sel))
    check("ZES_F_PIECES", ent, everyone, plain, *dev_read(z, gpu, t, ent, flags=z.ZES_F_PIECES))


def test_count_0_launches_nothing(z, gpu, standard):
    blob, plain, own, ent = standard
    t = dev(blob, gpu)
    z.set_profiling(True)
    try:
        check("one entry", ent, [4], plain, *dev_read(z, gpu, t, ent, sel=[4]))
        names = {name: n for name, _, n in z.last_kernel_times()}
        assert names.get("k_zip_stage") == 1 and names.get("k_crc32_seg") == 1, names
        status, out_len, off, host = dev_read(z, gpu, t, ent, sel=[])
        assert (status, out_len) == ([], []) and (host == 0xA5).all()
        assert z.last_kernel_times() == []
        check("stored entries only", ent, [13, 14, 15, 16, 17], plain, *dev_read(z, gpu, t, ent, sel=[13, 14, 15, 16, 17]))
        names = {name: n for name, _, n in z.last_kernel_times()}
        assert names == {"k_zip_stage": 1, "k_crc32_seg": 1}, names  # no decoder, no gather: the copy is the stage kernel's
    finally:
        z.set_profiling(False)


def test_failures_beside_successes(z, gpu, failure):
    blob, plan, ent = failure
    want = [p[2] for p in plan]
    expect = [p[1] for p in plan]
    everyone = list(range(ent.size))
    assert sum(1 for e in expect if e == 0) >= 6
    for at in (0, 3):
        check("failure archive at %d" % at, ent, everyone, want, *dev_read(z, gpu, dev(blob, gpu, at), ent), expect=expect)
    check("failure archive, reversed", ent, everyone[::-1], want, *dev_read(z, gpu, dev(blob, gpu, 5), ent, sel=everyone[::-1]), expect=expect)


def host_read(z, blob, ent, sel=None):
    """zes_zip_read_alloc -> (statuses, results by selection index, the allocator's calls)."""
    a = np.frombuffer(blob, dtype=np.uint8)
    cnt = ent.size if sel is None else len(sel)
    s = None if sel is None else np.ascontiguousarray(sel, dtype=np.uint32)
    got, calls = {}, []

    def alloc(_user, i, n):
        calls.append((int(i), int(n)))
        got[i] = np.full(int(n) + 16, 0xA5, dtype=np.uint8)
        return got[i].ctypes.data

    out_len = (C.c_uint64 * max(cnt, 1))()
    status = (C.c_int32 * max(cnt, 1))()
    rc = z.lib().zes_zip_read_alloc(a.ctypes.data, a.size, ent.ctypes.data, ent.size, s.ctypes.data if s is not None else None, cnt, z.ALLOC_FN(alloc),
                                    None, out_len, status, 0)
    assert rc == 0
    return list(status)[:cnt], list(out_len)[:cnt], got, calls


def test_host_form_matches_device_form(z, gpu, standard, failure):
    for what, (blob, want, ent, expect) in (("standard", (standard[0], standard[1], standard[3], None)),
                                            ("failure", (failure[0], [p[2] for p in failure[1]], failure[2], [p[1] for p in failure[1]]))):
        dstatus = dev_read(z, gpu, dev(blob, gpu, 1), ent)[0]
        for sel in (None, list(range(ent.size))[::-1], [2, 2, ent.size - 1]):
            picked = list(range(ent.size)) if sel is None else sel
            status, out_len, got, calls = host_read(z, blob, ent, sel)
            assert status == [dstatus[k] for k in picked], (what, sel)
            # alloc: once per entry that checks out, with its size, and never for another
            assert sorted(calls) == sorted((i, int(ent[k]["usize"])) for i, k in enumerate(picked) if status[i] == 0), (what, sel)
            for i, k in enumerate(picked):
                exp = 0 if expect is None else expect[k]
                assert status[i] == exp or (isinstance(exp, tuple) and status[i] in exp), (what, k)
                assert out_len[i] == (int(ent[k]["usize"]) if status[i] == 0 else 0)
                if status[i] == 0:
                    assert got[i][:out_len[i]].tobytes() == want[k] and (got[i][out_len[i]:] == 0xA5).all(), (what, k)
        res = z.zip_read(blob, (ent, None))
        assert [r.code if isinstance(r, z.ZlibEsError) else 0 for r in res] == dstatus, what
        assert all(r.tobytes() == want[k] for k, r in enumerate(res) if not isinstance(r, z.ZlibEsError)), what


def test_index_dev_equals_host_index(z, gpu):
    cases = [(what, b) for what, b in _zip.cpython_archives().items()] + [(what, v[0]) for what, v in _zip.reject_cases().items()]

    def index(fn):
        try:
            ent, names = fn()
        except z.ZlibEsError as e:
            return e.code, None, None
        return 0, ent.tobytes(), names

    for what, b in cases:
        want = index(lambda: z.zip_index(b))
        assert want[0] == _zip.index_rule(b)[0], what
        for at in (0, 3):
            assert index(lambda: z.zip_index_tensor(dev(b, gpu, at))) == want, (what, at)


def test_cpython_written_archive(z, gpu):
    f = io.BytesIO()
    plain = {}
    with zipfile.ZipFile(f, "w") as zf:
        for k in range(40):
            zi = zipfile.ZipInfo("gen/%02d.bin" % k)
            data = z.gen(("itext", "lowent4k", "xorshift")[k % 3], 900 + k, 37 * k * k + k).tobytes()
            zf.writestr(zi, data, compress_type=zipfile.ZIP_STORED if k % 4 == 3 else zipfile.ZIP_DEFLATED, compresslevel=(1, 6, 9, None)[k % 4])
    blob = f.getvalue()
    with zipfile.ZipFile(io.BytesIO(blob)) as zf:
        want = [zf.read(zi) for zi in zf.infolist()]
        levels = {zi.compress_type for zi in zf.infolist()}
    assert levels == {zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED} and len(want) == 40
    t = dev(blob, gpu, 1)
    ent, names = z.zip_index_tensor(t)
    assert names == [b"gen/%02d.bin" % k for k in range(40)]
    out, off, out_len, status = z.zip_read_tensor(t, ent)
    assert status == [0] * 40 and all(int(o) % 16 == 0 for o in off)
    host = out.cpu().numpy()
    assert [host[int(o):int(o) + n].tobytes() for o, n in zip(off, out_len)] == want
    assert [r.tobytes() for r in z.zip_read(blob, ent)] == want


def test_poisoned_scratch(z, gpu, standard, failure):
    sblob, plain, own, sent = standard
    fblob, plan, fent = failure
    ts, tf = dev(sblob, gpu, 1), dev(fblob, gpu, 3)
    for word in (0xFFFFFFFF, 0):
        z.stage_poison(word)
        check("standard, poison %#x" % word, sent, list(range(sent.size)), plain, *dev_read(z, gpu, ts, sent))
        z.stage_poison(word)
        check("failure, poison %#x" % word, fent, list(range(fent.size)), [p[2] for p in plan], *dev_read(z, gpu, tf, fent),
              expect=[p[1] for p in plan])
        z.stage_poison(word)
        assert host_read(z, fblob, fent)[0] == dev_read(z, gpu, tf, fent)[0]


def test_library_made_bodies_take_the_block_parallel_tier(z, gpu):
    datas = [z.gen("itext", 40 + k, n).tobytes() for k, n in enumerate((200000, 70000, 4096, 131072 + 5000))]
    entries = [_zip.entry(b"own/%d" % k, d, body=z.deflate_raw(np.frombuffer(d, dtype=np.uint8)).tobytes()) for k, d in enumerate(datas)]
    blob = _zip.build(entries)
    with zipfile.ZipFile(io.BytesIO(blob)) as zf:
        assert zf.testzip() is None
    t = dev(blob, gpu, 7)
    ent, _ = z.zip_index_tensor(t)
    out, off, out_len, status = z.zip_read_tensor(t, ent)
    assert status == [0] * 4 and z.last_inflate_tier() == 1
    host = out.cpu().numpy()
    assert [host[int(o):int(o) + n].tobytes() for o, n in zip(off, out_len)] == datas


def test_trim_gives_the_scratch_back(z, gpu, standard):
    blob, plain, own, ent = standard
    z.trim()
    before = z.pool_bytes()
    check("after trim", ent, list(range(ent.size)), plain, *dev_read(z, gpu, dev(blob, gpu), ent))
    assert len(z.zip_read(blob, ent)) == ent.size
    assert z.pool_bytes() > before
    z.trim()
    assert z.pool_bytes() == before
