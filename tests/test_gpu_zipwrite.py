"""The ZIP writer on the MI355X (zes_zipwrite_dev, zes_zipwrite): bit-exact with the archive that tests/_zip.py's builder and the
CPU oracle give (tests/_zipwrite.py) on the case list — entries on either side of the method rule, of one 64 KiB piece and of
one block, the lengths the encoder refuses, names of 0 and 300 bytes — as one archive and entry by entry, with the input and
the output at odd bytes of their tensors and canaries around the output."""
import ctypes as C
import io
import zipfile

import numpy as np
import pytest

import _zip
import _zipwrite as W
import _zipwrite_poison  # noqa: F401  (adds the writer's entries to the poison catalogue, tests/_poison_cases.py)

pytestmark = pytest.mark.gpu

IN_AT, OUT_AT, TAIL = 3, 5, 40  # the input at byte 3 and the output at byte 5 of their 16-byte aligned tensors; canary bytes behind


class Case:
    """A list of entries on the device: every entry's bytes once (equal data shares its place, so entries repeat), back to
    back without padding behind IN_AT bytes, and the archive expected for them."""

    def __init__(self, gpu, entries):
        import torch

        self.entries, self.at, blob = entries, {}, bytearray()
        for _, d in entries:
            if d not in self.at:
                self.at[d] = len(blob)
                blob += d
        self.t = torch.zeros(IN_AT + len(blob), dtype=torch.uint8, device=gpu)
        if blob:
            self.t[IN_AT:] = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(gpu)
        self.want = W.expect(entries)

    def sub(self, ks):
        """The entries ks as a case of their own, on the same tensor."""
        c = Case.__new__(Case)
        c.entries, c.at, c.t = [self.entries[k] for k in ks], self.at, self.t
        c.want = W.expect(c.entries)
        return c


@pytest.fixture(scope="module")
def whole(z, gpu):
    c = Case(gpu, W.cases(z))
    assert len({c.at[d] % 16 for _, d in c.entries}) >= 8  # the entries' bytes lie at many residues mod 16
    return c


def dev_write(z, gpu, c, cap=None, flags=0, null_out=False):
    """zes_zipwrite_dev into a tensor filled with 0xA5, OUT_AT bytes in -> (rc, out_len, the whole tensor on the host, ent)."""
    import torch

    es = c.entries
    room = W.bound(es) if cap is None else cap
    out = torch.full((OUT_AT + room + TAIL,), 0xA5, dtype=torch.uint8, device=gpu)
    off = np.array([c.at[d] for _, d in es], dtype=np.uint64)
    ln = np.array([len(d) for _, d in es], dtype=np.uint64)
    blob, nl = W.names_arrays(es)
    ent = np.zeros(max(len(es), 1), dtype=z.ZIP_ENTRY)
    n = C.c_uint64(77)
    torch.cuda.synchronize()
    rc = z.lib().zes_zipwrite_dev(c.t.data_ptr() + IN_AT, W.ptr(off), W.ptr(ln), W.ptr(blob), W.ptr(nl), len(es),
                                  None if null_out else out.data_ptr() + OUT_AT, room, C.byref(n), ent.ctypes.data, flags)
    return rc, n.value, out.cpu().numpy(), ent[:len(es)]


def exact(what, c, rc, n, host, ent):
    """The call wrote the expected archive between its canaries, and ent is the index of it."""
    assert (rc, n) == (0, len(c.want)), (what, rc, n, len(c.want))
    got = host[OUT_AT:OUT_AT + n].tobytes()
    if got != c.want:
        k = next(i for i in range(n) if got[i] != c.want[i])
        raise AssertionError("%s: first difference at byte %d of %d" % (what, k, n))
    assert (host[:OUT_AT] == 0xA5).all() and (host[OUT_AT + n:] == 0xA5).all(), what
    W.same_as_index(ent, c.want)


def test_device_form_is_bit_exact(z, gpu, whole):
    rc, n, host, ent = dev_write(z, gpu, whole)
    exact("the case list", whole, rc, n, host, ent)
    zent, znames = z.zip_index(host[OUT_AT:OUT_AT + n])
    assert zent.tobytes() == ent.tobytes() and znames == [name for name, _ in whole.entries]
    # an exact capacity, and the same bytes in groups of four
    exact("cap == size", whole, *dev_write(z, gpu, whole, cap=len(whole.want)))
    exact("ZES_F_PIECES", whole, *dev_write(z, gpu, whole, flags=z.ZES_F_PIECES))


def test_entry_by_entry(z, gpu, whole):
    for k, (name, d) in enumerate(whole.entries):
        c = whole.sub([k])
        exact("entry %d, %r of %d bytes" % (k, name[:20], len(d)), c, *dev_write(z, gpu, c))


def test_nine_entries_in_groups_of_four(z, gpu):
    c = Case(gpu, W.nine(z))
    z.set_profiling(True)
    try:
        exact("nine entries, ZES_F_PIECES", c, *dev_write(z, gpu, c, flags=z.ZES_F_PIECES))
        times = {name: n for name, _, n in z.last_kernel_times()}
        assert times.get("k_zip_pack") == 3 and times.get("k_crc32_seg") == 3, times  # a launch per group, none per entry
        exact("nine entries", c, *dev_write(z, gpu, c))
        times = {name: n for name, _, n in z.last_kernel_times()}
        assert times.get("k_zip_pack") == 1 and times.get("k_crc32_seg") == 1 and max(times.values()) < len(c.entries), times
    finally:
        z.set_profiling(False)


def test_groups_that_end_at_their_slots(z, gpu, whole):
    """Under ZES_F_PIECES a group's encoder slots take up to 1 MiB: two entries of 300000 bytes do not share one, so groups end
    before they hold four entries and a call has more groups than its entry count alone makes."""
    c = Case(gpu, W.slots(z))
    want = W.groups(c.entries, z.ZES_F_PIECES)
    assert want == [2, 2, 2] and len(want) > (len(c.entries) + 3) // 4
    z.set_profiling(True)
    try:
        exact("six entries, ZES_F_PIECES", c, *dev_write(z, gpu, c, flags=z.ZES_F_PIECES))
        times = {name: n for name, _, n in z.last_kernel_times()}
        assert times.get("k_zip_pack") == len(want) and times.get("k_crc32_seg") == len(want), times
        # the case list: one of its groups ends at its slots too
        want = W.groups(whole.entries, z.ZES_F_PIECES)
        assert min(want[:-1]) < 4 and max(want) == 4
        exact("the case list, ZES_F_PIECES", whole, *dev_write(z, gpu, whole, flags=z.ZES_F_PIECES))
        assert {name: n for name, _, n in z.last_kernel_times()}.get("k_zip_pack") == len(want)
    finally:
        z.set_profiling(False)
    rc, n, out, ent = W.host_write(z, c.entries, flags=z.ZES_F_PIECES)
    assert (rc, n) == (0, len(c.want)) and out[:n].tobytes() == c.want and (out[n:] == 0xA5).all()
    W.same_as_index(ent, c.want)
    # three entries, each a group of its own: what the entry count alone would take for one group
    c3 = c.sub([0, 2, 5])
    assert W.groups(c3.entries, z.ZES_F_PIECES) == [1, 1, 1]
    exact("three groups of one", c3, *dev_write(z, gpu, c3, flags=z.ZES_F_PIECES))


def test_nospace_and_size_query(z, gpu, whole):
    need = len(whole.want)
    for cap in (need - 1, need - 22, 1000, 0):
        rc, n, host, _ = dev_write(z, gpu, whole, cap=cap)
        assert (rc, n) == (_zip.ZES_E_NOSPACE, need), (cap, rc, n)
        assert (host[:OUT_AT] == 0xA5).all() and (host[OUT_AT + cap:] == 0xA5).all(), cap  # nothing at or behind cap
    rc, n, host, _ = dev_write(z, gpu, whole, cap=0, null_out=True)
    assert (rc, n) == (_zip.ZES_E_NOSPACE, need) and (host == 0xA5).all()
    empty = Case(gpu, [])
    rc, n, host, _ = dev_write(z, gpu, empty)
    assert (rc, n) == (0, 22) and host[OUT_AT:OUT_AT + 22].tobytes() == W.expect([]) and (host[OUT_AT + 22:] == 0xA5).all()


def test_the_reader_and_zipfile_extract_the_result(z, gpu, whole):
    view, (ent, names) = z.zip_write_tensor(whole.t[IN_AT:], [whole.at[d] for _, d in whole.entries], [len(d) for _, d in whole.entries],
                                           [n for n, _ in whole.entries])
    assert view.cpu().numpy().tobytes() == whole.want and names == [n for n, _ in whole.entries]
    out, off, out_len, status = z.zip_read_tensor(view, ent)
    assert status == [0] * len(whole.entries)
    host = out.cpu().numpy()
    assert [host[int(o):int(o) + n].tobytes() for o, n in zip(off, out_len)] == [d for _, d in whole.entries]
    with zipfile.ZipFile(io.BytesIO(view.cpu().numpy().tobytes())) as zf:
        assert zf.testzip() is None and [zf.read(zi) for zi in zf.infolist()] == [d for _, d in whole.entries]


def test_host_form(z, gpu, whole):
    es = whole.entries
    need = len(whole.want)
    rc, n, out, ent = W.host_write(z, es)
    assert (rc, n) == (0, need) and out[:n].tobytes() == whole.want and (out[n:] == 0xA5).all()
    W.same_as_index(ent, whole.want)
    rc, n, out, ent = W.host_write(z, es, cap=need, flags=z.ZES_F_PIECES, want_ent=False)
    assert (rc, n) == (0, need) and out[:n].tobytes() == whole.want and (out[n:] == 0xA5).all()
    rc, n, out, ent = W.host_write(z, es, cap=need - 1)
    assert (rc, n) == (_zip.ZES_E_NOSPACE, need) and (out == 0xA5).all() and not ent.tobytes().strip(b"\0")
    assert W.host_write(z, es, cap=0, null_out=True)[:2] == (_zip.ZES_E_NOSPACE, need)
    for k in (0, 3, 8, 13, 15, len(es) - 1):  # a few entries alone: stored and deflated, the longest, a refused length
        rc, n, out, ent = W.host_write(z, [es[k]])
        assert (rc, out[:n].tobytes()) == (0, W.expect([es[k]])), k
    arch, (ent, names) = z.zip_write(es)
    assert arch.tobytes() == whole.want and names == [n for n, _ in es]
    W.same_as_index(ent, whole.want)
    assert [r.tobytes() for r in z.zip_read(arch, ent)] == [d for _, d in es]


def test_poisoned_scratch_and_trim(z, gpu):
    c = Case(gpu, W.nine(z))
    for word in (0xFFFFFFFF, 0):
        z.stage_poison(word)
        exact("poison %#x" % word, c, *dev_write(z, gpu, c, flags=z.ZES_F_PIECES))
        z.stage_poison(word)
        assert W.host_write(z, c.entries)[2][:len(c.want)].tobytes() == c.want
    z.trim()
    before = z.pool_bytes()
    exact("after trim", c, *dev_write(z, gpu, c))
    assert z.pool_bytes() > before
    z.trim()
    assert z.pool_bytes() == before
