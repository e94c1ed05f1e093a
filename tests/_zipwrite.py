"""The archive zes_zipwrite* must write (include/zes.h), built from tests/_zip.py's builder with its default fields and the CPU
oracle, never from the library: the method rule restated, the case list the CPU and the GPU tests share, and the calls through
the C-ABI that both use.  Plain Python, no GPU.

The rule: let s be the oracle's raw stream of the entry's bytes alone.  Method 8 with body s when the encoder accepts the
length (not 0, not 1, not = 1 mod 131072) and len(s) < len; otherwise method 0 with the bytes themselves.  The name's flag is
0x0800 when it holds a byte >= 0x80.

A stream exactly as long as its data ("is not kept": stored): the oracle has such cases.  Searched over `itext` (seed 7) and
zero bytes of every length 2 .. 4096 it gives 14 zero bytes (a stream of 14) and text of 39, 43 and 45 bytes; they are EXACT
below and part of the case list.  test_zipwrite_cpu.py runs the search again over lengths 2 .. 64, where they all lie, so the
list cannot go stale."""
import ctypes as C
import functools

import numpy as np

import _oracle
import _zip

BLK = 131072
PIECES = 4  # ZES_F_PIECES
TEXT_LENGTHS = (2, 24, 32, 48, 64, 1000, 131072, 131074, 300000)
XORSHIFT_LENGTHS = (64, 4096, 131072)
THROW_LENGTHS = (0, 1, 131073, 262145)
ZERO_LENGTHS = (8, 64)


def throws(n):
    return n == 0 or n == 1 or n % BLK == 1


def name_flags(name):
    return 0x0800 if any(b >= 0x80 for b in name) else 0


@functools.lru_cache(maxsize=None)
def _body(data):
    """(method, body) of an entry's bytes under the rule."""
    if not throws(len(data)):
        s = _oracle.deflate_raw(np.frombuffer(data, dtype=np.uint8)).tobytes()
        if len(s) < len(data):
            return 8, s
    return 0, data


def entry(name, data):
    data = bytes(data)
    method, body = _body(data)
    return _zip.entry(bytes(name), data, method=method, body=body, flags=name_flags(name))


def expect(entries):
    """The archive of [(name, data)]."""
    return _zip.build([entry(n, d) for n, d in entries])


def bound(entries):
    return sum(30 + len(n) + len(d) for n, d in entries) + sum(46 + len(n) for n, d in entries) + 22


def exact_search(z, lengths):
    """[(kind, n)] over text and zero bytes of the given lengths whose raw stream has exactly n bytes."""
    out = []
    for n in lengths:
        for kind, data in (("itext", z.gen("itext", 7, n)), ("zeros", np.zeros(n, dtype=np.uint8))):
            if not throws(n) and _oracle.deflate_raw(data).size == n:
                out.append((kind, n))
    return out


EXACT = (("zeros", 14), ("itext", 39), ("itext", 43), ("itext", 45))  # exact_search(z, range(2, 4097))


@functools.lru_cache(maxsize=None)
def _cases(z):
    gen = lambda kind, seed, n: z.gen(kind, seed, n).tobytes()
    out = []
    for n in TEXT_LENGTHS:
        out.append((b"text/%d.txt" % n, gen("itext", 300 + n % 97, n)))
    for n in XORSHIFT_LENGTHS:
        out.append((b"random/%d.bin" % n, gen("xorshift", 400 + n % 97, n)))
    for n in THROW_LENGTHS:
        out.append((b"refused/%d" % n, gen("itext", 500 + n % 97, n)))
    for n in ZERO_LENGTHS:
        out.append((b"zero/%d" % n, bytes(n)))
    for kind, n in EXACT:
        out.append((b"exact/%s-%d" % (kind.encode(), n), bytes(n) if kind == "zeros" else gen("itext", 7, n)))
    out.append(("grüß/日本.txt".encode("utf-8"), gen("itext", 601, 700)))
    out.append((b"", gen("itext", 602, 90)))
    out.append(((b"long/" + b"n" * 300)[:300], gen("itext", 603, 5000)))
    same = gen("itext", 604, 20000)
    out.append((b"same/one", same))
    out.append((b"same/two", same))
    return tuple(out)


def cases(z):
    """[(name, data)]: the case list.  No entry is larger than 300000 bytes."""
    return list(_cases(z))


def nine(z):
    """Nine entries for ZES_F_PIECES: groups of four meet twice and the last group holds one."""
    c = {n: d for n, d in cases(z)}
    pick = [b"text/1000.txt", b"random/4096.bin", b"refused/1", b"text/131074.txt", b"zero/64", b"refused/131073", b"text/48.txt", b"", b"text/300000.txt"]
    return [(n, c[n]) for n in pick]


def slots(z):
    """Six entries whose groups under ZES_F_PIECES end at the 1 MiB of encoder slots, not at four entries: three groups of
    two (groups() says so), where the entry count alone would make two."""
    c = {n: d for n, d in cases(z)}
    big = c[b"text/300000.txt"]
    return [(b"slots/a", big), (b"slots/1000", c[b"text/1000.txt"]), (b"slots/b", big), (b"slots/131074", c[b"text/131074.txt"]),
            (b"slots/131072", c[b"text/131072.txt"]), (b"slots/c", big)]


def groups(entries, flags=0):
    """The group rule of include/zes.h restated -> the groups' entry counts: up to 1024 entries whose encoder slots take up
    to 256 MiB (4 entries and 1 MiB under ZES_F_PIECES), one entry at least.  A slot is zes_deflate_bound of the length,
    rounded up to 16; a length the encoder refuses has none."""
    most, room = (4, 1 << 20) if flags & PIECES else (1024, 256 << 20)
    slot = lambda n: 0 if throws(n) else ((BLK if n < BLK // 2 else 2 * n) + 6 + 15) // 16 * 16
    out, cnt, used = [], 0, 0
    for _, d in entries:
        if cnt and (cnt == most or used + slot(len(d)) > room):
            out.append(cnt)
            cnt, used = 0, 0
        cnt += 1
        used += slot(len(d))
    return out + ([cnt] if cnt else [])


def want_methods(z):
    """What the issue states about the case list, checked against the oracle by the CPU test: name -> method."""
    w = {}
    for n in TEXT_LENGTHS:
        w[b"text/%d.txt" % n] = 0 if n <= 32 else 8
    for n in XORSHIFT_LENGTHS:
        w[b"random/%d.bin" % n] = 0
    for n in THROW_LENGTHS:
        w[b"refused/%d" % n] = 0
    w[b"zero/8"], w[b"zero/64"] = 0, 8
    for kind, n in EXACT:
        w[b"exact/%s-%d" % (kind.encode(), n)] = 0
    return w


# ---- the calls ----
FIELDS = ("hdr_off", "name_pos", "csize", "usize", "crc", "name_off", "name_len", "method", "flags", "pad")


def names_arrays(entries):
    blob = np.frombuffer(b"".join(n for n, _ in entries), dtype=np.uint8)
    return blob, np.array([len(n) for n, _ in entries], dtype=np.uint16)


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def host_write(z, entries, cap=None, flags=0, want_ent=True, out_len=True, null_in=None, null_out=False, lens=None, names=True,
               name_len=True, in_len=True, ptrs=True):
    """zes_zipwrite -> (rc, out_len, the out buffer filled with 0xA5 beforehand, ent).  The keyword arguments take single
    arguments away or replace them, for the argument tests."""
    datas = [np.frombuffer(bytes(d), dtype=np.uint8) for _, d in entries]
    blob, nl = names_arrays(entries)
    cnt = len(entries)
    ln = np.array([d.size for d in datas] if lens is None else lens, dtype=np.uint64)
    if cap is None:
        cap = bound(entries)
    out = np.full(cap + 16, 0xA5, dtype=np.uint8)
    ent = np.zeros(max(cnt, 1), dtype=z.ZIP_ENTRY)
    p = (C.c_void_p * max(len(datas), 1))(*[None if (null_in is not None and i == null_in) else (d.ctypes.data if d.size else None)
                                            for i, d in enumerate(datas)])
    n = C.c_uint64(77)
    rc = z.lib().zes_zipwrite(p if ptrs else None, ptr(ln) if in_len else None, ptr(blob) if names else None, ptr(nl) if name_len else None, cnt,
                              None if null_out else out.ctypes.data, cap, C.byref(n) if out_len else None, ent.ctypes.data if want_ent else None, flags)
    return rc, n.value, out, ent[:cnt]


def same_as_index(ent, blob):
    """ent is what the restated index rule lists for blob, field by field."""
    st, want, _ = _zip.index_rule(blob)
    assert st == 0 and len(want) == ent.size
    for e, w in zip(ent, want):
        assert {f: int(e[f]) for f in FIELDS} == w
