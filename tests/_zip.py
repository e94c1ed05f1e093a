"""ZIP archives for the tests of zes_zip_index* / zes_zip_read*: a builder that puts an archive together from parts (so that
every field can be made to lie), a Python restatement of the two rules of include/zes.h (the index rule, an entry's status),
and the case lists the CPU and the GPU tests share."""
import io
import struct
import zipfile
import zlib

ZES_E_CHECKSUM, ZES_E_ZIP, ZES_E_UNSUPPORTED, ZES_E_NOSPACE, ZES_E_ARG, ZES_E_DEVICE = -21, -22, -23, -16, -18, -17
INFLATE = "the body's inflate status"  # entry_rule: the body does not decode; which status that is, is the inflate tiers' business
INFLATE_STATUSES = (-1, -2, -3, -4, -5)


def raw_body(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(data) + co.flush()


def entry(name, data=b"", method=8, level=6, body=None, flags=0, extra=b"", descriptor=False, usize=None, crc=None, spare=b"", local=None,
          central=None):
    """One entry.  body: the stored bytes (default: `data` itself for method 0, CPython's raw DEFLATE at `level` else);
    descriptor: flag bit 3, the local header's CRC and sizes zero and a data descriptor behind the body; spare: bytes behind the
    body that belong to nothing; local / central: fields of the two records set to other values (keys as in build())."""
    if body is None:
        body = data if method == 0 else raw_body(data, level)
    return dict(name=name, data=data, method=method, body=body, flags=flags | (8 if descriptor else 0), extra=extra, descriptor=descriptor,
                usize=len(data) if usize is None else usize, crc=zlib.crc32(data) if crc is None else crc, spare=spare, local=dict(local or {}),
                central=dict(central or {}))


LOCAL_FIELDS = ("sig", "ver", "flags", "method", "time", "date", "crc", "csize", "usize", "nlen", "elen")
CENTRAL_FIELDS = ("sig", "made", "ver", "flags", "method", "time", "date", "crc", "csize", "usize", "nlen", "elen", "clen", "disk", "iattr", "eattr",
                  "offset")
END_FIELDS = ("sig", "disk", "cd_disk", "count_disk", "count", "cd_size", "cd_off", "clen")


def build(entries, prefix=b"", comment=b"", end=None, cd_pad=b"", cd_tail=b"", trailer=b""):
    """The archive's bytes.  prefix: in front of the archive (the offsets do not count it, as for a self-extractor); cd_pad:
    bytes behind the last record that the directory's size counts; cd_tail: bytes between directory and end record that it
    does not count; trailer: bytes behind the end record's comment; end: end record fields set to other values."""
    out = io.BytesIO()
    out.write(prefix)
    offs = []
    for e in entries:
        offs.append(out.tell() - len(prefix))
        f = dict(sig=0x04034B50, ver=20, flags=e["flags"], method=e["method"], time=0, date=33, crc=0 if e["descriptor"] else e["crc"],
                 csize=0 if e["descriptor"] else len(e["body"]), usize=0 if e["descriptor"] else e["usize"], nlen=len(e["name"]), elen=len(e["extra"]))
        name = e["local"].get("name", e["name"])
        f.update({k: v for k, v in e["local"].items() if k != "name"})
        out.write(struct.pack("<IHHHHHIIIHH", *[f[k] for k in LOCAL_FIELDS]) + name + e["extra"] + e["body"])
        if e["descriptor"]:
            out.write(struct.pack("<IIII", 0x08074B50, e["crc"], len(e["body"]), e["usize"]))
        out.write(e["spare"])
    cd_off = out.tell() - len(prefix)
    for e, off in zip(entries, offs):
        f = dict(sig=0x02014B50, made=20, ver=20, flags=e["flags"], method=e["method"], time=0, date=33, crc=e["crc"], csize=len(e["body"]),
                 usize=e["usize"], nlen=len(e["name"]), elen=0, clen=0, disk=0, iattr=0, eattr=0, offset=off)
        f.update({k: v for k, v in e["central"].items() if k not in ("name", "extra", "comment")})
        ex, cm = e["central"].get("extra", b""), e["central"].get("comment", b"")
        if "elen" not in e["central"]:
            f["elen"] = len(ex)
        if "clen" not in e["central"]:
            f["clen"] = len(cm)
        out.write(struct.pack("<IHHHHHHIIIHHHHHII", *[f[k] for k in CENTRAL_FIELDS]) + e["central"].get("name", e["name"]) + ex + cm)
    out.write(cd_pad)
    cd_size = out.tell() - len(prefix) - cd_off
    out.write(cd_tail)
    f = dict(sig=0x06054B50, disk=0, cd_disk=0, count_disk=len(entries), count=len(entries), cd_size=cd_size, cd_off=cd_off, clen=len(comment))
    f.update(end or {})
    out.write(struct.pack("<IHHHHIIH", *[f[k] for k in END_FIELDS]) + comment + trailer)
    return out.getvalue()


# ---- the rules of include/zes.h, restated ----
def le16(b, i):
    return b[i] | b[i + 1] << 8


def le32(b, i):
    return b[i] | b[i + 1] << 8 | b[i + 2] << 16 | b[i + 3] << 24


def index_rule(b):
    """zes_zip_index on the bytes b -> (status, entries, names): entries as dicts with zes_zip_entry's fields."""
    c = len(b)
    if c < 22:
        return ZES_E_ZIP, [], []
    p = c - 22
    while True:
        if b[p:p + 4] == b"PK\x05\x06" and p + 22 + le16(b, p + 20) == c:
            break
        if p == 0 or p == c - 22 - 65535:
            return ZES_E_ZIP, [], []
        p -= 1
    count, cd_size, cd_off = le16(b, p + 10), le32(b, p + 12), le32(b, p + 16)
    if le16(b, p + 4) or le16(b, p + 6) or le16(b, p + 8) != count or count == 0xFFFF or cd_size == 0xFFFFFFFF or cd_off == 0xFFFFFFFF:
        return ZES_E_UNSUPPORTED, [], []
    if p >= 20 and b[p - 20:p - 16] == b"PK\x06\x07":
        return ZES_E_UNSUPPORTED, [], []
    if cd_size + cd_off > p:
        return ZES_E_ZIP, [], []
    base = p - cd_size - cd_off
    at, ent, names = base + cd_off, [], []
    while at < p:
        if p - at < 46 or b[at:at + 4] != b"PK\x01\x02":
            return ZES_E_ZIP, [], []
        nlen = le16(b, at + 28)
        size = 46 + nlen + le16(b, at + 30) + le16(b, at + 32)
        if size > p - at:
            return ZES_E_ZIP, [], []
        csize, usize, off = le32(b, at + 20), le32(b, at + 24), le32(b, at + 42)
        if 0xFFFFFFFF in (csize, usize, off) or le16(b, at + 34):
            return ZES_E_UNSUPPORTED, [], []
        if off + 30 > cd_off:
            return ZES_E_ZIP, [], []
        ent.append(dict(hdr_off=base + off, name_pos=at + 46, csize=csize, usize=usize, crc=le32(b, at + 16), name_off=sum(len(n) for n in names),
                        name_len=nlen, method=le16(b, at + 10), flags=le16(b, at + 8), pad=0))
        names.append(bytes(b[at + 46:at + 46 + nlen]))
        at += size
    if len(ent) != count:
        return ZES_E_ZIP, [], []
    return 0, ent, names


def entry_rule(b, e):
    """An entry's status and bytes under zes_zip_read*'s rule -> (status, bytes or None); status INFLATE when the body does not
    decode (the status is then the inflate tiers')."""
    c = len(b)
    if (e["flags"] & 0x61) or e["method"] not in (0, 8):
        return ZES_E_UNSUPPORTED, None
    if e["method"] == 0 and e["csize"] != e["usize"]:
        return ZES_E_ZIP, None
    h = e["hdr_off"]
    if h + 30 > c or e["name_pos"] + e["name_len"] > c:
        return ZES_E_ZIP, None
    nlen, elen = le16(b, h + 26), le16(b, h + 28)
    if b[h:h + 4] != b"PK\x03\x04" or le16(b, h + 8) != e["method"] or (b[h + 6] & 1) != (e["flags"] & 1) or nlen != e["name_len"]:
        return ZES_E_ZIP, None
    if h + 30 + nlen + elen + e["csize"] > c or b[h + 30:h + 30 + nlen] != b[e["name_pos"]:e["name_pos"] + nlen]:
        return ZES_E_ZIP, None
    body = bytes(b[h + 30 + nlen + elen:h + 30 + nlen + elen + e["csize"]])
    if e["method"] == 8:
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(body)
        except zlib.error:
            return INFLATE, None
        if not d.eof:
            return INFLATE, None
        if len(out) != e["usize"] or d.unused_data:
            return ZES_E_CHECKSUM, None
    else:
        out = body
    return (0, out) if zlib.crc32(out) == e["crc"] else (ZES_E_CHECKSUM, None)


# ---- archives CPython writes (the index tests) ----
class Unseekable(io.RawIOBase):
    def __init__(self):
        self.buf = io.BytesIO()

    def writable(self):
        return True

    def write(self, b):
        return self.buf.write(b)

    def flush(self):
        pass


def text(n, seed):
    """n bytes that compress (no GPU, no library: the CPU tests build their inputs with this)."""
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"eta", b"theta"]
    out, x = bytearray(), (seed * 2654435761 + 1) & 0xFFFFFFFF
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out += words[(x >> 16) % 8] + (b" " if x & 4 else b"\n")
    return bytes(out[:n])


def cpython_archives():
    """name -> bytes: archives written by CPython's zipfile, one per way it has of writing them."""
    def deflated(name, date_time=(1980, 1, 1, 0, 0, 0)):
        zi = zipfile.ZipInfo(name, date_time)
        zi.compress_type = zipfile.ZIP_DEFLATED
        return zi

    items = [("a.txt", text(3000, 1)), ("dir/b.bin", text(70000, 2)), ("empty", b"")]
    out = {}
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, data in items:
            zf.writestr(deflated(name), data)
        zf.comment = b"a comment of some length"
    out["seekable with a comment"] = f.getvalue()
    u = Unseekable()
    with zipfile.ZipFile(u, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, data in items:
            zf.writestr(deflated(name), data)
    out["unseekable, bit 3"] = u.buf.getvalue()
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, data in items:
            with zf.open(deflated(name), "w", force_zip64=True) as w:
                w.write(data)
    out["force_zip64"] = f.getvalue()
    out["a 100-byte prefix"] = bytes(range(100)) + out["seekable with a comment"]
    f = io.BytesIO()
    zipfile.ZipFile(f, "w").close()
    out["no entries"] = f.getvalue()
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", zipfile.ZIP_DEFLATED) as zf:
        zf.writestr(deflated("plain"), items[0][1])
        zi = zipfile.ZipInfo("bz")
        zi.compress_type = zipfile.ZIP_BZIP2
        zf.writestr(zi, items[0][1])
    out["a bzip2 entry"] = f.getvalue()
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", zipfile.ZIP_DEFLATED) as zf:
        zf.writestr(deflated("grüß/日本.txt"), items[0][1])
        zf.writestr(deflated("ascii.txt"), items[0][1])
    out["a UTF-8 name"] = f.getvalue()
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in range(300):
            zf.writestr(deflated("many/%03d" % k), text(10 + k, k))
    out["300 entries"] = f.getvalue()
    return out


def infolist(b):
    """What CPython's zipfile lists: dicts with the fields the index shares with it."""
    with zipfile.ZipFile(io.BytesIO(b)) as zf:
        return [dict(hdr_off=zi.header_offset, csize=zi.compress_size, usize=zi.file_size, crc=zi.CRC, method=zi.compress_type, flags=zi.flag_bits,
                     name=zi.orig_filename) for zi in zf.infolist()]


# ---- the reject list of the index (exact statuses) ----
def reject_cases():
    """name -> (bytes, status, entries when the status is 0)."""
    es = [entry(b"one", text(500, 3)), entry(b"two", text(900, 4), method=0)]
    good = build(es)
    n = len(es)
    cd_off = le32(good, len(good) - 22 + 16)

    def cen(k, **kw):
        return [entry(e["name"], e["data"], method=e["method"], central=kw if i == k else None) for i, e in enumerate(es)]

    cases = {
        "c == 0": (b"", ZES_E_ZIP, 0),
        "c == 21": (good[-21:], ZES_E_ZIP, 0),
        "no signature": (bytes(100), ZES_E_ZIP, 0),
        "5 bytes behind the end record": (build(es, trailer=b"\0" * 5), ZES_E_ZIP, 0),
        "a comment that holds the signature": (build(es[:1], comment=b"PK\x05\x06" + bytes(range(1, 40))), 0, 1),
        "cd_size + cd_off > p": (build(es, end=dict(cd_off=cd_off + 1)), ZES_E_ZIP, 0),
        "a damaged record signature": (build(cen(1, sig=0x02014B51)), ZES_E_ZIP, 0),
        "a record cut by the directory's end": (build(cen(1, clen=10)), ZES_E_ZIP, 0),
        "records that end early": (build(es, cd_pad=bytes(50)), ZES_E_ZIP, 0),
        "records that end 4 bytes early": (build(es, cd_pad=bytes(4)), ZES_E_ZIP, 0),
        "a count one too high": (build(es, end=dict(count=n + 1, count_disk=n + 1)), ZES_E_ZIP, 0),
        "a count one too low": (build(es, end=dict(count=n - 1, count_disk=n - 1)), ZES_E_ZIP, 0),
        "hdr_off + 30 beyond the directory start": (build(cen(1, offset=cd_off - 10)), ZES_E_ZIP, 0),
        "disk number": (build(es, end=dict(disk=1)), ZES_E_UNSUPPORTED, 0),
        "directory's disk number": (build(es, end=dict(cd_disk=1)), ZES_E_UNSUPPORTED, 0),
        "the two counts differ": (build(es, end=dict(count_disk=n - 1)), ZES_E_UNSUPPORTED, 0),
        "a count of 0xFFFF": (build(es, end=dict(count=0xFFFF, count_disk=0xFFFF)), ZES_E_UNSUPPORTED, 0),
        "a directory size of 0xFFFFFFFF": (build(es, end=dict(cd_size=0xFFFFFFFF)), ZES_E_UNSUPPORTED, 0),
        "a directory offset of 0xFFFFFFFF": (build(es, end=dict(cd_off=0xFFFFFFFF)), ZES_E_UNSUPPORTED, 0),
        "a ZIP64 locator": (build(es, cd_tail=b"PK\x06\x07" + bytes(16)), ZES_E_UNSUPPORTED, 0),
        "a record's csize of 0xFFFFFFFF": (build(cen(0, csize=0xFFFFFFFF)), ZES_E_UNSUPPORTED, 0),
        "a record's usize of 0xFFFFFFFF": (build(cen(1, usize=0xFFFFFFFF)), ZES_E_UNSUPPORTED, 0),
        "a record's offset of 0xFFFFFFFF": (build(cen(1, offset=0xFFFFFFFF)), ZES_E_UNSUPPORTED, 0),
        "a record's disk number": (build(cen(0, disk=2)), ZES_E_UNSUPPORTED, 0),
        # the longest comment: the 20 bytes in front of the end record lie outside the file's last 65557 bytes
        "the longest comment": (build(es, comment=bytes(65535)), 0, n),
        "a ZIP64 locator in front of the longest comment": (build(es, cd_tail=b"PK\x06\x07" + bytes(16), comment=bytes(65535)), ZES_E_UNSUPPORTED, 0),
    }
    for name, (b, status, cnt) in cases.items():
        got = index_rule(b)
        assert (got[0], len(got[1])) == (status, cnt), (name, got[0], len(got[1]))
    return cases


# ---- the archives of the read tests ----
def standard(lib_body=None):
    """The standard archive -> (bytes, [the entries' plain bytes], [whether an entry's body is the library's own]).  Its headers, its
    bodies and the directory's names lie at every residue mod 16 over OFFSETS, whatever the bodies' lengths: the free names'
    lengths are chosen for that, and it is asserted.
    lib_body(data) -> the library's deflate_raw of data; None: CPython's level 6 stands in (the CPU tests)."""
    fixed = lambda d: raw_body(d, 6, zlib.Z_FIXED)
    lib = lib_body or (lambda d: raw_body(d, 6))
    #        size    body                         name length (None: chosen below)  extra  bit 3
    plan = [(0, lambda d: raw_body(d, 6), None, 0, False),
            (1, lambda d: raw_body(d, 9), 1, 20, False),
            (15, fixed, None, 0, False),
            (16, lib, 255, 0, False),
            (17, lambda d: raw_body(d, 1), None, 20, False),
            (33, lambda d: raw_body(d, 0), 256, 0, False),
            (4096, lib, None, 0, False),
            (5000, lambda d: raw_body(d, 6), None, 20, True),
            (65535, lambda d: raw_body(d, 9), 257, 0, False),
            (65536, lambda d: raw_body(d, 1), None, 0, False),
            (65537, lambda d: raw_body(d, 6), None, 20, False),
            (200000, lib, 1000, 0, False),
            (300000, lambda d: raw_body(d, 6), None, 0, False),
            (0, None, None, 0, False),
            (1, None, None, 20, False),
            (17, None, None, 0, True),
            (65537, None, None, 0, False),
            (70000, None, None, 20, False)]
    made = [(text(size, 100 + k), None) for k, (size, *_rest) in enumerate(plan)]
    made = [(d, None if p[1] is None else p[1](d)) for (d, _), p in zip(made, plan)]
    for turn in range(16):  # (the first layout whose names in the directory cover the residues too: the first, as a rule)
        entries, at, seen_b, seen_h = [], 0, set(), {a % 16 for a in OFFSETS}
        for k, ((size, _, nlen, elen, bit3), (data, body)) in enumerate(zip(plan, made)):
            blen = len(data if body is None else body) + (16 if bit3 else 0)
            if nlen is None:  # a free name: the length of 2 to 17 bytes that brings the most new residues, of this body and the next header
                gain = lambda n: len({(at + 30 + n + elen + a) % 16 for a in OFFSETS} - seen_b) + len({(at + 30 + n + elen + blen + a) % 16 for a in OFFSETS} - seen_h)
                nlen = max(range(2, 18), key=lambda n: (gain(n), -((n + turn) % 16)))
            seen_b |= {(at + 30 + nlen + elen + a) % 16 for a in OFFSETS}
            seen_h |= {(at + 30 + nlen + elen + blen + a) % 16 for a in OFFSETS}
            name = (b"%02d/" % k + b"n" * 1000)[:nlen]
            entries.append(entry(name, data, method=0 if body is None else 8, body=body, extra=bytes(range(elen)), descriptor=bit3))
            at += 30 + nlen + elen + blen
        blob = build(entries)
        if all(len(r) == 16 for r in residues(blob)):
            break
    assert all(len(r) == 16 for r in residues(blob)), [sorted(r) for r in residues(blob)]
    return blob, [e["data"] for e in entries], [p[1] is lib and lib_body is not None for p in plan]


OFFSETS = (0, 1, 7)  # where the GPU tests put the file inside a 16-byte aligned tensor


def residues(blob):
    """(headers, names in the directory, bodies): the residues mod 16 at which an archive's parts lie in memory, over OFFSETS."""
    st, ent, _ = index_rule(blob)
    assert st == 0
    body = lambda e: e["hdr_off"] + 30 + e["name_len"] + le16(blob, e["hdr_off"] + 28)
    return tuple({(f(e) + a) % 16 for e in ent for a in OFFSETS} for f in (lambda e: e["hdr_off"], lambda e: e["name_pos"], body))


def failures():
    """The failure archive -> (bytes, [(what, expected, plain bytes)]): expected is a status, 0 for the good entries that stand
    between the damaged ones, or a tuple of statuses."""
    d = [text(3000 + 100 * k, 200 + k) for k in range(32)]
    body = raw_body(d[4])
    plan = [
        ("good, level 6", 0, entry(b"g0", d[0])),
        ("central CRC wrong", ZES_E_CHECKSUM, entry(b"crc", d[1], crc=zlib.crc32(d[1]) ^ 1)),
        ("good, stored", 0, entry(b"g1", d[2], method=0)),
        ("usize + 1", ZES_E_CHECKSUM, entry(b"u+", d[3], usize=len(d[3]) + 1)),
        ("usize - 1", ZES_E_CHECKSUM, entry(b"u-", d[3], usize=len(d[3]) - 1)),
        ("csize - 1", INFLATE_STATUSES + (ZES_E_CHECKSUM,), entry(b"c-", d[4], central=dict(csize=len(body) - 1))),
        ("csize + 1 with a spare byte", ZES_E_CHECKSUM, entry(b"c+", d[4], spare=b"\0", central=dict(csize=len(body) + 1))),
        ("good, level 1", 0, entry(b"g2", d[5], level=1)),
        ("local signature damaged", ZES_E_ZIP, entry(b"sig", d[6], local=dict(sig=0x04034B51))),
        ("local name differing in its first byte", ZES_E_ZIP, entry(b"name-first", d[7], local=dict(name=b"Name-first"))),
        ("local name differing in its last byte, length 257", ZES_E_ZIP, entry(b"n" * 257, d[8], local=dict(name=b"n" * 256 + b"m"))),
        ("good, a name of 257 bytes", 0, entry(b"o" * 257, d[9])),
        ("local method differing", ZES_E_ZIP, entry(b"meth", d[10], method=0, local=dict(method=8))),
        ("local name length differing", ZES_E_ZIP, entry(b"nlen", d[11], local=dict(nlen=5))),
        ("local flag bit 0 differing", ZES_E_ZIP, entry(b"enc", d[12], local=dict(flags=1))),
        ("stored with csize != usize", ZES_E_ZIP, entry(b"st", d[13], method=0, usize=len(d[13]) + 1)),
        ("method 12", ZES_E_UNSUPPORTED, entry(b"bz", d[14], method=12, body=b"BZh9" + d[14][:50])),
        ("flag bit 0", ZES_E_UNSUPPORTED, entry(b"pw", d[15], flags=1)),
        ("flag bit 6", ZES_E_UNSUPPORTED, entry(b"strong", d[15], flags=0x40)),
        ("a body starting a BTYPE 3 block", -2, entry(b"bt3", d[16], body=b"\x07" + bytes(11))),
        ("good, stored, empty", 0, entry(b"g3", b"", method=0)),
        ("data reaching past c: a csize no file has", ZES_E_ZIP, entry(b"far", d[17], central=dict(csize=0x7FFFFFFF))),
        ("good, level 9, bit 3", 0, entry(b"g4", d[18], level=9, descriptor=True)),
        # (its csize is set below: what fits without the local extra field, and not with it)
        ("data reaching past c by its extra field", ZES_E_ZIP, entry(b"edge", d[19], extra=bytes(20))),
        ("good, the last entry", 0, entry(b"g5", d[20])),
    ]
    entries = [p[2] for p in plan]
    first = build(entries)
    st, ent, _ = index_rule(first)
    assert st == 0
    k = [p[0] for p in plan].index("data reaching past c by its extra field")
    entries[k]["central"]["csize"] = len(first) - ent[k]["hdr_off"] - 30 - len(entries[k]["name"])
    blob = build(entries)
    assert len(blob) == len(first)
    st, ent, _ = index_rule(blob)
    assert st == 0 and len(ent) == len(plan)
    for (what, want, e), rec in zip(plan, ent):  # the table against the restated rule
        got = entry_rule(blob, rec)
        if got[0] == INFLATE:
            assert what in ("csize - 1", "a body starting a BTYPE 3 block"), what
        else:
            assert got[0] == want or (isinstance(want, tuple) and got[0] in want), (what, got[0], want)
            assert got[0] != 0 or got[1] == e["data"], what
    return blob, [(what, want, e["data"]) for what, want, e in plan]
