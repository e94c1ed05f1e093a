"""Test-only DEFLATE (RFC 1951) block writer: streams no encoder in this suite makes on its own.

Stored, fixed and dynamic blocks from explicit specs — any LEN / NLEN, any of the 288 literal/length and 32 distance
symbols, code lengths given by the caller — so the tests can build what zlib never emits (distances 32507..32768,
15-bit codes, length 258 as 284 + 31, empty blocks by the thousand) and the reference's quirks (distance codes 30/31,
length codes 286/287, runs past HLIT + HDIST, over-subscribed and incomplete codes) inside large streams.

Everything is a bit string: a 1-D uint8 numpy array of 0/1 values, LSB-first, so pieces join at any bit offset
(`oracle.deflate_range` output included) and pack once at the end.  Token streams are encoded with numpy — one
(value, width) pair per token, expanded in one pass — so streams of several MiB build in about a second.

Plain Python and numpy; imports `_oracle` only for the reference-style header (its Huffman length builder).
"""
import struct
import zlib

import numpy as np

LEN_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258],
                    dtype=np.int64)
LEN_XBITS = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0], dtype=np.int64)
DIST_BASE = np.array([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                      6145, 8193, 12289, 16385, 24577], dtype=np.int64)
DIST_XBITS = np.array([0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13], dtype=np.int64)
CODELEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LLENS = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, dtype=np.int64)
FIXED_DLENS = np.full(32, 5, dtype=np.int64)


# ---------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------
def _rev(codes, widths):
    """Bit-reverse each code within its width (MSB-first Huffman code -> LSB-first field)."""
    codes = np.asarray(codes, dtype=np.uint64)
    widths = np.asarray(widths, dtype=np.int64)
    out = np.zeros(codes.shape, dtype=np.uint64)
    for i in range(int(widths.max()) if widths.size else 0):
        sel = widths > i
        bit = (codes >> np.uint64(i)) & np.uint64(1)
        out[sel] |= bit[sel] << (widths[sel] - 1 - i).astype(np.uint64)
    return out


def fields_to_bits(values, widths):
    """LSB-first fields (value, width) -> one bit string; widths up to 64, zero widths allowed."""
    values = np.asarray(values, dtype=np.uint64).ravel()
    widths = np.asarray(widths, dtype=np.int64).ravel()
    total = int(widths.sum())
    if total == 0:
        return np.zeros(0, dtype=np.uint8)
    # every field lands in the 64-bit word its first bit falls into (the part that does not fit: in the next one); the
    # fields are in order, so the words are sums over runs of fields, and fields never share a bit: sum = or
    values = values & (~np.uint64(0) >> (64 - np.minimum(widths, 64)).astype(np.uint64)) * (widths > 0)
    off = np.cumsum(widths) - widths
    wi, sh = off >> 6, (off & 63).astype(np.uint64)
    first = np.flatnonzero(np.concatenate([[True], wi[1:] != wi[:-1]]))
    words = np.zeros((total + 63) // 64 + 1, dtype=np.uint64)
    words[wi[first]] = np.add.reduceat(values << sh, first)
    words[wi[first] + 1] |= np.add.reduceat((values >> np.uint64(1)) >> (np.uint64(63) - sh), first)
    return np.unpackbits(words.astype("<u8").view(np.uint8), bitorder="little")[:total]


class BitWriter:
    """A growing bit string; `bytes()` packs it, zero-padded to a whole byte."""

    def __init__(self):
        self.parts = []
        self.nbits = 0

    def bits(self, arr):
        arr = np.asarray(arr, dtype=np.uint8)
        self.parts.append(arr)
        self.nbits += arr.size
        return self

    def field(self, value, n):
        """n bits of value, LSB first (header fields, extra bits)."""
        return self.bits(fields_to_bits([value], [n]))

    def code(self, code, n):
        """A Huffman code of n bits, MSB first."""
        return self.field(int(_rev([code], [n])[0]) if n else 0, n)

    def raw(self, data, nbits=None):
        """Bytes as bits (all of them, or the first nbits: what `oracle.deflate_range` returns)."""
        b = np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8), bitorder="little")
        return self.bits(b if nbits is None else b[:nbits])

    def align(self):
        """Zero bits up to the next byte boundary."""
        return self.field(0, -self.nbits % 8)

    def array(self):
        return np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=np.uint8)

    def bytes(self):
        a = self.array()
        return np.packbits(np.concatenate([a, np.zeros(-a.size % 8, dtype=np.uint8)]), bitorder="little").tobytes()


# ---------------------------------------------------------------------------------------------
# tokens: symbol + extra bits, per token, as parallel arrays
# ---------------------------------------------------------------------------------------------
class Tokens:
    """sym: literal/length symbol 0..287; lext/lxn: length extra bits and their count; dsym: distance symbol 0..31
    (-1: a literal, or a token without one); dext/dxn: distance extra bits.  `out` = bytes the RFC says it writes."""

    def __init__(self, sym, lext, lxn, dsym, dext, dxn):
        self.sym = np.asarray(sym, dtype=np.int64)
        self.lext = np.asarray(lext, dtype=np.int64)
        self.lxn = np.asarray(lxn, dtype=np.int64)
        self.dsym = np.asarray(dsym, dtype=np.int64)
        self.dext = np.asarray(dext, dtype=np.int64)
        self.dxn = np.asarray(dxn, dtype=np.int64)

    def __len__(self):
        return self.sym.size

    def __add__(self, other):
        return cat([self, other])

    def out_len(self):
        """Output bytes under RFC 1951 (symbols 286/287 and distance codes 30/31 are not RFC: counted as 0 / as copied)."""
        lc = self.sym - 257
        m = (lc >= 0) & (lc < 29)
        return int((self.sym < 256).sum() + (LEN_BASE[lc[m]] + self.lext[m]).sum())


def cat(toks):
    """One token list from several."""
    return Tokens(*[np.concatenate([getattr(t, f) for t in toks]) for f in ("sym", "lext", "lxn", "dsym", "dext", "dxn")])


def empty_tokens():
    z = np.zeros(0, dtype=np.int64)
    return Tokens(z, z, z, z, z, z)


def literals(data):
    s = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.int64) if not isinstance(data, np.ndarray) else data.astype(np.int64)
    z = np.zeros(s.size, dtype=np.int64)
    return Tokens(s, z, z, z - 1, z, z)


def len_code(length):
    """Length -> code 0..28 (257 + code); 258 is code 28 (285)."""
    length = np.asarray(length, dtype=np.int64)
    return np.where(length == 258, 28, np.searchsorted(LEN_BASE[:28], length, side="right") - 1)


def dist_code(dist):
    return np.searchsorted(DIST_BASE, np.asarray(dist, dtype=np.int64), side="right") - 1


def matches(lengths, dists, lcode=None):
    """(length, distance) pairs; lcode forces the length code (0..28, e.g. 27 for 258 as 284 + 31)."""
    lengths = np.atleast_1d(np.asarray(lengths, dtype=np.int64))
    dists = np.broadcast_to(np.atleast_1d(np.asarray(dists, dtype=np.int64)), lengths.shape)
    assert (lengths >= 3).all() and (lengths <= 258).all() and (dists >= 1).all() and (dists <= 32768).all()
    lc = len_code(lengths) if lcode is None else np.broadcast_to(np.atleast_1d(np.asarray(lcode, dtype=np.int64)), lengths.shape)
    lext = lengths - LEN_BASE[lc]
    assert (lext >= 0).all() and (lext < (1 << LEN_XBITS[lc])).all(), "length does not fit the forced code"
    dc = dist_code(dists)
    return Tokens(257 + lc, lext, LEN_XBITS[lc], dc, dists - DIST_BASE[dc], DIST_XBITS[dc])


def raw_token(sym, lext=0, lxn=None, dsym=-1, dext=0, dxn=None):
    """One token by its symbols, for what RFC 1951 does not define (length codes 286/287, distance codes 30/31)."""
    if lxn is None:
        lxn = int(LEN_XBITS[sym - 257]) if 257 <= sym < 286 else 0
    if dxn is None:
        dxn = int(DIST_XBITS[dsym]) if 0 <= dsym < 30 else 0
    return Tokens([sym], [lext], [lxn], [dsym], [dext], [dxn])


def from_oracle(tok):
    """Tokens of `oracle.lz77_block` (bit 31: match, bits 16-23: length - 3, bits 0-14: distance - 1; else a literal)."""
    tok = np.asarray(tok, dtype=np.uint32)
    m = (tok & 0x80000000) != 0
    out_sym = tok.astype(np.int64)
    lengths = ((tok >> 16) & 0xFF).astype(np.int64) + 3
    dists = (tok & 0x7FFF).astype(np.int64) + 1
    lc = len_code(np.where(m, lengths, 3))
    dc = dist_code(np.where(m, dists, 1))
    return Tokens(np.where(m, 257 + lc, out_sym), np.where(m, lengths - LEN_BASE[lc], 0), np.where(m, LEN_XBITS[lc], 0),
                  np.where(m, dc, -1), np.where(m, dists - DIST_BASE[dc], 0), np.where(m, DIST_XBITS[dc], 0))


def expand(tok, history=b""):
    """The bytes RFC 1951 decodes from the tokens behind `history` (a model for the CPU tests; no quirk symbols)."""
    out = bytearray(history)
    i, n = 0, len(tok)
    sym, lext, dsym, dext = tok.sym, tok.lext, tok.dsym, tok.dext
    while i < n:
        j = i
        while j < n and sym[j] < 256:
            j += 1
        out += bytes(sym[i:j].astype(np.uint8))
        if j == n:
            break
        s = int(sym[j])
        assert 257 <= s <= 285 and 0 <= dsym[j] < 30
        length = int(LEN_BASE[s - 257] + lext[j])
        d = int(DIST_BASE[dsym[j]] + dext[j])
        assert d <= len(out)
        src = out[len(out) - d:len(out) - d + length]
        out += (src * (length // d + 1))[:length] if d < length else src
        i = j + 1
    return bytes(out[len(history):])


# ---------------------------------------------------------------------------------------------
# codes
# ---------------------------------------------------------------------------------------------
def canonical(lens):
    """Canonical codes of RFC 1951 §3.2.2 from code lengths (0 = unused).  Over-subscribed lengths still get codes,
    cut to their width, as the reference's table builder assigns them."""
    lens = np.asarray(lens, dtype=np.int64)
    codes = np.zeros(lens.size, dtype=np.int64)
    code = 0
    for length in range(1, 16):
        for s in np.nonzero(lens == length)[0]:
            codes[s] = code & ((1 << length) - 1)
            code += 1
        code <<= 1
    return codes


def fib_lengths(nsym, maxlen=15):
    """Code lengths with a Fibonacci shape: complete, reaching maxlen bits (the deepest two codes)."""
    lens = np.zeros(nsym, dtype=np.int64)
    assert nsym >= maxlen + 1
    for i in range(maxlen):
        lens[i] = i + 1
    lens[maxlen] = maxlen
    return lens


def kraft(lens):
    lens = np.asarray(lens, dtype=np.int64)
    return sum(2.0 ** -int(x) for x in lens if x)


def encode_tokens(tok, llens, dlens, fixed_dist=False):
    """Bits of the tokens under the code lengths llens (288) / dlens (32).  A fixed block's distance is 5 bits."""
    llens = np.asarray(llens, dtype=np.int64)
    dlens = np.asarray(dlens, dtype=np.int64)
    if len(tok) == 0:
        return np.zeros(0, dtype=np.uint8)
    lcodes, dcodes = canonical(llens), canonical(dlens)
    assert (llens[tok.sym] > 0).all(), "a symbol without a code"
    # (codes are reversed per symbol, not per token)
    lw = llens[tok.sym]
    lv = _rev(lcodes, llens)[tok.sym]
    hasd = tok.dsym >= 0
    ds = np.where(hasd, tok.dsym, 0)
    if fixed_dist:
        dw = np.where(hasd, 5, 0)
        dv = _rev(ds, dw)
    else:
        assert (dlens[ds[hasd]] > 0).all(), "a distance without a code"
        dw = np.where(hasd, dlens[ds], 0)
        dv = np.where(hasd, _rev(dcodes, dlens)[ds], np.uint64(0))
    # one field of at most 15 + 5 + 15 + 13 bits per token
    v = lv.copy()
    w = lw.copy()
    for val, wid in ((tok.lext, tok.lxn), (dv, dw), (tok.dext, tok.dxn)):
        v |= np.asarray(val, dtype=np.uint64) << w.astype(np.uint64)
        w += wid
    return fields_to_bits(v, w)


# ---------------------------------------------------------------------------------------------
# blocks
# ---------------------------------------------------------------------------------------------
def stored(w, data, final=False, nlen=None, length=None):
    """A stored block: header, zero bits to the byte boundary, LEN, NLEN (overridable), the bytes."""
    data = bytes(data)
    length = len(data) if length is None else length
    assert len(data) <= 65535
    w.field(1 if final else 0, 1).field(0, 2).align()
    w.field(length, 16).field((~length & 0xFFFF) if nlen is None else nlen, 16)
    return w.raw(data)


def fixed(w, tok, final=False, eob=True):
    w.field(1 if final else 0, 1).field(1, 2)
    w.bits(encode_tokens(tok, FIXED_LLENS, FIXED_DLENS, fixed_dist=True))
    if eob:
        w.code(0, 7)  # 256: seven zero bits
    return w


def rle_lengths(lens):
    """An ordinary run-length coding of code lengths -> [(symbol, extra)]: 17/18 for zeros, 16 after a length."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v = int(lens[i])
        j = i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, 0)] * run
        i = j
    return out


def cl_lengths(syms):
    """Code-length code lengths (19, by symbol) for the symbols used: the reference's builder at 7 bits, with a
    second symbol added when only one is used (a one-symbol code-length code is incomplete, which zlib rejects)."""
    import _oracle

    hist = np.zeros(19, dtype=np.uint32)
    for s in syms:
        hist[s] += 1
    if (hist > 0).sum() < 2:
        hist[0 if hist[0] == 0 else 18] += 1
    return _oracle.huff_lengths(hist, 7).astype(np.int64)


def dynamic_header(w, hlit, hdist, clens, cl_syms, hclen=None):
    """HLIT / HDIST / HCLEN (as counts: 257.., 1.., 4..), the code-length code, then the (symbol, extra) list."""
    clens = np.asarray(clens, dtype=np.int64)
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if clens[CODELEN_ORDER[i]]])
    w.field(hlit - 257, 5).field(hdist - 1, 5).field(hclen - 4, 4)
    for i in range(hclen):
        w.field(int(clens[CODELEN_ORDER[i]]), 3)
    ccodes = canonical(clens)
    xb = {16: 2, 17: 3, 18: 7}
    syms = np.array([s for s, _ in cl_syms], dtype=np.int64)
    ext = np.array([e for _, e in cl_syms], dtype=np.int64)
    if syms.size:
        cw = clens[syms]
        assert (cw > 0).all(), "a code-length symbol without a code"
        xw = np.array([xb.get(int(s), 0) for s in syms], dtype=np.int64)
        w.bits(fields_to_bits(_rev(ccodes[syms], cw) | (ext.astype(np.uint64) << cw.astype(np.uint64)), cw + xw))
    return w


def dynamic(w, tok, llens, dlens, final=False, cl_syms=None, hlit=None, hdist=None, hclen=None, clens=None, eob=True):
    """A dynamic block.  llens / dlens: the code lengths the decoder ends up with (they code the tokens).  The header
    is an ordinary run-length coding of them unless cl_syms gives the (symbol, extra) list to write as it is; hlit /
    hdist / hclen / clens override what is derived (for the quirks)."""
    llens = np.zeros(288, dtype=np.int64) + np.pad(np.asarray(llens, dtype=np.int64), (0, 288 - len(llens)))
    dlens = np.zeros(32, dtype=np.int64) + np.pad(np.asarray(dlens, dtype=np.int64), (0, 32 - len(dlens)))
    if hlit is None:
        hlit = max(257, int(np.nonzero(llens)[0].max()) + 1 if llens.any() else 257)
    if hdist is None:
        hdist = max(1, int(np.nonzero(dlens)[0].max()) + 1 if dlens.any() else 1)
    if cl_syms is None:
        cl_syms = rle_lengths(np.concatenate([llens[:hlit], dlens[:hdist]]))
    if clens is None:
        clens = cl_lengths([s for s, _ in cl_syms])
    w.field(1 if final else 0, 1).field(2, 2)
    dynamic_header(w, hlit, hdist, clens, cl_syms, hclen)
    w.bits(encode_tokens(tok, llens, dlens))
    if eob:
        w.code(int(canonical(llens)[256]), int(llens[256]))
    return w


def ref_header(tok):
    """What the reference puts into a dynamic block's header for these tokens (src/deflate.ts:56-148): histograms with
    EOB counted once, lengths by its Huffman builder at 15 bits, HLIT / HDIST up to the largest symbol used, its
    run-length rule, the code-length code at 7 bits -> (llens, dlens, hlit, hdist, cl_syms, clens)."""
    import _oracle

    lhist = np.bincount(tok.sym, minlength=286)[:286].astype(np.uint32)
    lhist[256] += 1
    hasd = tok.dsym >= 0
    dhist = np.bincount(tok.dsym[hasd], minlength=30)[:30].astype(np.uint32)
    lmax = max(256, int(tok.sym.max()) if len(tok) else 0)
    dmax = int(tok.dsym[hasd].max()) if hasd.any() else 0
    llens = _oracle.huff_lengths(lhist, 15).astype(np.int64)
    dlens = _oracle.huff_lengths(dhist, 15).astype(np.int64)
    codelens = list(llens[:lmax + 1]) + list(dlens[:dmax + 1])
    cl_syms, i, n = [], 0, len(codelens)
    while i < n:
        cl, rep = codelens[i], 1
        while i + 1 < n and cl == codelens[i + 1]:
            rep += 1
            i += 1
            if rep >= (138 if cl == 0 else 6):
                break
        if rep >= 4:
            if cl == 0:
                cl_syms.append((18 if rep >= 11 else 17, rep - (11 if rep >= 11 else 3)))
            else:
                cl_syms += [(int(cl), 0), (16, rep - 1 - 3)]
        else:
            cl_syms += [(int(cl), 0)] * rep
        i += 1
    chist = np.bincount([s for s, _ in cl_syms], minlength=19).astype(np.uint32)
    clens = _oracle.huff_lengths(chist, 7).astype(np.int64)
    return llens, dlens, lmax + 1, dmax + 1, cl_syms, clens


def ref_dynamic(w, tok, final=False):
    """A dynamic block the way the reference writes one (src/deflate.ts:56-227): ref_header's header (HCLEN up to the
    code-length code's last non-zero length), then the tokens."""
    llens, dlens, hlit, hdist, cl_syms, clens = ref_header(tok)
    return dynamic(w, tok, llens, dlens, final, cl_syms=cl_syms, hlit=hlit, hdist=hdist, clens=clens)


def ref_block(w, data, start, length, final=False):
    """The reference's block over data[start:start + length] (its own LZ77), reference-style header."""
    import _oracle

    return ref_dynamic(w, from_oracle(_oracle.lz77_block(data, start, length)), final)


# ---------------------------------------------------------------------------------------------
# splicing with CPython's zlib
# ---------------------------------------------------------------------------------------------
def zlib_piece(w, data, level=6, flush=zlib.Z_SYNC_FLUSH, zdict=None, final=False, **kw):
    """A raw zlib piece at the next byte boundary: the writer is aligned first by an empty stored block (what a sync
    flush writes), then a fresh raw compressobj's output ending in `flush` (Z_SYNC_FLUSH / Z_FULL_FLUSH), or its
    final block when final.  Matches in it reach back into zdict only (e.g. the plaintext so far)."""
    if w.nbits % 8:
        sync(w)
    args = dict(level=level, wbits=-15, **kw)
    if zdict:
        args["zdict"] = bytes(zdict[-32768:])
    co = zlib.compressobj(**args)
    body = co.compress(bytes(data)) + (co.flush() if final else co.flush(flush))
    return w.raw(body)


def sync(w):
    """An empty non-final stored block: the writer ends on a byte boundary."""
    return stored(w, b"")


def final_empty(w):
    """An empty final fixed block (ten bits) to end a stream."""
    return fixed(w, empty_tokens(), final=True)


def zlib_wrap(raw):
    """78 9c, the raw stream, Adler-32 of what zlib decodes from it (an undecodable body gets that of nothing)."""
    try:
        plain = zlib.decompress(raw, -15)
    except zlib.error:
        plain = b""
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(plain))


def gzip_wrap(raw, plain):
    """One gzip member around a raw stream: fixed header (no flags), CRC-32 and ISIZE of plain."""
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff" + raw + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xFFFFFFFF)
