"""Hand-built DEFLATE streams for the CPU tests of the writer and the GPU tests of every inflate tier.

Each valid case carries the plaintext it is built to decode to (tracked token by token while writing), each quirk
case the reference's result claimed for it (bytes, or its error code).  Both test files build from here.
"""
import functools
import zlib

import numpy as np

import _deflate_writer as W

FAR = (32506, 32507, 32767, 32768)  # zlib matches up to 32506 back; T2's window ends at 32768


@functools.lru_cache(maxsize=64)
def text(n, seed=1):
    """Readable bytes with repeats (words from a fixed list), deterministic."""
    rng = np.random.default_rng(seed)
    words = np.array([w.encode() for w in ("the ", "window ", "block ", "of ", "inflate ", "tier ", "match ", "distance ", "segment ",
                                           "piece ", "and ", "a ", "bits ", "zlib ", "code ", "length ", "\n", "huffman ", "stored ")])
    out = b"".join(words[rng.integers(0, words.size, n // 3 + 16)])
    return out[:n]


def lens_for(tok):
    """Code lengths (288 / 32) for the symbols the tokens use, plus EOB: the reference's builder at 15 bits."""
    import _oracle

    lh = np.bincount(tok.sym, minlength=286)[:286].astype(np.uint32)
    lh[256] += 1
    d = tok.dsym[tok.dsym >= 0]
    dh = np.bincount(d, minlength=30)[:30].astype(np.uint32)
    ll = np.zeros(288, dtype=np.int64)
    ll[:286] = _oracle.huff_lengths(lh, 15)
    dl = np.zeros(32, dtype=np.int64)
    if d.size:
        dl[:30] = _oracle.huff_lengths(dh, 15)
    return ll, dl


class Stream:
    """A bit writer plus the plaintext its blocks decode to."""

    def __init__(self):
        self.w = W.BitWriter()
        self.plain = bytearray()

    def zlib(self, data, level=6, flush=zlib.Z_SYNC_FLUSH, final=False, zdict=False):
        W.zlib_piece(self.w, data, level, flush, zdict=bytes(self.plain) if zdict and self.plain else None, final=final)
        self.plain += data
        return self

    def sync(self):
        W.sync(self.w)
        return self

    def _grow(self, tok):
        self.plain += W.expand(tok, bytes(self.plain[-32768:]))

    def fixed(self, tok, final=False):
        W.fixed(self.w, tok, final)
        self._grow(tok)
        return self

    def dynamic(self, tok, final=False, llens=None, dlens=None, **kw):
        if llens is None:
            llens, dlens = lens_for(tok)
        W.dynamic(self.w, tok, llens, dlens, final, **kw)
        self._grow(tok)
        return self

    def stored(self, data, final=False):
        W.stored(self.w, data, final)
        self.plain += data
        return self

    def raw(self):
        return self.w.bytes()


# ---------------------------------------------------------------------------------------------
# valid shapes (RFC 1951): each a Stream, decoded by zlib to .plain
# ---------------------------------------------------------------------------------------------
def far_tokens(rng, out_len, src):
    """~out_len bytes of tokens: a match at distance 32768 first, then runs of literals from src and matches at the
    far distances (and some near ones)."""
    first = int(rng.integers(3, 259))
    n, pos = first, int(rng.integers(0, len(src) - 64))
    k = 0
    lits, lens, dists = [], [first], [32768]
    while n < out_len:
        k = int(rng.integers(8, 40))
        lits.append(src[pos:pos + k])
        pos = (pos + k) % (len(src) - 64)
        dists.append(int(FAR[rng.integers(0, 4)]) if rng.random() < 0.8 else int(rng.integers(1, 32768)))
        lens.append(int(rng.integers(3, 40)) if rng.random() < 0.9 else 258)
        n += k + lens[-1]
    # match 0, literal run 1, match 1, ..., literal run k, match k
    m, lit = W.matches(lens, dists), W.literals(b"".join(lits))
    runs = np.array([0] + [len(x) for x in lits])
    at = np.arange(len(lens)) + np.cumsum(runs)
    is_m = np.zeros(len(m) + len(lit), dtype=bool)
    is_m[at] = True
    f = ("sym", "lext", "lxn", "dsym", "dext", "dxn")
    cols = []
    for name in f:
        c = np.empty(is_m.size, dtype=np.int64)
        c[is_m], c[~is_m] = getattr(m, name), getattr(lit, name)
        cols.append(c)
    return W.Tokens(*cols)


def far_distance_stream(mib=8, seed=5):
    """>= mib MiB of zlib text; behind every 64 KiB piece, eight hand-built blocks (dynamic, fixed, stored) whose
    first token is a match at distance 32768 and whose other matches are mostly at 32506 / 32507 / 32767 / 32768:
    whichever block a segment or a piece starts at, its first bytes come from the oldest bytes of the window."""
    rng = np.random.default_rng(seed)
    src = text(4 << 20, seed)
    s = Stream()
    s.zlib(src[:40000], final=False)
    pos = 40000
    while pos < (mib << 20):
        for kind in ("dynamic", "dynamic", "fixed", "dynamic", "stored", "dynamic", "fixed", "dynamic"):
            if kind == "stored":
                s.stored(src[(pos * 7) % (3 << 20):(pos * 7) % (3 << 20) + 2000])
            else:
                getattr(s, kind)(far_tokens(rng, 8000, src))
        chunk = src[pos % (3 << 20):pos % (3 << 20) + 65536]
        s.zlib(chunk, flush=zlib.Z_FULL_FLUSH if rng.random() < 0.3 else zlib.Z_SYNC_FLUSH)
        pos += 65536
    s.dynamic(far_tokens(rng, 3000, src), final=True)
    return s


def pad_text(s, n, seed, final=False):
    return s.zlib(text(n, seed), final=final)


def shape_cases():
    """-> [(name, Stream)] of rare but legal shapes, each spliced between zlib text (>= 32 KiB compressed)."""
    cases = []
    src = text(1 << 20, 11)

    # 15-bit literal/length and distance codes: 8-bit literals, and a Fibonacci-shaped tail of 8..15, 15 bits in the
    # two 8-bit slots left free (two letters, EOB and six length codes); distance codes of 1..15, 15 bits
    ll = np.zeros(288, dtype=np.int64)
    ll[:256] = 8
    tail = [257, 258, 259, b"e"[0], 260, 261, b"t"[0], 262, 256]
    ll[tail] = [8, 9, 10, 11, 12, 13, 14, 15, 15]
    dl = np.zeros(32, dtype=np.int64)
    dl[:16] = W.fib_lengths(16)
    assert W.kraft(ll) == 1.0 and W.kraft(dl) == 1.0 and ll.max() == 15 and dl.max() == 15
    rng = np.random.default_rng(3)
    parts = []
    for i in range(3000):
        parts.append(W.literals(src[i * 20:i * 20 + 12]))
        length = 3 + i % 6  # codes 257..262: no extra bits
        dc = i % 16
        parts.append(W.matches(length, int(W.DIST_BASE[dc] + rng.integers(0, 1 << int(W.DIST_XBITS[dc])))))
    s = pad_text(Stream(), 200000, 12)
    s.dynamic(W.cat(parts), llens=ll, dlens=dl)
    cases.append(("15-bit codes", pad_text(s, 200000, 13, final=True)))

    # HLIT = 286, HDIST = 30, HCLEN = 19; lengths 283..285 and distance codes 0, 1 all of 4 bits: one run of 16 covers
    # the end of the literal/length lengths and the start of the distance lengths
    ll = np.zeros(288, dtype=np.int64)
    ll[:192] = 8
    ll[[256, 283, 284, 285]] = 4
    dl = np.zeros(32, dtype=np.int64)
    dl[:30] = 5
    dl[:2] = 4
    assert W.kraft(ll) == 1.0 and W.kraft(dl) == 1.0
    parts = [W.literals(src[:3000])]
    for i in range(200):
        dc = i % 30
        d = min(int(W.DIST_BASE[dc]), 100000)
        parts += [W.matches(195 + (i * 7) % 64, d), W.literals(src[3000 + i * 9:3000 + i * 9 + 9])]
    tok = W.cat(parts)
    cl = W.rle_lengths(np.concatenate([ll[:286], dl[:30]]))
    assert any(sym == 16 for sym, _ in cl)
    s = pad_text(Stream(), 150000, 14)
    s.dynamic(tok, llens=ll, dlens=dl, hlit=286, hdist=30, hclen=19)
    cases.append(("hlit 286 hclen 19, 16 across the tables", pad_text(s, 150000, 15, final=True)))

    # a single distance code; HDIST = 1 with length 0 in a block without matches
    s = pad_text(Stream(), 150000, 16)
    tok = W.literals(src[:2000]) + W.matches([10, 20, 258], 7) + W.literals(src[2000:2100])
    ll, dl = lens_for(tok)
    s.dynamic(tok, llens=ll, dlens=dl)
    tok = W.literals(src[5000:9000])
    ll, dl = lens_for(tok)
    s.dynamic(tok, llens=ll, dlens=np.zeros(32, dtype=np.int64))
    cases.append(("one distance code, hdist 1 of length 0", pad_text(s, 150000, 17, final=True)))

    # 258 as 285 and as 284 + 31; overlapping copies at distances 1, 2, 3, 257
    s = pad_text(Stream(), 150000, 18)
    for kind in ("fixed", "dynamic"):
        tok = W.literals(b"a") + W.matches(258, 1) + W.matches(258, 1, lcode=27) + W.literals(src[:300])
        for d in (1, 2, 3, 257):
            tok = tok + W.matches([258, 3, 17, 258], d) + W.matches(258, d, lcode=27) + W.literals(src[d:d + 5])
        getattr(s, kind)(tok)
    cases.append(("258 as 285 and 284+31, overlapping copies", pad_text(s, 150000, 19, final=True)))

    # stored blocks of 0 and 65535 bytes at all 8 header bit phases (a fixed block of k literals shifts the phase)
    s = pad_text(Stream(), 100000, 20)
    big = bytes(src[:65535])
    for phase in range(8):
        s.fixed(W.literals(b"\xc8" * phase))  # 10 + 9 * phase bits (9-bit literals)
        s.stored(b"")
        s.fixed(W.literals(b"\xc9" * phase))
        s.stored(big)
    cases.append(("stored 0 and 65535 at every phase", pad_text(s, 100000, 21, final=True)))

    # EOB-only dynamic blocks and empty fixed blocks, 5000 tiny blocks in a row
    s = pad_text(Stream(), 100000, 22)
    eob = np.zeros(288, dtype=np.int64)
    eob[256] = 1
    w_eob, w_fix = W.BitWriter(), W.BitWriter()
    W.dynamic(w_eob, W.empty_tokens(), eob, np.zeros(32))
    W.fixed(w_fix, W.empty_tokens())
    for i in range(5000):
        if i % 2:
            s.w.bits(w_eob.array())
        elif i % 4:
            s.w.bits(w_fix.array())
        else:
            s.fixed(W.literals(b"%d" % i))
    cases.append(("5000 tiny blocks", pad_text(s, 100000, 23, final=True)))

    # code 16 right behind 17 / 18 (repeats the zero): legal, though the reference's writer never does it
    tok = W.literals(src[:4000]) + W.matches([30, 40], [100, 3000])
    ll, dl = lens_for(tok)
    cl = W.rle_lengths(np.concatenate([ll[:286], dl[:30]]))
    out = []
    for sym, ex in cl:
        if sym == 18 and ex >= 3:  # 18 of n zeros -> 18 of n - 3, then 16 of three (zeros again)
            out += [(18, ex - 3), (16, 0)]
        elif sym == 17 and ex >= 3:
            out += [(17, ex - 3), (16, 0)]
        else:
            out.append((sym, ex))
    s = pad_text(Stream(), 150000, 24)
    s.dynamic(tok, llens=ll, dlens=dl, cl_syms=out, hlit=286, hdist=30)
    cases.append(("16 behind 17/18", pad_text(s, 150000, 25, final=True)))
    return cases


def lens_any(tok):
    """Complete code lengths over all 288 / 32 symbols the tokens use (quirk symbols included), plus EOB."""
    import _oracle

    lh = np.bincount(tok.sym, minlength=288).astype(np.uint32)
    lh[256] += 1
    d = tok.dsym[tok.dsym >= 0]
    ll = _oracle.huff_lengths(lh, 15).astype(np.int64)
    dl = _oracle.huff_lengths(np.bincount(d, minlength=32).astype(np.uint32), 15).astype(np.int64) if d.size else np.zeros(32, dtype=np.int64)
    return ll, dl


def bfinal_middle():
    """A final block in the middle: the decoders stop there; what follows is trailing data."""
    src = text(600000, 31)
    s = Stream()
    s.zlib(src[:200000])
    s.dynamic(W.literals(src[200000:203000]) + W.matches(200, 32768), final=True)
    plain = bytes(s.plain)
    s.zlib(src[300000:], final=True)
    return s.raw(), plain


def big_run_block(n):
    """One dynamic block of n output bytes: a literal, then runs at distance 1."""
    k, r = divmod(n - 1, 258)
    tok = W.literals(b"Z") + W.matches(np.full(k, 258), 1)
    if r >= 3:
        tok = tok + W.matches(r, 1)
    else:
        tok = tok + W.literals(b"Z" * r)
    w = W.BitWriter()
    ll, dl = lens_for(tok)
    W.dynamic(w, tok, ll, dl, final=True)
    return w.bytes()


# ---------------------------------------------------------------------------------------------
# quirks: outside RFC 1951 (zlib rejects them), defined by the reference
# ---------------------------------------------------------------------------------------------
PRE = text(300, 41)
POST = b" and the end."


def _ref_copy(out, length, dist):
    """The reference's copy: sources before the output (or no distance: dist None) write zeros."""
    for _ in range(length):
        src = len(out) - dist if dist is not None else -1
        out.append(out[src] if src >= 0 else 0)


def quirk_cases():
    """-> [(name, block writer fn(w, final), claimed result for the block alone behind nothing, may_follow_data)].
    The claim is the output bytes, or the reference's error code."""
    cases = []

    def fixed_q(tok_mid):
        return lambda w, final: W.fixed(w, W.literals(PRE) + tok_mid + W.literals(POST), final)

    for dsym in (30, 31):
        cases.append(("fixed dist code %d" % dsym, fixed_q(W.raw_token(264, dsym=dsym)), PRE + b"\x00" * 10 + POST, True))
        tok = W.literals(PRE) + W.raw_token(265, lext=1, dsym=dsym) + W.matches(4, 7) + W.literals(POST)
        ll, dl = lens_any(tok)
        want = bytearray(PRE + b"\x00" * 12)
        _ref_copy(want, 4, 7)
        cases.append(("dynamic dist code %d, hdist %d" % (dsym, dsym + 1),
                      lambda w, final, tok=tok, ll=ll, dl=dl, h=dsym + 1: W.dynamic(w, tok, ll, dl, final, hdist=h),
                      bytes(want) + POST, True))
    for lsym in (286, 287):
        mid = W.raw_token(lsym, dsym=29, dext=12345) + W.raw_token(lsym, dsym=2)
        cases.append(("fixed length code %d" % lsym, fixed_q(mid), PRE + POST, True))
        tok = W.literals(PRE) + W.raw_token(lsym, dsym=29, dext=777) + W.literals(POST)
        ll, dl = lens_any(tok)
        cases.append(("dynamic length code %d, hlit %d" % (lsym, lsym + 1),
                      lambda w, final, tok=tok, ll=ll, dl=dl, h=lsym + 1: W.dynamic(w, tok, ll, dl, final, hlit=h), PRE + POST, True))
    want = bytearray(b"abc")
    _ref_copy(want, 10, 100)
    cases.append(("distance before the output", lambda w, final: W.fixed(w, W.literals(b"abc") + W.matches(10, 100) + W.literals(POST), final),
                  bytes(want) + POST, False))
    # code-length sequences
    tok = W.literals(PRE[10:] + POST) + W.matches(7, 3)
    ll, dl = lens_for(tok)
    assert not ll[:3].any() and ll[262:].sum() == 0 and dl[3:].sum() == 0
    cl = [(16, 0)] + W.rle_lengths(np.concatenate([ll[3:262], dl[:3]]))  # 16 first: three zeros
    cases.append(("16 as the first code-length symbol", lambda w, final, tok=tok, ll=ll, dl=dl, cl=cl: W.dynamic(
        w, tok, ll, dl, final, cl_syms=cl, hlit=262, hdist=3), W.expand(tok), True))
    tok = W.literals(PRE + POST) + W.matches([5, 6, 9], [1, 2, 3])
    ll, dl = lens_for(tok)
    dl2 = np.zeros(32, dtype=np.int64)
    dl2[:5] = 2  # hdist 3: one length of 2, then 16 x4 runs two past HLIT + HDIST: an over-full distance table
    hlit = int(np.nonzero(ll)[0].max()) + 1
    cl = W.rle_lengths(ll[:hlit]) + [(2, 0), (16, 1)]
    cases.append(("run past hlit + hdist", lambda w, final, tok=tok, ll=ll, dl2=dl2, cl=cl, hlit=hlit: W.dynamic(
        w, tok, ll, dl2, final, cl_syms=cl, hlit=hlit, hdist=3), W.expand(tok), True))
    # over-subscribed codes
    ll = np.zeros(288, dtype=np.int64)
    ll[:255] = 8
    ll[255:257] = 9
    cl = [(8, 0)] * 255 + [(9, 0), (9, 0), (0, 0)]
    clens = np.zeros(19, dtype=np.int64)
    clens[[0, 8, 9, 18]] = [1, 2, 2, 2]  # Kraft 5/4; 18 gets no reachable code and is not used
    tok = W.literals(PRE + bytes([255]) + POST)
    cases.append(("over-subscribed code-length code", lambda w, final, tok=tok, ll=ll, cl=cl, clens=clens: W.dynamic(
        w, tok, ll, np.zeros(32), final, cl_syms=cl, hlit=257, hdist=1, clens=clens), PRE + bytes([255]) + POST, True))
    ll = np.zeros(288, dtype=np.int64)
    ll[:255] = 8
    ll[255:258] = 9  # Kraft 1 + 1/512; 257 lands on no reachable code
    cases.append(("over-subscribed literal/length code", lambda w, final, tok=tok, ll=ll: W.dynamic(w, tok, ll, np.zeros(32), final),
                  PRE + bytes([255]) + POST, True))
    tok = W.literals(PRE + POST) + W.matches([5, 6], [1, 2]) + W.literals(b"!")
    ll, _ = lens_for(tok)
    dl = np.zeros(32, dtype=np.int64)
    dl[:3] = 1  # three codes of one bit; code 2 is unreachable and unused
    cases.append(("over-subscribed distance code", lambda w, final, tok=tok, ll=ll, dl=dl: W.dynamic(w, tok, ll, dl, final), W.expand(tok), True))
    # incomplete codes: unused, and hit
    ll = np.zeros(288, dtype=np.int64)
    ll[:254] = 8
    ll[256] = 8  # 255 codes of 8 bits: 11111111 is no code
    tok = W.literals(PRE[:50] + b"\x01\x02")
    cases.append(("incomplete literal/length code, not hit", lambda w, final, tok=tok, ll=ll: W.dynamic(w, tok, ll, np.zeros(32), final),
                  W.expand(tok), True))
    cases.append(("incomplete literal/length code, hit",
                  lambda w, final, tok=tok, ll=ll: W.dynamic(w, tok, ll, np.zeros(32), final, eob=False).code(255, 8).field(0, 16), -3, True))
    tok = W.literals(PRE + POST) + W.matches([5, 6, 7], [1, 2, 3])
    ll, _ = lens_for(tok + W.matches(3, 1))
    dl = np.zeros(32, dtype=np.int64)
    dl[:3] = 2  # 00 01 10; 11 is no code
    cases.append(("incomplete distance code, not hit", lambda w, final, tok=tok, ll=ll, dl=dl: W.dynamic(w, tok, ll, dl, final), W.expand(tok), True))

    def dist_hit(w, final, tok=tok, ll=ll, dl=dl):
        W.dynamic(w, tok, ll, dl, final, eob=False)
        c = W.canonical(ll)
        return w.code(int(c[257]), int(ll[257])).code(3, 2).field(0, 16)

    cases.append(("incomplete distance code, hit", dist_hit, -3, True))
    # empty tables
    cases.append(("empty literal/length table", lambda w, final: W.dynamic(w, W.empty_tokens(), np.zeros(288), np.zeros(32), final, eob=False,
                                                                            cl_syms=[(18, 127), (18, 109)], hlit=257, hdist=1).field(0, 64), -5, True))
    tok = W.literals(PRE)
    ll, _ = lens_for(tok + W.matches(3, 1))

    def empty_dist(w, final, tok=tok, ll=ll):
        W.dynamic(w, tok, ll, np.zeros(32), final, eob=False)
        c = W.canonical(ll)
        return w.code(int(c[257]), int(ll[257])).field(0, 64)

    cases.append(("empty distance table, then a length", empty_dist, -5, True))
    cases.append(("stored LEN/NLEN mismatch", lambda w, final: W.stored(w, PRE, final, nlen=(~len(PRE) & 0xFFFF) ^ 4), -3, True))
    return cases


def quirk_stream(fn, where, seed=0):
    """The quirk block alone (final), first, last or in the middle of a zlib-spliced stream: 2 MiB of text in front
    of it (last, middle), ~200 KB behind it (first, middle: the serial tiers decode what follows a quirk) -> raw."""
    w = W.BitWriter()
    if where == "alone":
        fn(w, True)
        return w.bytes()
    before = text(2 << 20, 50 + seed) if where in ("last", "middle") else b""
    if before:
        W.zlib_piece(w, before)
    fn(w, where == "last")
    if where != "last":
        W.zlib_piece(w, text(200000, 60 + seed), final=True)
    return w.bytes()


# ---------------------------------------------------------------------------------------------
# T1 impostors: reference-style headers, but not a clean chain
# ---------------------------------------------------------------------------------------------
def impostor_cases():
    """-> [(name, raw stream, T1 may take it)]: blocks of oracle.deflate_range and reference-style hand-built blocks."""
    import _oracle

    B = 131072
    src = np.frombuffer(text(6 * B, 71), dtype=np.uint8).copy()
    cases = []

    def join(*parts):
        w = W.BitWriter()
        for p in parts:
            if isinstance(p, tuple):
                w.raw(p[0], p[1])
            else:
                p(w)
        return w.bytes()

    # block 1's first tokens are matches into block 0 (the data repeats there)
    a = src.copy()
    a[B:B + 300] = a[B - 1000:B - 700]
    tok = W.matches([258, 42], 1000) + W.from_oracle(_oracle.lz77_block(a, B + 300, B - 300))
    cases.append(("matches into the previous block", join(_oracle.deflate_range(a, 0, B, False), lambda w: W.ref_dynamic(w, tok),
                                                          _oracle.deflate_range(a, 2 * B, 2 * B + 5, True)), False))
    for n in (B - 1, B + 1):
        cases.append(("non-final block of %d bytes" % n, join(lambda w, n=n: W.ref_block(w, src, 0, n), lambda w, n=n: W.ref_block(w, src[n:], 0, B),
                                                              lambda w, n=n: W.ref_block(w, src[n + B:], 0, 3000, True)), False))
    cases.append(("bfinal on a middle block", join(_oracle.deflate_range(src, 0, 2 * B, True), _oracle.deflate_range(src, 2 * B, 2 * B, True)), None))
    other = np.frombuffer(text(3 * B, 72), dtype=np.uint8).copy()
    cases.append(("blocks of different inputs", join(_oracle.deflate_range(src, 0, 2 * B, False), _oracle.deflate_range(other, 0, 2 * B + 7, True)), True))
    return cases
