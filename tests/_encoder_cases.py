"""Inputs built to reach each data-dependent route of the deflate kernels and each rule of the reference's encoder
(src/lz77.ts, src/deflate.ts, src/huffman.ts), with the tools that say what an input reaches.

    cases(z)            name -> Case(data, start, length, route, rules): the bytes, the block the stage-level checks take,
                        the route that block is built for (decode_route's fields) and the rules the case claims
    decode_route(w, n)  the nine words of zes_stage_lz77_route as named fields
    census(data)        the rules the oracle's tokens and headers show on these bytes (RULES lists them all)
    sort_model / index_model / eager_matches: the integer decisions of k_lz_sort, k_lz_index and k_lz_match restated with
                        numpy, so that a case's route is a checked property of its bytes (tests/test_encoder_cases_cpu.py)

tests/golden/make_encoder_cases.py runs every case through the reference and records lengths, hashes and the census in
tests/golden/encoder_cases.json; no input bytes are kept anywhere: the builders make them again, from the library's
generators and numpy.

Rules and routes without a case, and why:
  * a token count of 1: the shortest block has two bytes (deflate throws on n = 0, 1 and n = 1 mod 131072), and every
    byte of a block without a match is a token;
  * HCLEN 4: the code-length code would hold 16, 17, 18 and 0 alone, but end-of-block always has a code, so a length
    of 1..15 is always written, and those stand behind the first four places of the HCLEN order;
(k_lz_index's three reasons for handing a block back all have inputs: class_handed_back, group_handed_back,
heavy_handed_back.)
"""
import bisect
import collections
import functools

import numpy as np

import _deflate_writer as dw
import _oracle

BLK = 131072
WINDOW = 32768
MLIST_CAP = 4095

Case = collections.namedtuple("Case", "data start length route rules deep")

# every rule the census knows, in the order of the issue's lists
LZ_RULES = ["dist_32768", "dist_32769_unseen", "len_3", "len_257", "len_258", "tie_nearer", "cand16_taken", "cand17_unseen",
            "cand128_taken", "cand129_unseen", "end_exact", "end_plus1_literal", "run_to_input_end", "len_through_next_block",
            "prev_block_only_literal", "key_000000", "key_ffffff"]
HDR_RULES = ["no_match_hdist1", "one_dist_code", "hlit286_dist30", "lit_code_15", "token_15_13", "cl_code_7", "hclen_19",
             "nzrun_3", "nzrun_4", "nzrun_6", "nzrun_7", "nzrun_8", "zrun_3", "zrun_4", "zrun_10", "zrun_11", "zrun_138", "zrun_139",
             "run_crosses_lit_dist", "one_literal_eob",
             "ntok_2", "ntok_3", "ntok_4", "ntok_5", "ntok_4095", "ntok_4096", "ntok_4097", "ntok_8192"]
RULES = LZ_RULES + HDR_RULES


# ---------------------------------------------------------------------------------------------
# the route record
# ---------------------------------------------------------------------------------------------
F_LAZY, F_INDEX, F_REDO, F_COUNT = 0x80000000, 0x40000000, 0x20000000, 0x1FFFFFFF
LAZY_BITS = ["guarded", "probed", "periodic", "abort3", "late_clear", "walk3"]


def decode_route(w, length):
    """Named fields of a route record (include/zes.h, zes_stage_lz77_route) of a block of `length` bytes:
    sort   nokeys | two | one | dense | to_index      what the first k_lz_sort launch did
    index  None | regs | radix | back:<reasons>       k_lz_index: took it (largest class <= 512 words / above), handed back
    kept   positions the match finder got
    match  lazy | list_only | listed | overflow       k_lz_match_lazy, or k_lz_match's three forms
    nml    matches k_lz_match found (None: lazy)
    lazy   the names of the lazy matcher's route bits, in LAZY_BITS order (None: eager)
    parse  mask | list | maps
    ntok   tokens"""
    w = [int(x) for x in w]
    f0, f1, f2, sortw, idxw, ml0, tm0, lz, ntok = w
    r = {}
    if f0 & F_INDEX:
        r["sort"] = "to_index"
        assert f0 & F_LAZY and (f0 & F_COUNT) == length - 2 and sortw == 0
        maxc = idxw & 0x3FFFF
        if f1 & F_REDO:
            why = (["class"] if maxc > 4096 else []) + (["group"] if idxw & 0x40000000 else []) + (["heavy"] if idxw & 0x80000000 else [])
            assert why and not f1 & (F_LAZY | F_INDEX)
            r["index"] = "back:" + "+".join(why)
            assert f2 == (length - 2) | F_LAZY, "the second k_lz_sort launch sorts every position of a block handed back"
        else:
            assert f1 == f0 == f2 and maxc <= 4096 and not idxw & 0xC0000000
            r["index"] = "regs" if maxc <= 512 else "radix"
        final = f2
    else:
        assert f1 == 0 and f2 == 0 and idxw == 0 and not f0 & F_REDO
        r["sort"] = "nokeys" if length < 3 else {0: "one", 1: "two", 2: "dense"}[sortw]
        r["index"] = None
        final = f0
        if sortw == 2:
            assert f0 == (length - 2) | F_LAZY
    r["kept"] = final & F_COUNT
    if final & F_LAZY:
        assert ml0 == 0xFFFFFFFF and tm0 == 1, "a lazy block leaves its chain as a mask"
        r["match"], r["nml"], r["parse"] = "lazy", None, "mask"
        r["lazy"] = tuple(name for k, name in enumerate(LAZY_BITS) if lz >> k & 1)
        assert lz < 64 and bool(lz & 1) == (r["index"] in ("regs", "radix")), "guarded: the blocks k_lz_index took"
    else:
        assert ml0 != 0xFFFFFFFF and tm0 == 0 and lz == 0
        r["nml"], r["lazy"] = ml0, None
        r["match"] = "list_only" if r["kept"] <= MLIST_CAP else ("listed" if ml0 <= MLIST_CAP else "overflow")
        r["parse"] = "list" if ml0 <= MLIST_CAP else "maps"
        assert ml0 <= r["kept"]
    r["ntok"] = ntok
    return r


def route_matches(got, want):
    """The fields of `want` (a case's expected route: every field but the counts it does not state) against a decoded record."""
    need = {"sort", "index", "match", "lazy", "parse"}
    assert need <= set(want), "an expected route states %s" % sorted(need)
    return {k: got[k] for k in want} == want


# ---------------------------------------------------------------------------------------------
# the kernels' integer decisions, restated
# ---------------------------------------------------------------------------------------------
def _keys_le(block):
    """Key of every position as the kernels read it: the three bytes as a little-endian number."""
    b = np.asarray(block, dtype=np.uint8).astype(np.uint32)
    return b[:-2] | (b[1:-1] << 8) | (b[2:] << 16) if b.size >= 3 else np.zeros(0, dtype=np.uint32)


def _h19(key, mul):
    return ((key.astype(np.uint64) * mul) & 0xFFFFFFFF) >> 13


def sort_model(block):
    """k_lz_sort, first launch, on a block: (sort, kept) with sort as decode_route names it.  The filter's counters
    (two bits per slot of a 2^19 table, two hashes), the density sample (every sixteenth position) and the heavy-key
    sample (one position in each run of sixteen, counted per 2048 classes) with the kernel's own integer tests."""
    block = np.asarray(block, dtype=np.uint8)
    T = block.size
    if T < 3:
        return "nokeys", 0
    cnt = T - 2
    key = _keys_le(block)
    h = _h19(key, 0x9E3779B1)
    keep = np.bincount(h, minlength=1 << 19)[h] >= 2
    samp = keep[::16]
    kept, tried = int(samp.sum()), samp.size
    if kept * 4 >= tried * 3:  # dense
        runs = np.arange(0, cnt, 16, dtype=np.uint64)  # run c of thread tid starts at 128 tid + 16 c
        tid, c = runs // 128, (runs % 128) // 16
        sp = np.minimum(runs + ((((tid * 8 + c) * 0x9E3779B1) & 0xFFFFFFFF) >> 28), max(T - 8, 0)).astype(np.int64)
        if T >= 8:
            b = block.astype(np.uint32)
            ky = b[sp] | (b[sp + 1] << 8) | (b[sp + 2] << 16)
        else:
            ky = np.zeros(sp.size, dtype=np.uint32)
        cc = np.bincount(_h19(ky, 0x9E3779B1) >> 8, minlength=2048)
        thr = max(2, (32 * cnt + BLK - 1) >> 17)
        heavy = int(cc[cc > thr].sum())
        return ("to_index", cnt) if heavy * 256 <= cnt else ("dense", cnt)
    if kept * 5 < tried * 2:
        k2 = key[keep]
        h2 = (((k2 ^ (k2 >> 11)).astype(np.uint64) * 0xC2B2AE35) & 0xFFFFFFFF) >> 13
        return "two", int((np.bincount(h2, minlength=1 << 19)[h2] >= 2).sum())
    return "one", int(keep.sum())


def index_model(block):
    """k_lz_index on a block k_lz_sort left to it: 'regs' | 'radix' | 'back:<reasons>' from the class sizes under its
    hash (key * 0x9E3779 mod 2^24, top eleven bits)."""
    cnt = len(block) - 2
    cls = ((_keys_le(block).astype(np.uint64) * 0x9E3779) & 0xFFFFFF) >> 13
    size = np.bincount(cls, minlength=2048)
    maxc, gmax = int(size.max()), int(size.reshape(16, 128).sum(axis=1).max())
    hv = max(128, (512 * cnt + BLK - 1) >> 17)
    nheavy = int(size[size > hv].sum())
    why = (["class"] if maxc > 4096 else []) + (["group"] if gmax > 16384 else []) + (["heavy"] if nheavy * 16 > cnt else [])
    if why:
        return "back:" + "+".join(why)
    return "regs" if maxc <= 512 else "radix"


def prev_same_key(block):
    """Per position with a key: the distance to the nearest earlier position of the same key (0: none)."""
    key = _keys_le(block)
    order = np.argsort(key, kind="stable")
    ks, ps = key[order], order.astype(np.int64)
    d = np.zeros(key.size, dtype=np.int64)
    same = np.zeros(key.size, dtype=bool)
    same[1:] = ks[1:] == ks[:-1]
    d[ps[same]] = ps[same] - ps[np.nonzero(same)[0] - 1]
    return d


def eager_matches(block, tail=300):
    """Matches k_lz_match finds in a block: the positions whose nearest earlier position of the same key lies within
    32768.  (A match must also end three bytes in front of the block's end; the builders keep repeats out of the last
    `tail` bytes, which is asserted here, so that every such position counts.)"""
    d = prev_same_key(block)
    assert not d[-tail:].any(), "a repeat in the block's tail"
    return int(((d > 0) & (d <= WINDOW)).sum())


# ---------------------------------------------------------------------------------------------
# the reference's LZ77, instrumented (src/lz77.ts:24-119 line by line; for the small rule cases)
# ---------------------------------------------------------------------------------------------
def ref_lz77_events(data, start, length, last):
    """(tokens in the oracle's form, set of LZ_RULES events) of one block, by a plain restatement of generateLZ77Codes.
    Bytes past the input's end read as `undefined` there: equal to each other, different from every byte."""
    a = bytes(data)
    n = len(a)
    at = lambda i: a[i] if i < n else -1
    end = start + length - 3
    index = collections.defaultdict(list)
    for i in range(start, end + 1):
        index[(at(i), at(i + 1), at(i + 2))].append(i)
    before = set()
    lo = max(0, start - WINDOW)
    for i in range(lo, max(lo, start - 2)):
        before.add((a[i], a[i + 1], a[i + 2]))
    ev, tok = set(), []

    def lcp(i, j, frm):  # first k >= frm, k <= 258, with input[i + k] !== input[j + k]; 258 when there is none
        k = frm
        while k <= 258 and at(i + k) == at(j + k):
            k += 1
        return min(k, 258) if k <= 258 else 258

    now = start
    while now <= end:
        key = (at(now), at(now + 1), at(now + 2))
        idx = index.get(key)
        if idx is None or len(idx) <= 1:
            if key in before and start > 0:
                ev.add("prev_block_only_literal")
            tok.append(a[now])
            now += 1
            continue
        base = now - 0x8000 if now > 0x8000 else 0
        i0, i1 = bisect.bisect_left(idx, base), bisect.bisect_left(idx, now)
        if i0 > 0 and idx[i0 - 1] == now - 32769:
            ev.add("dist_32769_unseen")
        best, besti, check, ge8_before, ordinal, tie = 0, 0, 0, False, 0, False
        i = i1 - 1
        stopped = None
        while i >= i0:
            if check >= 128 or (best >= 8 and check >= 16):
                stopped = i
                break
            check += 1
            c = idx[i]
            i -= 1
            if any(at(c + j) != at(now + j) for j in range(best - 1, 0, -1)):
                continue
            rl = lcp(c, now, best)
            if rl == best and best >= 3:
                tie = True
            if best < rl:
                ge8_before = best >= 8
                best, besti, ordinal = rl, c, check
                if rl >= 258:
                    break
        if stopped is not None and lcp(idx[stopped], now, 0) > best:
            ev.add("cand17_unseen" if check == 16 else "cand129_unseen" if check == 128 else "cand_limit_other")
        if best >= 3 and now + best <= end:
            if tie:
                ev.add("tie_nearer")
            if ordinal == 16 and ge8_before:
                ev.add("cand16_taken")
            if ordinal == 128:
                ev.add("cand128_taken")
            if now + best == end:
                ev.add("end_exact")
            if key == (0, 0, 0):
                ev.add("key_000000")
            if key == (255, 255, 255):
                ev.add("key_ffffff")
            tok.append(0x80000000 | (best - 3) << 16 | (now - besti - 1))
            now += best
        else:
            if best >= 3:
                if now + best == end + 1:
                    ev.add("end_plus1_literal")
                if now + best == n:
                    ev.add("run_to_input_end")
                if not last and now + best > start + length:
                    ev.add("len_through_next_block")
            tok.append(a[now])
            now += 1
    tok += [a[now], a[now + 1]] if length >= 2 else []
    ev.discard("cand_limit_other")
    return np.array(tok, dtype=np.uint32), ev


# ---------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------
def _runs(v):
    """Maximal runs of equal values: [(value, length)]."""
    out, i = [], 0
    while i < len(v):
        j = i
        while j < len(v) and v[j] == v[i]:
            j += 1
        out.append((int(v[i]), j - i))
        i = j
    return out


def header_census(tok):
    """HDR_RULES a block with these tokens (oracle form) shows, from the header the reference writes for them."""
    t = dw.from_oracle(tok)
    llens, dlens, hlit, hdist, cl_syms, clens = dw.ref_header(t)
    r = set()
    ismatch = t.dsym >= 0
    nd = len(set(t.dsym[ismatch].tolist()))
    if not ismatch.any():
        assert hdist == 1 and dlens[0] == 0
        r.add("no_match_hdist1")
        if len(tok) in (2, 3, 4, 5, 4095, 4096, 4097, 8192):
            r.add("ntok_%d" % len(tok))
        if len(set(t.sym.tolist())) == 1:
            r.add("one_literal_eob")
    if nd == 1:
        r.add("one_dist_code")
    if hlit == 286 and nd == 30:
        r.add("hlit286_dist30")
    if llens[:256].max() == 15:
        r.add("lit_code_15")
    if ismatch.any() and ((llens[t.sym] == 15) & ismatch & (t.dxn == 13)).any():
        r.add("token_15_13")
    if clens.max() == 7:
        r.add("cl_code_7")
    hclen = max(i + 1 for i in range(19) if clens[dw.CODELEN_ORDER[i]])
    assert hclen >= 5
    if hclen == 19:
        r.add("hclen_19")
    codelens = list(llens[:hlit]) + list(dlens[:hdist])
    at = 0
    for v, n in _runs(codelens):
        name = ("zrun_%d" if v == 0 else "nzrun_%d") % n
        if name in HDR_RULES:
            r.add(name)
        if at < hlit < at + n:
            r.add("run_crosses_lit_dist")
        at += n
    return r


def census(data, deep):
    """Sorted rule names the bytes show: per block the header's rules and the token-level LZ77 rules, and for `deep`
    cases (small or sparse inputs) the events of the instrumented reference, whose tokens must be the oracle's."""
    data = np.asarray(data, dtype=np.uint8)
    n, r = data.size, set()
    for start in range(0, n, BLK):
        length = min(BLK, n - start)
        tok = _oracle.lz77_block(data, start, length)
        r |= header_census(tok)
        m = tok[(tok & 0x80000000) != 0]
        ln, dist = ((m >> 16) & 0xFF) + 3, (m & 0x7FFF) + 1
        r |= {"len_%d" % k for k in (3, 257, 258) if (ln == k).any()}
        if (dist == 32768).any():
            r.add("dist_32768")
        if deep:
            mine, ev = ref_lz77_events(data, start, length, start + length == n)
            assert mine.size == tok.size and (mine == tok).all(), "the restated reference and the oracle differ"
            r |= ev
    return sorted(r)


# ---------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------
def _rnd(z, seed, n):
    return z.gen("xorshift", seed, n)


def _rnd32(z, seed, n):
    return _rnd(z, seed, 4 * n).view(np.uint32).astype(np.int64)


def _unique(z, seed, n):
    """n random bytes in which no 3-byte key occurs twice (n of a few thousand): the oracle finds no match."""
    a = _rnd(z, seed, n).copy()
    for it in range(1, 200):
        if n < 4:
            break
        key = _keys_le(a)
        _, first, cnts = np.unique(key, return_index=True, return_counts=True)
        if (cnts == 1).all():
            break
        dup = np.setdiff1d(np.arange(key.size), first)
        a[dup + 1] = (a[dup + 1].astype(np.int64) + 37 * it + dup) & 255
    assert n < 4 or np.unique(_keys_le(a)).size == n - 2
    return a


def _pieces(z, seed, n, share256):
    """Random bytes in which 64-byte pieces are, with probability share256 / 256 each, copies of an earlier piece."""
    a = _rnd(z, seed, n).copy()
    pick, src = _rnd(z, seed + 1, n // 64), _rnd32(z, seed + 2, n // 64)
    for i in range(1, n // 64):
        if pick[i] < share256:
            j = int(src[i] % i)
            a[64 * i: 64 * i + 64] = a[64 * j: 64 * j + 64]
    return a


def _pool(z, seed, n, npool):
    """A sequence of 64-byte pieces drawn from a pool of `npool` random ones: every key repeats, none is heavy, and
    nothing is periodic."""
    pool = _rnd(z, seed, 64 * npool).reshape(npool, 64)
    return pool[_rnd32(z, seed + 1, (n + 63) // 64) % npool].reshape(-1)[:n].copy()


def _stamped(z, seed, stamps):
    """A 4096-byte random pattern with one 3-byte marker stamped in `stamps` times, tiled over a block."""
    pat = _rnd(z, seed, 4096).copy()
    step = 4096 // stamps
    assert step >= 6
    for k in range(stamps):
        pat[k * step + 1: k * step + 4] = (0xA5, 0x5A, 0xC3)
    return np.tile(pat, BLK // 4096)


IDX_MUL = 0x9E3779  # k_lz_index's hash: key * IDX_MUL mod 2^24; top four bits the group, top eleven the class


def _one_group(z, seed):
    """Pieces from two pools, a fifth of them from a pool whose every key falls into group 0 of k_lz_index's hash (of the
    256 bytes that can follow two given ones, sixteen make such a key: one of them, by a random byte): a quarter of the
    block's positions in one group — above IDX_GCAP — in classes of ~250 words."""
    r = _rnd(z, seed, 64 * 128)
    g = np.zeros(64 * 128, dtype=np.uint8)
    g[:2] = r[:2]
    for i in range(2, g.size):
        two = int(g[i - 2]) | int(g[i - 1]) << 8
        good = [b for b in range(256) if (((two | b << 16) * IDX_MUL) & 0xFFFFFF) >> 20 == 0]
        g[i] = good[r[i] % len(good)]
    gp, op = g.reshape(128, 64), _rnd(z, seed + 1, 64 * 512).reshape(512, 64)
    pick, sel = _rnd(z, seed + 2, BLK // 64), _rnd32(z, seed + 3, BLK // 64)
    return np.concatenate([gp[sel[i] % 128] if pick[i] < 51 else op[sel[i] % 512] for i in range(BLK // 64)])


def _paired_markers(z, seed):
    """512 random pieces, each four times, with 36 markers stamped into them 260 times each.  The markers come in
    pairs that share a class of k_lz_index's hash (520 words and the class's own ~64: above IDX_REGCAP, eighteen such
    classes: more than a sixteenth of the block) but not a class of k_lz_sort's sample (a marker alone stays below that
    kernel's line of 512), so k_lz_sort leaves the block to k_lz_index and k_lz_index hands it back for its heavy classes."""
    seen, pairs = {}, []
    for m in _rnd(z, seed, 3 * 4000).reshape(-1, 3).astype(np.int64):
        key = int(m[0] | m[1] << 8 | m[2] << 16)
        c, sc = ((key * IDX_MUL) & 0xFFFFFF) >> 13, ((key * 0x9E3779B1) & 0xFFFFFFFF) >> 21
        if c not in seen:
            seen[c] = (key, sc, m)
        elif seen[c] is not None and seen[c][0] != key and seen[c][1] != sc:
            pairs.append((seen[c][2], m))
            seen[c] = None
        if len(pairs) == 18:
            break
    marks = [m for p in pairs for m in p]
    pool = _rnd(z, seed + 1, 64 * 512).reshape(512, 64).copy()
    slots = [(p, o) for p in range(512) for o in (2, 14, 26, 38, 50)]
    order = np.argsort(_rnd32(z, seed + 2, len(slots)), kind="stable")
    for j, m in enumerate(marks):
        for k in order[65 * j: 65 * j + 65]:
            p, o = slots[k]
            pool[p, o: o + 3] = m
    seq = np.tile(np.arange(512), 4)[np.argsort(_rnd32(z, seed + 3, 2048), kind="stable")]
    return pool[seq].reshape(-1)


def _planted(z, seed, want):
    """A random block with short repeats planted until k_lz_match finds exactly `want` matches in it."""
    a = _rnd(z, seed, BLK).copy()
    for it in range(1, 50):  # the tail: no key that occurred before (a match there could run into the block's last three bytes)
        bad = np.nonzero(prev_same_key(a)[-300:])[0]
        if bad.size == 0:
            break
        a[BLK - 2 - 300 + bad + 1] += np.uint8(it)
    spots = list(range(64, BLK - 1000, 30))  # a[p : p + 3] = a[p - 10 : p - 7]: one more match, as a rule
    k = 0
    have = eager_matches(a)
    assert have < want
    while have < want:
        take = want - have - 25 if want - have > 50 else 1  # the last ones singly: a plant can make two matches, or undo one
        for p in spots[k: k + take]:
            a[p: p + 3] = a[p - 10: p - 7]
        k += take
        have = eager_matches(a)
    assert have == want, "planting overshot: %d" % have
    return a


def _route(sort, index, match, lazy, parse, **more):
    return dict(sort=sort, index=index, match=match, lazy=lazy, parse=parse, **more)


def _route_cases(z):
    c = {}
    lazy_text = _route("dense", None, "lazy", (), "mask")
    eager_list = lambda sort, **kw: _route(sort, None, "list_only", None, "list", **kw)
    # no repeated key at all: the sort leaves at `ns == 0` (n = 2: no key, it leaves even earlier)
    c["nokeys_2"] = Case(np.array([7, 9], dtype=np.uint8), 0, 2, eager_list("nokeys", kept=0, nml=0, ntok=2), ["ntok_2"], True)
    for n in (3, 4, 300):
        rules = ["no_match_hdist1"] + (["ntok_%d" % n] if n < 5 else [])
        c["nokeys_%d" % n] = Case(_unique(z, 100 + n, n), 0, n, eager_list("two", kept=0, nml=0, ntok=n), rules, True)
    # incompressible: two filter levels, a few thousand kept, the matches listed and the words never cleared
    c["random_full"] = Case(_rnd(z, 11, BLK), 0, BLK, eager_list("two"), [], False)
    c["random_short"] = Case(_rnd(z, 12, 3000), 0, 3000, eager_list("two"), [], True)
    # a share of the 64-byte pieces are copies: one filter level, eager below half kept (the list overflows), lazy above
    c["pieces_eager"] = Case(_pieces(z, 21, BLK, 51), 0, BLK, _route("one", None, "overflow", None, "maps"), [], False)
    c["pieces_lazy"] = Case(_pieces(z, 24, BLK, 115), 0, BLK, _route("one", None, "lazy", (), "mask"), [], False)
    c["pieces_eager_short"] = Case(_pieces(z, 27, 4096, 90), 0, 4096, _route("one", None, "list_only", None, "list"), [], True)
    c["pieces_lazy_short"] = Case(_pieces(z, 30, 4096, 115), 0, 4096, _route("one", None, "lazy", (), "mask"), [], True)
    # text: dense with heavy keys, sorted by k_lz_sort itself; the chains merge
    c["text_full"] = Case(z.gen("itext", 31, BLK), 0, BLK, lazy_text, ["lit_code_15", "hclen_19"], False)
    c["text_short"] = Case(z.gen("itext", 32, 3000), 0, 3000, lazy_text, [], True)
    # text with a periodic stretch longer than LAZY_MERGE_CAP: a second chain gives up, the words are cleared late
    t = z.gen("itext", 33, BLK).copy()
    t[50000:56000] = np.tile(_rnd(z, 34, 300), 20)
    c["text_periodic_stretch"] = Case(t, 0, BLK, _route("dense", None, "lazy", ("late_clear", "walk3"), "mask"), ["hlit286_dist30"], False)
    # the 4 KiB pattern: dense without heavy keys, k_lz_index sorts every class in registers; probed and found periodic
    periodic = ("guarded", "probed", "periodic", "walk3")
    c["periodic_full"] = Case(z.gen("lowent4k", 41, BLK), 0, BLK, _route("to_index", "regs", "lazy", periodic, "mask"), [], False)
    # ... below 64 windows: no probe; the second chains give up and phase 3 walks
    c["periodic_short"] = Case(z.gen("lowent4k", 42, 20000), 0, 20000, _route("to_index", "regs", "lazy", ("guarded", "walk3"), "mask"), [], False)
    # one marker 1280 times: a class for the radix passes
    c["class_radix"] = Case(_stamped(z, 43, 40), 0, BLK, _route("to_index", "radix", "lazy", periodic, "mask"), [], False)
    # ... 5024 times: above IDX_BIGCAP, handed back, sorted by the second k_lz_sort launch; the unguarded loop on periodic data
    c["class_handed_back"] = Case(_stamped(z, 44, 157), 0, BLK, _route("to_index", "back:class", "lazy", ("late_clear", "walk3"), "mask"), [], False)
    # ... and its two other reasons: a group above the LDS's share, a sixteenth of the positions in heavy classes; the data
    # is not periodic: the unguarded loop's chains merge
    c["group_handed_back"] = Case(_one_group(z, 71), 0, BLK, _route("to_index", "back:group", "lazy", (), "mask"), [], False)
    c["heavy_handed_back"] = Case(_paired_markers(z, 81), 0, BLK, _route("to_index", "back:heavy", "lazy", (), "mask"), [], False)
    # pieces from a pool: dense, no heavy key, not periodic: probed, found not periodic
    c["pool_not_periodic"] = Case(_pool(z, 51, BLK, 1024), 0, BLK, _route("to_index", "regs", "lazy", ("guarded", "probed"), "mask"), [], False)
    # the same with a periodic stretch over the probed windows (16 g, 16 g + 1, 16 g + 2 of 512 bytes): found periodic, then
    # phase 3 runs out of its budget in the pool data between them
    a = _pool(z, 53, BLK, 1024)
    per = np.tile(_rnd(z, 55, 300), 8)[:2304]
    for g in range(16):
        a[8192 * g: 8192 * g + 2304] = per
    c["pool_probe_fooled"] = Case(a, 0, BLK, _route("to_index", "regs", "lazy", ("guarded", "probed", "periodic", "abort3", "walk3"), "mask"), [], False)
    # eager, more than 4095 kept: the words are cleared; the list holds every match up to 4095 of them
    c["planted_2000"] = Case(_planted(z, 61, 2000), 0, BLK, _route("two", None, "listed", None, "list", nml=2000), [], False)
    c["planted_4095"] = Case(_planted(z, 62, 4095), 0, BLK, _route("two", None, "listed", None, "list", nml=4095), [], False)
    c["planted_4096"] = Case(_planted(z, 63, 4096), 0, BLK, _route("two", None, "overflow", None, "maps", nml=4096), [], False)
    return c


def _put(a, at, s):
    a[at: at + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8) if not isinstance(s, np.ndarray) else s
    return at + len(s)


def _twice(a, first, second, s):
    """s at both places, with different bytes in front of and behind the two copies: the match is len(s) long exactly."""
    _put(a, first, s), _put(a, second, s)
    a[second - 1] = a[first - 1] ^ 0x80
    a[second + len(s)] = a[first + len(s)] ^ 0x80


def _lz_rule_cases(z):
    c = {}
    eager = _route("two", None, "list_only", None, "list")
    # distance 32768 is taken, 32769 is not seen (block 0: positions are distances from the input's start)
    a = _unique(z, 201, 3000)
    a = np.concatenate([a, _rnd(z, 202, 40000 - 3000)])
    w1, w2 = _rnd(z, 203, 8), _rnd(z, 204, 8)
    _put(a, 1000, w1), _put(a, 1000 + 32768, w1)
    _put(a, 2000, w2), _put(a, 2000 + 32769, w2)
    c["distance_limit"] = Case(a, 0, 40000, eager, ["dist_32768", "dist_32769_unseen"], True)
    # lengths 3, 257, 258 and a tie
    a = _unique(z, 211, 4000)
    s = _rnd(z, 212, 600)
    _twice(a, 100, 200, s[:3])
    _twice(a, 400, 800, s[10:267])
    _put(a, 1200, s[300:558]), _put(a, 1600, s[300:558])  # 258 and more
    _put(a, 1600 + 258, s[558:570]), _put(a, 1200 + 258, s[558:570])
    tie = bytes(s[580:586])
    _put(a, 2000, tie + b"\x01"), _put(a, 2100, tie + b"\x02"), _put(a, 2200, tie + b"\x03")
    c["lengths_and_tie"] = Case(a, 0, 4000, eager, ["len_3", "len_257", "len_258", "tie_nearer"], True)
    # candidate limits: K + x, the longest match the 16th / 17th / 128th / 129th nearest
    for name, nth, near8, rules in (("cand_16th", 16, True, ["cand16_taken"]), ("cand_17th", 17, True, ["cand17_unseen"]),
                                    ("cand_128th", 128, False, ["cand128_taken"]), ("cand_129th", 129, False, ["cand129_unseen"])):
        a = _unique(z, 220 + nth, 3000)
        K, X = bytes(_rnd(z, 230 + nth, 3)), bytes(_rnd(z, 240 + nth, 24))
        # (the byte in front of each occurrence: none of them the last one's, or a match from there would swallow it)
        at = 100
        at = _put(a, at, b"\x00" + K + X[:20] + bytes([X[20] ^ 0x55])) + 5  # the farthest: 23 bytes in common with the last
        for k in range(nth - 2):
            at = _put(a, at, bytes([1 + k]) + K + bytes([X[0] ^ (1 + k % 255)])) + 5  # the key alone
        at = _put(a, at, b"\xf0" + ((K + X[:5] + bytes([X[5] ^ 0x33])) if near8 else (K + bytes([X[0] ^ 0xFF])))) + 5  # the nearest: 8 in common, or 3
        _put(a, at, b"\xff" + K + X)
        c[name] = Case(a, 0, 3000, eager, rules, True)
    # block end: a match that ends exactly at endIndex = n - 3, one that is a byte longer, a run up to the input's end
    s = _rnd(z, 251, 40)
    a = _unique(z, 252, 600)
    _put(a, 100, s[:12]), _put(a, 600 - 3 - 12, s[:12])
    c["end_exact"] = Case(a, 0, 600, eager, ["end_exact"], True)
    a = _unique(z, 253, 600)
    _put(a, 100, s[:12]), _put(a, 600 - 3 - 11, s[:12])
    c["end_plus1"] = Case(a, 0, 600, eager, ["end_plus1_literal"], True)
    a = _unique(z, 254, 600)
    a[540:] = 0x58
    c["run_to_end"] = Case(a, 0, 600, eager, ["run_to_input_end"], True)
    # keys 00 00 00 and FF FF FF
    a = _unique(z, 255, 1000)
    a[100:108], a[300:308], a[500:508], a[700:708] = 0, 0, 255, 255
    c["keys_00_ff"] = Case(a, 0, 1000, eager, ["key_000000", "key_ffffff"], True)
    # two blocks: a match measured through the next block's bytes; a repeat whose only source is in the block before
    a = np.concatenate([_rnd(z, 261, BLK), _unique(z, 262, 2000)])
    w = _rnd(z, 263, 15)
    _put(a, BLK - 5000, w), _put(a, BLK - 3 - 7, w)
    w = _rnd(z, 264, 20)
    _put(a, BLK - 900, w), _put(a, BLK + 500, w)
    c["block_border"] = Case(a, 0, BLK, eager, ["len_through_next_block", "prev_block_only_literal"], True)
    return c


def _fib_counts(nsym):
    f = [1, 1]
    while len(f) < nsym:
        f.append(f[-1] + f[-2])
    return f


def _spread(z, seed, counts, symbols):
    """The symbols with the given counts in an order that repeats no 3-byte key where it can be helped: a shuffle."""
    a = np.repeat(np.asarray(symbols, dtype=np.uint8), counts)
    return a[np.argsort(_rnd32(z, seed, a.size), kind="stable")]


def _no_repeat(z, seed, a, keep=()):
    """The bytes of `a` reordered until no 3-byte key occurs twice (positions in `keep` stay): swaps, so the histogram holds."""
    a = a.copy()
    r = _rnd32(z, seed, 4096)
    fixed = np.zeros(a.size, dtype=bool)
    fixed[list(keep)] = True
    k = 0
    for it in range(400):
        key = _keys_le(a)
        _, first = np.unique(key, return_index=True)
        dup = np.setdiff1d(np.arange(key.size), first)
        dup = dup[~fixed[dup + 1]]
        if dup.size == 0:
            return a
        for p in dup[:64]:
            q = int(r[k % r.size] % a.size)
            k += 1
            if not fixed[q]:
                a[p + 1], a[q] = a[q], a[p + 1]
    raise AssertionError("repeated keys remain")


def _hdr_rule_cases(z):
    c = {}
    eager = _route("two", None, "list_only", None, "list")
    # zero runs of 138 and 139 lengths: byte 0, then the bytes from 139 (140) up, once each
    for n in (138, 139):
        a = np.concatenate([[0], np.arange(n + 1, 256)]).astype(np.uint8)
        c["zero_run_%d" % n] = Case(a, 0, a.size, eager, ["zrun_%d" % n, "no_match_hdist1"], True)
    # a run of one byte: a literal, matches of 258 at distance 1: the last literal/length length (285) and the only
    # distance length are both 1, and the reference's run-length rule runs across the border.  (One heavy key: k_lz_sort
    # keeps the block; chains of maximal matches from 512 w and from a window's exit never meet: a second chain gives up.)
    a = np.concatenate([np.full(258 * 12 + 1, 0x58), [1, 2, 3]]).astype(np.uint8)
    c["run_crossing"] = Case(a, 0, a.size, _route("dense", None, "lazy", ("late_clear", "walk3"), "mask"), ["run_crosses_lit_dist", "one_dist_code", "len_258"], True)
    # counts that double from level to level (the large levels split over many bytes, so that no key need repeat): a
    # literal/length code that wants more levels than 15: the rarest literal, end-of-block and the block's one match
    # get 15 bits, and the match, far back, 13 extra distance bits
    counts = [1, 2, 4, 8, 16, 32, 64] + [64] * 2 + [64] * 4 + [64] * 8 + [128] * 8 + [128] * 16 + [256] * 16 + [256] * 32 + [256] * 64
    a = np.repeat(np.arange(len(counts), dtype=np.uint8), counts)
    a = a[np.argsort(_rnd32(z, 331, a.size), kind="stable")]
    a[21000:21003] = a[500:503]
    a = _no_repeat(z, 332, a, keep=list(range(498, 506)) + list(range(20998, 21006)))
    c["deep_code_far_match"] = Case(a, 0, a.size, eager, ["lit_code_15", "token_15_13", "hclen_19"], True)
    for n in (5, 4095, 4096, 4097, 8192):
        c["ntok_%d" % n] = Case(_unique(z, 300 + n % 97, n), 0, n, dict(eager, ntok=n), ["ntok_%d" % n, "no_match_hdist1"], True)
    c["one_literal"] = Case(np.array([65, 65], dtype=np.uint8), 0, 2, _route("nokeys", None, "list_only", None, "list", ntok=2), ["one_literal_eob", "ntok_2"], True)
    return c


def _multi_block_cases(z):
    c = {}
    a = np.concatenate([z.gen("itext", 401, BLK), _rnd(z, 402, BLK), z.gen("lowent4k", 403, BLK), z.gen("itext", 404, 3000)])
    c["mixed_four_blocks"] = Case(a, 2 * BLK, BLK, _route("to_index", "regs", "lazy", ("guarded", "probed", "periodic", "walk3"), "mask"), [], False)
    return c


@functools.lru_cache(maxsize=None)
def _cases_cached(zid):
    z = _cases_cached.z
    c = {}
    for part in (_route_cases, _lz_rule_cases, _hdr_rule_cases, _multi_block_cases):
        new = part(z)
        assert not set(new) & set(c)
        c.update(new)
    for name, k in c.items():
        n = k.data.size
        assert k.data.dtype == np.uint8 and k.start % BLK == 0 and k.length == min(BLK, n - k.start) and n <= 4 * BLK, name
        assert set(k.rules) <= set(RULES), name
        k.data.setflags(write=False)
    return c


def cases(z):
    """name -> Case, built once per process."""
    _cases_cached.z = z
    return _cases_cached(id(z))
