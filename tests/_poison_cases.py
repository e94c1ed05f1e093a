"""A catalogue of named calls, one per route, form and tier the other case modules reach, for tests/test_gpu_poison.py:
the pooled scratch is filled with a chosen word (zes_stage_poison, include/zes.h) and every call must still give its
known answer.  The library never clears its pools between calls, so a call may read only words that the same call wrote;
a stale word that happens to hold a list-head sentinel, a flag bit or a plausible count changes a route or a result.

An Entry is a thunk `run(z, gpu, oracle)` that returns a comparable value (status, lengths, hashes, tier, members, a
route's verdict) and the value it must return, `want()`, which never comes from the library under test: the CPU oracle,
CPython's zlib / gzip, or a file under tests/golden/ (`source` says which).  Nothing here is a new input: every entry is
a case of tests/_encoder_cases.py, _container_cases.py, _handbuilt_cases.py, _range_cases.py, _seam_cases.py,
_verify_cases.py, _chain_cases.py or a golden fixture, at its smallest shape.  The module imports without a GPU;
tests/test_poison_cpu.py holds COVERS / EXEMPT against include/zes.h and recomputes the expected values.
"""
import ctypes as C
import fnmatch
import functools
import hashlib
import json
import os
import zlib as pz

import numpy as np

import _bgzip_expect
import _chain_cases as cc
import _container_cases as K
import _deflate_writer as W
import _encoder_cases as ec
import _handbuilt_cases as H
import _range_cases as rc
import _seam_cases as sc
import _verify_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BLK = 131072
TAIL = 3 * BLK + 1234  # the inflate entries' streams: three blocks and a short one
NOSPACE = -16


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def golden_bytes(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else bytes(a)).hexdigest()


def u8(b):
    return b if isinstance(b, np.ndarray) else np.frombuffer(bytes(b), dtype=np.uint8)


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.array(u8(a), dtype=np.uint8, copy=True)).to(gpu)


def up16(n):
    return (int(n) + 15) // 16 * 16


class Entry:
    """name; calls: the entry points of include/zes.h it goes through; run(z, gpu, oracle) -> value; want() -> the value,
    computed once; source: where the value comes from; recheck(): the value once more, by a second way where there is one
    (another source, or the builders run again), for the CPU test."""

    def __init__(self, name, calls, run, want, source, recheck=None):
        assert source in ("oracle", "zlib", "golden"), source
        self.name, self.calls, self.run, self.source, self.recheck = name, tuple(calls), run, source, recheck
        self._want, self._have = want, False

    def want(self):
        if not self._have:
            self._want, self._have = self._want(), True
        return self._want


def outcome(z, fn):
    """("out", length, sha256) of what fn returns, or ("err", code)."""
    try:
        got = fn()
    except z.ZlibEsError as e:
        return ("err", e.code)
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    return ("out", int(len(got)), sha(got))


def oracle_outcome(oracle, blob):
    try:
        out = oracle.inflate(u8(blob))
    except oracle.OracleError as e:
        return ("err", e.code)
    return ("out", int(out.size), sha(out))


def tier_class(t):
    """1 block-parallel, 2 segment-parallel, "serial" for the wavefront and the exact restatement behind it."""
    return "serial" if t in (3, 4) else t


def inflate_dev(z, gpu, blob, cap, flags=0):
    """zes_inflate_dev -> (outcome, tier class); the capacity is the result's length (a failing stream: 1 MiB)."""
    import torch

    out = torch.empty(up16(cap), dtype=torch.uint8, device=gpu)[:cap]
    got = outcome(z, lambda: z.inflate_tensor(dev(blob, gpu), out, flags))
    return got, tier_class(z.last_inflate_tier())


# =====================================================================================================================
# deflate
# =====================================================================================================================
def _stage(z, gpu, k, start, length):
    tok = z.stage_lz77_tensor(dev(k.data, gpu), start, length)
    return tok, ec.decode_route(z.stage_lz77_route(), length)


def _deflate_entries(z, oracle):
    gold = golden("encoder_cases.json")
    cases = ec.cases(z)
    out = []
    for name in sorted(gold):
        k = cases[name]

        def run_lz(z, gpu, oracle, k=k):
            tok, route = _stage(z, gpu, k, k.start, k.length)
            return (int(tok.size), sha(tok), route["ntok"] == tok.size, ec.route_matches(route, k.route) or route)

        def want_lz(k=k):
            t = oracle.lz77_block(k.data, k.start, k.length)
            return (int(t.size), sha(t), True, True)

        out.append(Entry("lz77 " + name, ["zes_stage_lz77_dev", "zes_stage_lz77_route"], run_lz, want_lz, "oracle"))
        g = gold[name]
        out.append(Entry("deflate_dev " + name, ["zes_deflate_dev"],
                         lambda z, gpu, oracle, k=k: outcome(z, lambda: z.deflate_tensor(dev(k.data, gpu))),
                         lambda g=g: ("out", g["deflate_len"], g["deflate_sha256"]), "golden",
                         recheck=lambda k=k: (lambda c: ("out", int(c.size), sha(c)))(oracle.deflate(k.data))))

    # the one-batch arena of tests/test_gpu_encoder_cases.py::test_one_batch
    names = [n for n in sorted(gold) if cases[n].data.size <= BLK]
    names.remove("run_crossing")
    names.insert(names.index("run_to_end") + 1, "run_crossing")

    def run_batch(z, gpu, oracle):
        import torch

        in_off, out_off, at, ot = [], [], 0, 0
        for n in names:
            in_off.append(at)
            out_off.append(ot)
            at += up16(cases[n].data.size) + 16
            ot += up16(z.deflate_bound(cases[n].data.size))
        arena = np.zeros(at, dtype=np.uint8)
        for n, off, nxt in zip(names, in_off, in_off[1:] + [at]):
            d = cases[n].data
            arena[off: off + d.size] = d
            arena[off + d.size: nxt] = d[-1]
        out = torch.zeros(ot, dtype=torch.uint8, device=gpu)
        caps = [z.deflate_bound(cases[n].data.size) for n in names]
        olen, st = z.deflate_batch_tensor(dev(arena, gpu), in_off, [cases[n].data.size for n in names], out, out_off, caps)
        host = out.cpu().numpy()
        return [(n, int(s), int(ln), sha(host[off: off + int(ln)])) for n, off, ln, s in zip(names, out_off, olen, st)]

    out.append(Entry("deflate_batch_dev one batch", ["zes_deflate_batch_dev"], run_batch,
                     lambda: [(n, 0, gold[n]["deflate_len"], gold[n]["deflate_sha256"]) for n in names], "golden"))

    # consecutive blocks of one buffer on different routes
    k4 = cases["mixed_four_blocks"]
    starts = list(range(0, k4.data.size, BLK))

    def run_four(z, gpu, oracle):
        res = []
        for s in starts:
            tok, route = _stage(z, gpu, k4, s, min(BLK, k4.data.size - s))
            res.append((int(tok.size), sha(tok), route["sort"], route["match"]))
        return res

    routes4 = [("dense", "lazy"), ("two", "list_only"), ("to_index", "lazy"), ("dense", "lazy")]  # (test_multi_block's)

    def want_four():
        toks = [oracle.lz77_block(k4.data, s, min(BLK, k4.data.size - s)) for s in starts]
        return [(int(t.size), sha(t)) + r for t, r in zip(toks, routes4)]

    out.append(Entry("lz77 mixed_four_blocks, block by block", ["zes_stage_lz77_dev", "zes_stage_lz77_route"], run_four, want_four, "oracle"))

    # block ranges joined: the two three-block rows of tests/test_gpu_configs.py::test_block_ranges_join_to_the_whole_stream
    for kind, seed, n, cuts in (("xorshift", 33, 2 * BLK + 2, (0, 1, 1, 3)), ("lowent4k", 32, 3 * BLK, (0, 1, 2, 3))):
        spans = [(cuts[i] * BLK, min(n, cuts[i + 1] * BLK)) for i in range(3)]
        spans = [(lo, hi) for lo, hi in spans if hi > lo]

        def run_ranges(z, gpu, oracle, kind=kind, seed=seed, n=n, spans=spans):
            t = dev(z.gen(kind, seed, n), gpu)
            pieces, res = [], []
            for lo, hi in spans:
                p, nb, ad = z.deflate_range_tensor(t, lo, hi, final=(hi == n))
                pieces.append((p.clone(), nb, ad, hi - lo))
                res.append((int(nb), sha(p.cpu().numpy()), int(ad)))
            whole = z.deflate_join_tensors(*[[p[i] for p in pieces] for i in range(4)]).cpu().numpy()
            return res, (int(whole.size), sha(whole))

        def want_ranges(kind=kind, seed=seed, n=n, spans=spans):
            a = z.gen(kind, seed, n)
            res = []
            for lo, hi in spans:
                p, nb = oracle.deflate_range(a, lo, hi - lo, hi == n)
                res.append((int(nb), sha(p), oracle.adler32(a[lo:hi])))
            whole = oracle.deflate(a)
            return res, (int(whole.size), sha(whole))

        out.append(Entry("deflate_range + join %s" % kind, ["zes_deflate_range_dev", "zes_deflate_join_dev"], run_ranges, want_ranges, "oracle"))

    out.append(Entry("deflate_join small cases", ["zes_deflate_join_dev"], _run_joins, lambda: ([], len(_join_cases())), "zlib"))

    text = cases["text_short"].data

    def run_raw(z, gpu, oracle):
        import torch

        t = dev(text, gpu)
        o = torch.zeros(up16(z.deflate_bound(text.size)), dtype=torch.uint8, device=gpu)
        n = C.c_uint64()
        rc_ = z.lib().zes_deflate_raw_dev(t.data_ptr(), t.numel(), o.data_ptr(), o.numel(), C.byref(n))
        return (rc_, int(n.value), sha(o[: n.value].cpu().numpy()))

    out.append(Entry("deflate_raw_dev text_short", ["zes_deflate_raw_dev"], run_raw,
                     lambda: (lambda r: (0, int(r.size), sha(r)))(oracle.deflate_raw(text)), "oracle",
                     recheck=lambda: (lambda r: (0, int(r.size), sha(r)))(oracle.deflate(text)[2:-4])))
    out.append(Entry("gzip_dev text_short", ["zes_gzip_dev"], lambda z, gpu, oracle: outcome(z, lambda: z.gzip_tensor(dev(text, gpu))),
                     lambda: (lambda b: ("out", len(b), sha(b)))(W.gzip_wrap(oracle.deflate_raw(text).tobytes(), text.tobytes())), "oracle"))

    for i, e in enumerate(golden("huffman.json")[:3]):
        out.append(Entry("huff_lengths %d symbols, limit %d" % (len(e["hist"]), e["maxlen"]), ["zes_stage_huff_lengths_dev"],
                         lambda z, gpu, oracle, e=e: [int(x) for x in z.stage_huff_lengths(e["hist"], e["maxlen"])],
                         lambda e=e: list(e["lens"]), "golden",
                         recheck=lambda e=e: [int(x) for x in oracle.huff_lengths(e["hist"], e["maxlen"])]))
    return out


@functools.lru_cache(maxsize=None)
def _join_cases():
    return sc.small_cases()


def _run_joins(z, gpu, oracle):
    """Every list of _seam_cases.small_cases() through zes_deflate_join_dev, out of one arena -> (names that differ, lists)."""
    import torch

    cases = _join_cases()
    src_off, pos = [], 0
    for c in cases:
        offs = []
        for p in c.pieces:
            offs.append(None if p is None else pos)
            pos += 0 if p is None else up16(len(p))
        src_off.append(offs)
    host = np.full(max(pos, 16), 0xFF, dtype=np.uint8)
    for c, offs in zip(cases, src_off):
        for p, o in zip(c.pieces, offs):
            if p is not None:
                host[o: o + len(p)] = p
    out_off = np.cumsum([0] + [up16(len(c.want)) + 32 for c in cases]).tolist()
    src = dev(host, gpu)
    out = torch.full((out_off[-1],), 0xA5, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    lens = []
    for i, c in enumerate(cases):
        cnt = len(c.pieces)
        ptrs = (C.c_void_p * cnt)(*[None if o is None else src.data_ptr() + o for o in src_off[i]])
        n = C.c_uint64(0xDEAD)
        rc_ = z.lib().zes_deflate_join_dev(ptrs, (C.c_uint64 * cnt)(*c.nbits), (C.c_uint32 * cnt)(*c.adlers), (C.c_uint64 * cnt)(*c.lens), cnt,
                                           out.data_ptr() + out_off[i], out_off[i + 1] - out_off[i], C.byref(n))
        lens.append((rc_, n.value))
    got = out.cpu().numpy()
    bad = [c.name for i, c in enumerate(cases)
           if lens[i] != (0, len(c.want)) or got[out_off[i]: out_off[i] + len(c.want)].tobytes() != bytes(c.want)]
    return bad, len(cases)


# =====================================================================================================================
# inflate
# =====================================================================================================================
REF_KINDS = (("itext", 811), ("xorshift", 812), ("lowent4k", 813))


@functools.lru_cache(maxsize=None)
def _ref_stream(kind, seed, n):
    """(plain, the oracle's zlib stream of it)"""
    z, oracle = _ref_stream.z, _ref_stream.oracle
    a = z.gen(kind, seed, n)
    return a, oracle.deflate(a)


@functools.lru_cache(maxsize=None)
def _hand_streams():
    """The raw streams of tests/_handbuilt_cases.py, written once per process: the rare shapes with their plain bytes, every
    quirk alone and (where data may follow it) in the middle of a zlib-spliced stream, the impostors."""
    shapes = [(name, s.raw(), bytes(s.plain)) for name, s in H.shape_cases()]
    quirks = [(name, where, H.quirk_stream(fn, where)) for name, fn, _, follows in H.quirk_cases()
              for where in (("alone", "middle") if follows else ("alone",))]
    return shapes, quirks, H.impostor_cases()


def _inflate_entries(z, oracle):
    _ref_stream.z, _ref_stream.oracle = z, oracle
    out = []
    dev_calls = ["zes_inflate_dev", "zes_last_inflate_tier"]

    def ref_entry(name, kind, seed, n, flags, tier):
        def run(z, gpu, oracle):
            return inflate_dev(z, gpu, _ref_stream(kind, seed, n)[1], n, flags)

        def want():
            return ("out", n, sha(_ref_stream(kind, seed, n)[0])), tier

        def recheck():  # CPython's zlib reads the oracle's stream back to the input
            plain = pz.decompress(_ref_stream(kind, seed, n)[1].tobytes())
            return ("out", len(plain), sha(plain)), tier

        return Entry(name, dev_calls, run, want, "oracle", recheck)

    for kind, seed in REF_KINDS:
        out.append(ref_entry("inflate_dev %s" % kind, kind, seed, TAIL, 0, 1))
        out.append(ref_entry("inflate_dev %s, no fast path" % kind, kind, seed, TAIL, z.ZES_F_NO_FASTPATH, "serial"))
    # one block: what the shrinking test runs behind a four-block call
    k1 = ec.cases(z)["text_full"]

    def one_block(flags, tier):
        comp = functools.lru_cache(maxsize=None)(lambda: oracle.deflate(k1.data))
        return Entry("inflate_dev text_full, one block%s" % (", no fast path" if flags else ""), dev_calls,
                     lambda z, gpu, oracle: inflate_dev(z, gpu, comp(), k1.data.size, flags),
                     lambda: (("out", int(k1.data.size), sha(k1.data)), tier), "oracle")

    out.append(one_block(0, 1))
    out.append(one_block(z.ZES_F_NO_FASTPATH, "serial"))
    # a valid-looking dynamic header inside a block: with the loose search it reaches the block decoder
    for kind, seed in (("itext", 1093), ("xorshift", 1025)):
        out.append(ref_entry("inflate_dev false candidate %s %d, loose search" % (kind, seed), kind, seed, 1 << 20, z.ZES_F_LOOSE_CANDIDATES, 1))
    for f in golden("foreign.json"):
        out.append(Entry("inflate_dev " + f["file"], dev_calls,
                         lambda z, gpu, oracle, f=f: inflate_dev(z, gpu, golden_bytes(f["file"]), f["n"]),
                         lambda f=f: (("out", f["n"], f["output_sha256"]), 2), "golden",
                         recheck=lambda f=f: (lambda p: (("out", len(p), sha(p)), 2))(pz.decompress(golden_bytes(f["file"])))))

    # hand-built streams, through the host form (staging, the exact-size allocation) and the tier it must or must not take
    def hand(name, raw, want, tier, source, recheck=None):
        blob = W.zlib_wrap(raw)

        def run(z, gpu, oracle):
            got = outcome(z, lambda: z.inflate(blob))
            t = z.last_inflate_tier()
            return got, (tier is None or (t == tier if tier > 0 else t != -tier)) or ("tier", t)

        return Entry(name, ["zes_inflate_alloc", "zes_last_inflate_tier"], run, lambda: (want(blob), True), source,
                     recheck=None if recheck is None else (lambda: (recheck(blob), True)))

    by_oracle = lambda blob: oracle_outcome(oracle, blob)
    shapes, quirks, impostors = _hand_streams()
    for name, raw, plain in shapes:
        out.append(hand("shape: " + name, raw, lambda blob, plain=plain: ("out", len(plain), sha(plain)), 2, "zlib",
                        recheck=lambda blob: (lambda p: ("out", len(p), sha(p)))(pz.decompress(blob))))
    for name, where, raw in quirks:
        out.append(hand("quirk: %s, %s" % (name, where), raw, by_oracle, None, "oracle"))
    for name, raw, t1_ok in impostors:
        out.append(hand("impostor: " + name, raw, by_oracle, 1 if t1_ok else (-1 if t1_ok is False else None), "oracle",
                        recheck=lambda blob: (lambda p: ("out", len(p), sha(p)))(pz.decompressobj(-15).decompress(blob[2:-4]))))

    def malformed(e):
        def run(z, gpu, oracle):
            try:
                return ("out", z.inflate(bytes.fromhex(e["input"])).tobytes().hex())
            except z.ZlibEsError as ex:
                return ("err", str(ex))

        return Entry("malformed: " + e["name"], ["zes_inflate_alloc"], run,
                     lambda: ("err", e["error"]) if "error" in e else ("out", e["output"]), "golden")

    out += [malformed(e) for e in golden("inflate_cases.json")[::16]]
    runaway = golden_bytes("truncated_runaway.zz")
    out.append(Entry("inflate_dev truncated_runaway.zz", ["zes_inflate_dev"], lambda z, gpu, oracle: inflate_dev(z, gpu, runaway, 1 << 20)[0],
                     lambda: oracle_outcome(oracle, runaway), "oracle"))

    def raw_status(fn):
        """a C entry point called directly -> (status, the length it reports)"""
        n = C.c_uint64(0)
        return (int(fn(C.byref(n))), int(n.value))

    kind, seed = REF_KINDS[0]

    def run_nospace(z, gpu, oracle):
        import torch

        t, o = dev(_ref_stream(kind, seed, TAIL)[1], gpu), torch.zeros(1024, dtype=torch.uint8, device=gpu)
        return raw_status(lambda n: z.lib().zes_inflate_dev(t.data_ptr(), t.numel(), o.data_ptr(), 1024, n, 0))

    out.append(Entry("inflate_dev no space at cap 1024", ["zes_inflate_dev"], run_nospace, lambda: (NOSPACE, TAIL), "oracle"))

    def run_size(z, gpu, oracle):
        comp = _ref_stream(kind, seed, TAIL)[1]
        return raw_status(lambda n: z.lib().zes_inflate_size(comp.ctypes.data, comp.size, n, 0))

    out.append(Entry("inflate_size", ["zes_inflate_size"], run_size, lambda: (0, TAIL), "oracle"))

    # where a raw stream ends, device form: five bytes in front, eight behind
    lead, trail = b"\x05" * 5, b"TRAILING"

    def run_used(z, gpu, oracle):
        import torch

        a, comp = _ref_stream(kind, seed, TAIL)
        t = dev(lead + comp.tobytes()[2:-4] + trail, gpu)
        o = torch.zeros(up16(TAIL), dtype=torch.uint8, device=gpu)
        n, used = C.c_uint64(), C.c_uint64()
        rc_ = z.lib().zes_inflate_raw_used_dev(t.data_ptr(), t.numel(), 5, o.data_ptr(), o.numel(), C.byref(n), C.byref(used), 0)
        return (rc_, int(n.value), int(used.value), sha(o[: n.value].cpu().numpy()))

    def want_used():
        a, comp = _ref_stream(kind, seed, TAIL)
        d = pz.decompressobj(-15)
        plain = d.decompress(comp.tobytes()[2:-4] + trail)
        assert plain == a.tobytes()
        return (0, TAIL, comp.size - 6 + len(trail) - len(d.unused_data), sha(a))

    out.append(Entry("inflate_raw_used_dev", ["zes_inflate_raw_used_dev"], run_used, want_used, "zlib"))

    # batches
    for flagged in (False, True):
        def run_small(z, gpu, oracle, flagged=flagged):
            return _inflate_batch(z, gpu, vc.small_batch(z, oracle), z.ZES_F_CHECK_ADLER if flagged else 0)

        def want_small(flagged=flagged):
            return [_batch_want(c, flagged) for c in vc.small_batch(z, oracle)]

        out.append(Entry("inflate_batch_dev few short streams%s" % (", trailers checked" if flagged else ""), ["zes_inflate_batch_dev"],
                         run_small, want_small, "zlib"))

    def mixed():
        s = vc.streams(z, oracle)
        a, comp = _ref_stream(kind, seed, TAIL)
        f = golden("foreign.json")[0]
        foreign = golden_bytes(f["file"])
        return [vc.Case("reference-made", comp.tobytes(), a.tobytes(), 0), vc.Case("foreign", foreign, pz.decompress(foreign), 0)] + vc.others(z, oracle, s)[:2]

    out.append(Entry("inflate_batch_dev mixed: reference-made, foreign, corrupt, no space", ["zes_inflate_batch_dev"],
                     lambda z, gpu, oracle: _inflate_batch(z, gpu, mixed(), 0), lambda: [_batch_want(c, False) for c in mixed()], "oracle"))

    # bit ranges of one stream over three ranks
    shard = sc.load_shard()

    def run_ranges(z, gpu, oracle):
        import torch

        s = rc.range_stream(z, oracle, "itext")
        t = dev(s.comp, gpu)
        res = []
        for rank, (lo, own) in enumerate(shard.split_bits(len(s.comp), 3)):
            o = torch.zeros(s.n + BLK, dtype=torch.uint8, device=gpu)
            r = z.inflate_range_tensor(t, lo, own, rank == 0, o)
            res.append(r if r is None else tuple(int(v) for v in r) + (sha(o[: r[0]].cpu().numpy()),))
        return res

    def want_ranges():
        s = rc.range_stream(z, oracle, "itext")
        res = []
        for rank, (lo, own) in enumerate(shard.split_bits(len(s.comp), 3)):
            w = s.expect(max(lo, 16), own, rank == 0)
            res.append((w["out_len"], w["first_bit"], w["end_bit"], w["nblocks"], w["final"], sha(s.a[w["out_lo"]: w["out_lo"] + w["out_len"]])))
        return res

    out.append(Entry("inflate_range_dev itext over three ranges", ["zes_inflate_range_dev"], run_ranges, want_ranges, "oracle"))

    for name, (recs, cap, first_bit, verdict) in cc.fixed_cases().items():
        out.append(Entry("stage_chain on the device: " + name, ["zes_stage_chain"],
                         lambda z, gpu, oracle, a=(recs, cap, first_bit): tuple(z.stage_chain(*a, on_device=True)),
                         lambda a=(recs, cap, first_bit): tuple(cc.restate(*a)), "oracle",  # (the rule restated: tests/_chain_cases.py)
                         recheck=lambda a=(recs, cap, first_bit), v=verdict: (lambda r: r if r[0] == v else ("verdict", v))(tuple(cc.restate(*a)))))
    return out


def _inflate_batch(z, gpu, cases, flags):
    """The batch through zes_inflate_batch_dev -> per buffer (label, status, out_len, sha256 of the bytes), the last two
    where _verify_cases.expected states them."""
    import torch

    sizes = [c.stream.size for c in cases]
    in_off = np.cumsum([0] + [up16(n) for n in sizes]).tolist()
    h_in = np.zeros(in_off[-1] + 64, dtype=np.uint8)
    for c, o in zip(cases, in_off):
        h_in[o:o + c.stream.size] = c.stream
    caps = [c.cap if c.cap is not None else (1 << 16 if isinstance(c.raw, int) else max(len(c.raw), 16)) for c in cases]
    out_off = np.cumsum([0] + [up16(n) for n in caps]).tolist()
    d_out = torch.zeros(max(out_off[-1], 16), dtype=torch.uint8, device=gpu)
    olen, st = z.inflate_batch_tensor(dev(h_in, gpu), in_off[:-1], sizes, d_out, out_off[:-1], caps, flags)
    host = d_out.cpu().numpy()
    res = []
    for c, o, n, s, cap in zip(cases, out_off, olen, st, caps):
        _, wn, wb = vc.expected(c, bool(flags))
        res.append((c.label, int(s), None if wn is None else int(n), None if wb is None else sha(host[o:o + min(int(n), cap)])))
    return res


def _batch_want(c, flagged):
    ws, wn, wb = vc.expected(c, flagged)
    return (c.label, ws, wn, None if wb is None else sha(wb))


# =====================================================================================================================
# containers, checksums, host forms
# =====================================================================================================================
CONTAINER_CALLS = {
    "crc32 batch": ["zes_crc32_batch_dev"], "adler32 batch": ["zes_adler32_batch_dev"], "gunzip_tensor bgzf": ["zes_gunzip_dev", "zes_last_gunzip_members"],
    "gunzip bgzf": ["zes_gunzip_alloc", "zes_last_gunzip_members"], "gunzip two members": ["zes_gzip", "zes_gunzip_alloc", "zes_last_gunzip_members"],
    "bgzip_tensor": ["zes_bgzip_dev"],
    "bgzip_tensor pieces": ["zes_bgzip_dev"], "bgzf_index_tensor": ["zes_bgzf_index_dev"], "bgzf_index_tensor walk": ["zes_bgzf_index_dev"],
    "bgzf_read_tensor": ["zes_bgzf_read_dev", "zes_last_gunzip_members"], "bgzf_read": ["zes_bgzf_read", "zes_last_gunzip_members"], "inflate_batch_tensor checked": ["zes_inflate_batch_dev"],
    "inflate_batch checked": ["zes_inflate_batch_alloc"],
}
CHECKSUM_LENGTHS = (1, 65537, 131075)


def _container_entries(z, oracle):
    out = []
    for name in K.CASES:
        calls = CONTAINER_CALLS.get(name) or CONTAINER_CALLS.get(name.split(",")[0])
        if calls is None:  # the ZIP cases (tests/_zip_poison.py, tests/_zipwrite_poison.py hold the ZIP calls' entries) and the damaged files
            continue
        out.append(Entry("container: " + name, calls + ["zes_last_kernel_times", "zes_set_profiling"], lambda z, gpu, oracle, name=name: K.run_case(z, gpu, name),
                         lambda name=name: golden("container_launches.json")[name], "golden"))
    for n in CHECKSUM_LENGTHS:
        data = functools.lru_cache(maxsize=None)(lambda n=n: z.gen("itext", 900 + n % 7, n))
        out.append(Entry("crc32_dev %d bytes" % n, ["zes_crc32_dev"], lambda z, gpu, oracle, data=data: z.crc32_tensor(dev(data(), gpu)),
                         lambda data=data: pz.crc32(data().tobytes()), "zlib"))
        out.append(Entry("adler32_dev %d bytes" % n, ["zes_adler32_dev"], lambda z, gpu, oracle, data=data: z.adler32_tensor(dev(data(), gpu)),
                         lambda data=data: pz.adler32(data().tobytes()), "zlib", recheck=lambda data=data: oracle.adler32(data())))
    return out


HOST_N = 200001


def _host_entries(z, oracle):
    text = functools.lru_cache(maxsize=None)(lambda: z.gen("itext", 77, HOST_N))
    comp = functools.lru_cache(maxsize=None)(lambda: oracle.deflate(text()))
    raw = functools.lru_cache(maxsize=None)(lambda: oracle.deflate_raw(text()))
    plain_out = lambda: ("out", HOST_N, sha(text()))
    stream_out = lambda c: ("out", int(c.size), sha(c))
    by_zlib = lambda: (lambda p: ("out", len(p), sha(p)))(pz.decompress(comp().tobytes()))
    out = [
        Entry("host deflate", ["zes_deflate"], lambda z, gpu, oracle: outcome(z, lambda: z.deflate(text())), lambda: stream_out(comp()), "oracle"),
        Entry("host inflate", ["zes_inflate_alloc"], lambda z, gpu, oracle: outcome(z, lambda: z.inflate(comp())), plain_out, "oracle", by_zlib),
        Entry("host deflate_raw", ["zes_deflate_raw"], lambda z, gpu, oracle: outcome(z, lambda: z.deflate_raw(text())), lambda: stream_out(raw()), "oracle",
              recheck=lambda: stream_out(comp()[2:-4])),
        Entry("host inflate_raw at offset 3", ["zes_inflate_raw"],
              lambda z, gpu, oracle: outcome(z, lambda: z.inflate_raw(np.concatenate([np.arange(3, dtype=np.uint8), raw()]), 3)), plain_out, "oracle", by_zlib),
        Entry("host gzip", ["zes_gzip"], lambda z, gpu, oracle: outcome(z, lambda: z.gzip(text())),
              lambda: (lambda b: ("out", len(b), sha(b)))(W.gzip_wrap(raw().tobytes(), text().tobytes())), "oracle"),
        Entry("host crc32", ["zes_crc32"], lambda z, gpu, oracle: z.crc32(text()), lambda: pz.crc32(text().tobytes()), "zlib"),
        Entry("host adler32", ["zes_adler32"], lambda z, gpu, oracle: z.adler32(text()), lambda: pz.adler32(text().tobytes()), "zlib",
              recheck=lambda: oracle.adler32(text())),
    ]

    def run_inflate_into(z, gpu, oracle):  # the form with the caller's buffer
        o, n = np.zeros(HOST_N, dtype=np.uint8), C.c_uint64()
        rc_ = z.lib().zes_inflate(comp().ctypes.data, comp().size, o.ctypes.data, o.size, C.byref(n), 0)
        return (rc_, int(n.value), sha(o[: n.value]))

    out.append(Entry("host inflate into a buffer", ["zes_inflate"], run_inflate_into, lambda: (0, HOST_N, sha(text())), "oracle"))

    def run_used(z, gpu, oracle):
        got, used = z.inflate_raw_used(np.concatenate([raw(), np.frombuffer(b"TAIL", dtype=np.uint8)]), 0)
        return (int(got.size), sha(got), int(used))

    out.append(Entry("host inflate_raw_used", ["zes_inflate_raw_used"], run_used, lambda: (HOST_N, sha(text()), int(raw().size)), "oracle"))

    def run_gunzip_into(z, gpu, oracle):
        gz = u8(W.gzip_wrap(raw().tobytes(), text().tobytes()))
        o, n = np.zeros(HOST_N, dtype=np.uint8), C.c_uint64()
        rc_ = z.lib().zes_gunzip(gz.ctypes.data, gz.size, o.ctypes.data, o.size, C.byref(n), 0)
        return (rc_, int(n.value), sha(o[: n.value]))

    out.append(Entry("host gunzip into a buffer", ["zes_gunzip"], run_gunzip_into, lambda: (0, HOST_N, sha(text())), "oracle"))

    bplain = functools.lru_cache(maxsize=None)(lambda: z.gen("itext", 11, 70000))  # (_container_cases.bgzf_file(70000)'s bytes)
    out.append(Entry("host bgzip", ["zes_bgzip"], lambda z, gpu, oracle: outcome(z, lambda: z.bgzip(bplain())),
                     lambda: (lambda b: ("out", len(b), sha(b)))(_bgzip_expect.expect(bplain().tobytes())), "oracle"))

    def run_raw_dev(z, gpu, oracle):
        import torch

        t, o = dev(np.concatenate([np.zeros(16, dtype=np.uint8), raw()]), gpu), torch.zeros(up16(HOST_N), dtype=torch.uint8, device=gpu)
        n = C.c_uint64()
        rc_ = z.lib().zes_inflate_raw_dev(t.data_ptr(), t.numel(), 16, o.data_ptr(), o.numel(), C.byref(n), 0)
        return (rc_, int(n.value), sha(o[: n.value].cpu().numpy()))

    out.append(Entry("inflate_raw_dev at offset 16", ["zes_inflate_raw_dev"], run_raw_dev, lambda: (0, HOST_N, sha(text())), "oracle"))

    # three buffers, host batches
    bufs = functools.lru_cache(maxsize=None)(lambda: [text(), u8(H.text(70000, 9)), z.gen("itext", 5, 300)])

    def run_dbatch(z, gpu, oracle):
        return [("err", r.code) if isinstance(r, Exception) else ("out", int(r.size), sha(r)) for r in z.deflate_batch(bufs())]

    out.append(Entry("host deflate_batch of three", ["zes_deflate_batch"], run_dbatch, lambda: [stream_out(oracle.deflate(b)) for b in bufs()], "oracle"))

    def streams3():
        b = bufs()
        return [comp(), u8(pz.compress(b[1].tobytes(), 6)), u8(pz.compress(b[2].tobytes()))]

    def run_ibatch(z, gpu, oracle):
        return [("err", r.code) if isinstance(r, Exception) else ("out", int(r.size), sha(r)) for r in z.inflate_batch(streams3())]

    out.append(Entry("host inflate_batch of three", ["zes_inflate_batch_alloc"], run_ibatch, lambda: [("out", int(b.size), sha(b)) for b in bufs()], "zlib",
                     recheck=lambda: [oracle_outcome(oracle, s) for s in streams3()]))
    return out


# =====================================================================================================================
# the catalogue
# =====================================================================================================================
_CATALOGUE = {}


def build(z, oracle):
    """The entries, built afresh (the streams and inputs behind them are made on first use)."""
    _ref_stream.z, _ref_stream.oracle = z, oracle
    entries = _deflate_entries(z, oracle) + _inflate_entries(z, oracle) + _container_entries(z, oracle) + _host_entries(z, oracle)
    names = [e.name for e in entries]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return entries


def catalogue(z, oracle):
    """name -> Entry, in catalogue order, built once per process."""
    if not _CATALOGUE:
        _CATALOGUE.update((e.name, e) for e in build(z, oracle))
    return _CATALOGUE


# entry point of include/zes.h -> patterns of the catalogue entries that call it
COVERS = {
    "zes_stage_lz77_dev": ["lz77 *"], "zes_stage_lz77_route": ["lz77 *"], "zes_stage_huff_lengths_dev": ["huff_lengths *"],
    "zes_stage_chain": ["stage_chain on the device: *"],
    "zes_deflate_dev": ["deflate_dev *"], "zes_deflate_batch_dev": ["deflate_batch_dev *"], "zes_deflate_raw_dev": ["deflate_raw_dev *"],
    "zes_deflate_range_dev": ["deflate_range + join *"], "zes_deflate_join_dev": ["deflate_range + join *", "deflate_join small cases"],
    "zes_gzip_dev": ["gzip_dev *"],
    "zes_inflate_dev": ["inflate_dev *"], "zes_inflate_size": ["inflate_size"], "zes_inflate_alloc": ["shape: *", "quirk: *", "impostor: *", "malformed: *", "host inflate"],
    "zes_inflate_raw_dev": ["inflate_raw_dev *"], "zes_inflate_raw_used_dev": ["inflate_raw_used_dev"],
    "zes_inflate_batch_dev": ["inflate_batch_dev *", "container: inflate_batch_tensor checked"], "zes_inflate_range_dev": ["inflate_range_dev *"],
    "zes_last_inflate_tier": ["inflate_dev *", "shape: *", "quirk: *", "impostor: *"],
    "zes_crc32_dev": ["crc32_dev *"], "zes_adler32_dev": ["adler32_dev *"],
    "zes_crc32_batch_dev": ["container: crc32 batch*"], "zes_adler32_batch_dev": ["container: adler32 batch*"],
    "zes_gunzip_dev": ["container: gunzip_tensor bgzf"], "zes_gunzip_alloc": ["container: gunzip bgzf", "container: gunzip two members"],
    "zes_last_gunzip_members": ["container: gunzip*", "container: bgzf_read*"],
    "zes_bgzip_dev": ["container: bgzip_tensor*"], "zes_bgzf_index_dev": ["container: bgzf_index_tensor*"],
    "zes_bgzf_read_dev": ["container: bgzf_read_tensor"], "zes_bgzf_read": ["container: bgzf_read"],
    "zes_last_kernel_times": ["container: *"], "zes_set_profiling": ["container: *"],
    "zes_deflate": ["host deflate"], "zes_inflate": ["host inflate into a buffer"], "zes_deflate_raw": ["host deflate_raw"],
    "zes_inflate_raw": ["host inflate_raw at offset 3"], "zes_inflate_raw_used": ["host inflate_raw_used"], "zes_gzip": ["host gzip", "container: gunzip two members"],
    "zes_gunzip": ["host gunzip into a buffer"], "zes_bgzip": ["host bgzip"], "zes_crc32": ["host crc32"], "zes_adler32": ["host adler32"],
    "zes_deflate_batch": ["host deflate_batch of three"], "zes_inflate_batch_alloc": ["host inflate_batch of three", "container: inflate_batch checked"],
}

# entry point -> why no catalogue entry calls it
_LIFECYCLE = "lifecycle: it brings a context up or takes it down and runs no kernel over pool contents"
_NO_DEVICE = "host arithmetic only: it touches no device"
EXEMPT = {
    "zes_init": _LIFECYCLE + " (the gpu fixture calls it)", "zes_shutdown": _LIFECYCLE,
    "zes_trim": _LIFECYCLE + " (test_hook calls it: the pools are given back, nothing is read)",
    "zes_init_devices": "several contexts in one process: the hook walks them, the tests drive one",
    "zes_device_count": "several contexts in one process: the hook walks them, the tests drive one",
    "zes_partition": _NO_DEVICE, "zes_device_info": "reads the device's properties kept at init, no pool",
    "zes_host_alloc": "page-locked memory of the caller's, not a pool", "zes_host_free": "page-locked memory of the caller's, not a pool",
    "zes_deflate_bound": _NO_DEVICE, "zes_gzip_bound": _NO_DEVICE, "zes_bgzip_members": _NO_DEVICE, "zes_bgzip_bound": _NO_DEVICE,
    "zes_bgzf_index": "the host form walks the caller's memory on the host and touches no device",
    "zes_stage_poison": "the hook itself (test_hook)",
    "zes_selftest_lds_order": "a hardware diagnostic with no known answer but its own: it clears the two words it counts in",
    "zes_gen": _NO_DEVICE,
}

# one entry per form and tier: what runs behind every spoiler
SUBSET = [
    "lz77 periodic_full", "deflate_dev text_short", "deflate_batch_dev one batch", "gzip_dev text_short",
    "inflate_dev itext", "inflate_dev foreign_itext_300000.zz", "inflate_dev itext, no fast path",
    "inflate_batch_dev few short streams, trailers checked", "inflate_range_dev itext over three ranges",
    "container: gunzip_tensor bgzf", "host inflate", "host inflate_batch of three",
]


def spoilers(z, oracle):
    """name -> thunk(z, gpu): four calls that fail, each leaving the state of a call that ended early behind it."""
    s = vc.streams(z, oracle)
    corrupt = vc.others(z, oracle, s)[0]
    runaway = golden_bytes("truncated_runaway.zz")
    a, comp = _ref_stream(REF_KINDS[0][0], REF_KINDS[0][1], TAIL)

    def fails(got, code):
        assert got == ("err", code), got

    def nospace(z, gpu):
        import torch

        t, o, n = dev(comp, gpu), torch.zeros(1024, dtype=torch.uint8, device=gpu), C.c_uint64()
        assert z.lib().zes_inflate_dev(t.data_ptr(), t.numel(), o.data_ptr(), 1024, C.byref(n), 0) == NOSPACE and n.value == TAIL

    return {
        "a corrupt stream": lambda z, gpu: fails(inflate_dev(z, gpu, corrupt.stream, 1 << 20)[0], corrupt.raw),
        "the truncated runaway": lambda z, gpu: fails(inflate_dev(z, gpu, runaway, 1 << 20)[0], -5),
        "an inflate without space": nospace,
        "a deflate that throws": lambda z, gpu: fails(outcome(z, lambda: z.deflate_tensor(dev(z.gen("xorshift", 1, BLK + 1), gpu))), -3),
    }


def shrinking(z, oracle):
    """[(form, big(z, gpu) -> (got, want), the catalogue entry that follows it)]: a call of four blocks and more, then a
    smaller call of the same form, which finds the larger one's results in every pool."""
    cases = ec.cases(z)
    four = cases["mixed_four_blocks"].data
    comp4 = functools.lru_cache(maxsize=None)(lambda: oracle.deflate(four))
    four_out = lambda: ("out", int(four.size), sha(four))
    stream_out = lambda c: ("out", int(c.size), sha(c))
    big_foreign = golden("foreign.json")[3]

    def big_batch(z, gpu):
        cs = [vc.Case("four blocks %d" % i, comp4().tobytes(), four.tobytes(), 0) for i in range(2)]
        return _inflate_batch(z, gpu, cs, z.ZES_F_CHECK_ADLER), [_batch_want(c, True) for c in cs]

    def big_stage(z, gpu):
        k = cases["text_full"]
        tok, _ = _stage(z, gpu, k, 0, BLK)
        return sha(tok), sha(oracle.lz77_block(k.data, 0, BLK))

    def big_gzip(z, gpu):
        return outcome(z, lambda: z.gzip_tensor(dev(four, gpu))), stream_out(u8(W.gzip_wrap(oracle.deflate_raw(four).tobytes(), four.tobytes())))

    return [
        ("deflate_dev", lambda z, gpu: (outcome(z, lambda: z.deflate_tensor(dev(four, gpu))), stream_out(comp4())), "deflate_dev text_short"),
        ("stage_lz77", big_stage, "lz77 text_short"),
        ("gzip_dev", big_gzip, "gzip_dev text_short"),
        ("inflate_dev, block-parallel", lambda z, gpu: (inflate_dev(z, gpu, comp4(), four.size), (four_out(), 1)), "inflate_dev text_full, one block"),
        ("inflate_dev, serial", lambda z, gpu: (inflate_dev(z, gpu, comp4(), four.size, z.ZES_F_NO_FASTPATH), (four_out(), "serial")),
         "inflate_dev text_full, one block, no fast path"),
        ("inflate_dev, segment-parallel", lambda z, gpu: (inflate_dev(z, gpu, golden_bytes(big_foreign["file"]), big_foreign["n"]),
                                                         (("out", big_foreign["n"], big_foreign["output_sha256"]), 2)), "inflate_dev foreign_xorshift_100000.zz"),
        ("inflate_batch_dev", big_batch, "inflate_batch_dev few short streams, trailers checked"),
        ("crc32_dev", lambda z, gpu: (z.crc32_tensor(dev(four, gpu)), pz.crc32(four.tobytes())), "crc32_dev 1 bytes"),
        ("adler32_dev", lambda z, gpu: (z.adler32_tensor(dev(four, gpu)), pz.adler32(four.tobytes())), "adler32_dev 1 bytes"),
        ("host deflate", lambda z, gpu: (outcome(z, lambda: z.deflate(four)), stream_out(comp4())), "host deflate"),
        ("host inflate", lambda z, gpu: (outcome(z, lambda: z.inflate(comp4())), four_out()), "host inflate"),
    ]


def covering(entries, pattern):
    return [e for e in entries if fnmatch.fnmatchcase(e.name, pattern)]
