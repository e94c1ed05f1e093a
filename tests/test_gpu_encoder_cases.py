"""The deflate kernels on inputs built per route and per rule (tests/_encoder_cases.py), with the route as a recorded
fact: every case's block goes through the stage entry, and zes_stage_lz77_route's record of what k_lz_sort, k_lz_index,
the two match finders and the parser did with it must be the route the case was built for.  A matcher that is wrong on
one route still writes a valid stream, only not the reference's: tokens are compared with the oracle's, whole streams
with the hashes recorded from the reference itself (tests/golden/encoder_cases.json).

Routes shown by a record (test_case, per name): `ns == 0` (nokeys_*), two filter levels (random_*), one level eager and
lazy (pieces_*), dense and heavy kept by k_lz_sort (text_*), k_lz_index with every class in registers (periodic_*), with a
class for its radix passes (class_radix), handed back for a class above 4096 words (class_handed_back), for a group above
16384 (group_handed_back), for its heavy classes (heavy_handed_back); eager list-only
(random_*), cleared words with every match listed (planted_2000, planted_4095), list overflow (planted_4096,
pieces_eager); lazy unguarded merging (text_*), with a second chain that gives up (text_periodic_stretch, run_crossing,
class_handed_back), guarded below 64 windows (periodic_short), probed and periodic (periodic_full), probed and not
periodic (pool_not_periodic), probed, periodic, then out of budget (pool_probe_fooled); parse from a mask, a list and
exit maps.  Routes and rules without a case are named, with the reason, in tests/_encoder_cases.py's docstring.

The pools are not cleared between calls, and several routes rest on "words nobody wrote are never read": test_order runs
every case after every other kind on one context, forwards and backwards."""
import hashlib

import numpy as np
import pytest

import _encoder_cases as ec
from conftest import golden

pytestmark = pytest.mark.gpu
GOLD = golden("encoder_cases.json")
NAMES = sorted(GOLD)
_TOKENS = {}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def cases(z):
    return ec.cases(z)


@pytest.fixture(scope="module")
def on_gpu(cases, gpu):
    import torch

    return {name: torch.from_numpy(k.data.copy()).to(gpu) for name, k in cases.items()}


def want_tokens(oracle, cases, name, start=None):
    """The oracle's tokens of a case's block (computed once, shared, never changed)."""
    k = cases[name]
    start = k.start if start is None else start
    if (name, start) not in _TOKENS:
        t = oracle.lz77_block(k.data, start, min(ec.BLK, k.data.size - start))
        t.setflags(write=False)
        _TOKENS[name, start] = t
    return _TOKENS[name, start]


def same_tokens(got, want, what):
    """Equal, or the first token that differs and the input position it stands on."""
    n = min(got.size, want.size)
    diff = np.nonzero(got[:n] != want[:n])[0]
    if diff.size == 0 and got.size == want.size:
        return
    i = int(diff[0]) if diff.size else n
    step = np.where(want[:i] & 0x80000000, ((want[:i] >> 16) & 0xFF) + 3, 1)
    show = lambda t: "none" if i >= t.size else ("match len %d dist %d" % (((t[i] >> 16) & 0xFF) + 3, (t[i] & 0x7FFF) + 1) if t[i] & 0x80000000 else "literal %d" % t[i])
    raise AssertionError("%s: token %d (position %d of the block): got %s, the oracle has %s; %d tokens against %d"
                         % (what, i, int(step.sum()), show(got), show(want), got.size, want.size))


def stage(z, t, k, start=None):
    start = k.start if start is None else start
    length = min(ec.BLK, k.data.size - start)
    tok = z.stage_lz77_tensor(t, start, length)
    return tok, z.stage_lz77_route(), length


@pytest.mark.parametrize("name", NAMES)
def test_case(name, z, oracle, cases, on_gpu):
    k = cases[name]
    tok, words, length = stage(z, on_gpu[name], k)
    same_tokens(tok, want_tokens(oracle, cases, name), name)
    route = ec.decode_route(words, length)
    print(name, [hex(int(w)) for w in words], route)
    assert route["ntok"] == tok.size
    assert ec.route_matches(route, k.route), "%s took %r, built for %r" % (name, route, k.route)
    comp = z.deflate(k.data)
    assert (comp.size, _sha(comp)) == (GOLD[name]["deflate_len"], GOLD[name]["deflate_sha256"]), "not the reference's stream"
    back = z.inflate(comp)
    assert back.size == k.data.size and (back == k.data).all()


def test_order(z, oracle, cases, on_gpu):
    """Every case after every other on one context, then in reverse: the same tokens and the same record both times."""
    seen = {}
    for name in NAMES + NAMES[::-1]:
        tok, words, _ = stage(z, on_gpu[name], cases[name])
        same_tokens(tok, want_tokens(oracle, cases, name), name)
        if name in seen:
            assert (words == seen[name]).all(), "%s: %r after its successors, %r after its predecessors" % (name, list(words), list(seen[name]))
        seen[name] = words


def test_one_batch(z, cases, gpu):
    """All one-block cases in one zes_deflate_batch_dev call: blocks of every route side by side in each launch.  The
    gap behind a buffer is filled with that buffer's last byte, and the buffer that ends in a run of a byte is followed
    by one that begins with the same byte: a compare must stop at the buffer's own end (src/lz77.ts reads `undefined`)."""
    import torch

    names = [n for n in NAMES if cases[n].data.size <= ec.BLK]
    names.remove("run_crossing")
    names.insert(names.index("run_to_end") + 1, "run_crossing")
    a, b = cases["run_to_end"].data, cases["run_crossing"].data
    assert a[-1] == b[0] and (a[-40:] == a[-1]).all() and (b[:40] == b[0]).all()
    up = lambda n: (n + 15) // 16 * 16
    in_off, out_off, at, ot = [], [], 0, 0
    for n in names:
        in_off.append(at)
        out_off.append(ot)
        at += up(cases[n].data.size) + 16  # (at least sixteen bytes of padding behind every buffer)
        ot += up(z.deflate_bound(cases[n].data.size))
    arena = np.zeros(at, dtype=np.uint8)
    for n, off, nxt in zip(names, in_off, in_off[1:] + [at]):
        d = cases[n].data
        arena[off: off + d.size] = d
        arena[off + d.size: nxt] = d[-1]
    out = torch.zeros(ot, dtype=torch.uint8, device=gpu)
    caps = [z.deflate_bound(cases[n].data.size) for n in names]
    olen, st = z.deflate_batch_tensor(torch.from_numpy(arena).to(gpu), in_off, [cases[n].data.size for n in names], out, out_off, caps)
    host = out.cpu().numpy()
    for n, off, ln, s in zip(names, out_off, olen, st):
        assert s == 0, n
        assert (int(ln), _sha(host[off: off + int(ln)])) == (GOLD[n]["deflate_len"], GOLD[n]["deflate_sha256"]), "%s: not the reference's stream" % n


@pytest.mark.parametrize("name", ["mixed_four_blocks", "block_border"])
def test_multi_block(name, z, oracle, cases, on_gpu):
    """Consecutive blocks of one buffer on different routes (text, random, periodic, a short last block), each against
    the oracle, one after the other on one context."""
    k = cases[name]
    routes = []
    for start in range(0, k.data.size, ec.BLK):
        tok, words, length = stage(z, on_gpu[name], k, start)
        same_tokens(tok, want_tokens(oracle, cases, name, start), "%s, block at %d" % (name, start))
        r = ec.decode_route(words, length)
        routes.append((r["sort"], r["match"]))
    print(name, routes)
    if name == "mixed_four_blocks":
        assert routes == [("dense", "lazy"), ("two", "list_only"), ("to_index", "lazy"), ("dense", "lazy")]
