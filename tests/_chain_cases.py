"""Candidate records for the block-parallel inflate tier's acceptance rule (csrc/zes_chain.h), and the rule restated.

A case is (records, cap, first_bit); a record is (start_bit, end_bit, out_len, flags) of one candidate block start, in
ascending start order, as the block decoder leaves them (flags: 1 decoded, 2 final).  `restate` is written from
k_inf_chain's header comment, not from the header's code: tests compare zes_stage_chain against it and, on a GPU, the
host's decision against the device's.
"""
import random

BLK = 131072
OK, FINAL = 1, 2
DECLINED = (1, 0, 0, [])


def restate(records, cap, first_bit):
    """(status, total, aux, chain): 0 = candidate k is chain block k up to the first decoded final one (aux = its index
    + 1); 2 = a chain exists but false candidates sit between its blocks (aux = its length); 1 = no chain."""
    count = len(records)
    recs = records[: min(count, cap)]
    if not recs or count > cap or recs[0][0] != first_bit:
        return DECLINED
    closing = [k for k, r in enumerate(recs) if r[3] & OK and r[3] & FINAL]
    if closing:
        K = closing[0]
        if all(recs[k][3] & OK and recs[k][2] == BLK and recs[k + 1][0] == recs[k][1] for k in range(K)):
            return 0, sum(r[2] for r in recs[: K + 1]), K + 1, list(range(K + 1))
    starts = [r[0] for r in recs]
    j, chain, total = 0, [], 0
    while True:
        _, end, length, flags = recs[j]
        if not flags & OK:
            return DECLINED
        chain.append(j)
        total += length
        if flags & FINAL:
            return 2, total, len(chain), chain
        if length != BLK or end not in starts[j + 1:]:
            return DECLINED
        j = starts.index(end, j + 1)


def true_chain(bits, last_len=BLK // 3):
    """A clean chain: block k takes bits[k] bits of the stream, every block a full slot but the final one."""
    recs, at = [], 16
    for k, b in enumerate(bits):
        last = k + 1 == len(bits)
        recs.append((at, at + b, last_len if last else BLK, OK | (FINAL if last else 0)))
        at += b
    return recs


def with_false(recs, where, kind, off=1000):
    """A false candidate `off` bits into block `where`: 'undecoded', 'garbage' (decoded, leads nowhere), 'final' (garbage
    that claims to close a chain)."""
    start = recs[where][0] + off
    assert start < recs[where][1]
    rec = {"undecoded": (start, 0, 0, 0), "garbage": (start, start + 777, 4321, OK), "final": (start, start + 555, 99, OK | FINAL)}[kind]
    return sorted(recs + [rec])


def _edit(recs, k, **kw):
    r = dict(zip(("start", "end", "len", "flags"), recs[k]))
    r.update(kw)
    return recs[:k] + [(r["start"], r["end"], r["len"], r["flags"])] + recs[k + 1:]


MUTATIONS = ("none", "not_decoded", "short_by_one", "end_plus_one", "end_minus_one", "no_final", "first_elsewhere", "over_cap", "no_candidates",
             "early_final")


def mutate(recs, chain_at, what, rng):
    """One way to break (or shorten) the chain whose blocks sit at indices chain_at of recs.  Returns (recs, cap, first_bit)."""
    cap, first_bit = len(recs) + rng.randrange(0, 3), 16
    inner = chain_at[:-1]  # the non-final blocks
    k = rng.choice(chain_at)
    if what == "not_decoded":
        recs = _edit(recs, k, flags=recs[k][3] & ~OK)
    elif what == "short_by_one" and inner:
        k = rng.choice(inner)
        recs = _edit(recs, k, len=BLK - 1)
    elif what == "end_plus_one" and inner:
        k = rng.choice(inner)
        recs = _edit(recs, k, end=recs[k][1] + 1)
    elif what == "end_minus_one" and inner:
        k = rng.choice(inner)
        recs = _edit(recs, k, end=recs[k][1] - 1)
    elif what == "no_final":
        recs = _edit(recs, chain_at[-1], flags=OK)
    elif what == "first_elsewhere":
        first_bit = 16 + rng.choice((1, 8, 64)) if rng.randrange(2) else 16
        if first_bit == 16:
            recs = _edit(recs, 0, start=recs[0][0] + 1)
    elif what == "over_cap":
        cap = len(recs) - 1
    elif what == "no_candidates":
        recs = []
    elif what == "early_final" and inner:
        k = rng.choice(inner)
        recs = _edit(recs, k, flags=OK | FINAL)
    return recs, cap, first_bit


def generated(seed):
    """A true chain of 1 - 40 blocks with 0 - 3 false candidates and one of MUTATIONS (half of the cases: none)."""
    rng = random.Random(seed)
    nblk = rng.randrange(1, 41)
    recs = true_chain([rng.randrange(20000, 1100000) for _ in range(nblk)], rng.randrange(1, BLK + 1))
    true_starts = [r[0] for r in recs]
    for _ in range(rng.choice((0, 0, 1, 1, 2, 3))):
        where = rng.randrange(len(recs))
        if recs[where][3] == 0 or recs[where][1] - recs[where][0] < 4000:
            continue
        recs = with_false(recs, where, rng.choice(("undecoded", "garbage", "final")), rng.randrange(1, 3000))
    chain_at = [k for k, r in enumerate(recs) if r[0] in true_starts]
    what = rng.choice(MUTATIONS[1:]) if rng.randrange(2) else "none"
    return mutate(recs, chain_at, what, rng)


def fixed_cases():
    """name -> (records, cap, first_bit), and the verdict each must get."""
    c3 = true_chain([300000, 280000, 90000])
    c12 = true_chain([250000 + 1000 * k for k in range(12)], 5)
    f1 = with_false(c12, 4, "undecoded")
    f3 = with_false(with_false(with_false(c12, 2, "undecoded"), 2, "garbage", 2000), 7, "final")
    cases = {
        "one block": (true_chain([70000]), 66, 16, 0),
        "many blocks": (c12, 80, 16, 0),
        "short final block": (true_chain([300000, 40], 1), 66, 16, 0),
        "full-slot final block": (true_chain([300000, 300000], BLK), 66, 16, 0),
        "one false candidate, undecoded": (f1, 80, 16, 2),
        "one false candidate, decoded garbage": (with_false(c12, 0, "garbage"), 80, 16, 2),
        "one false candidate, garbage that claims to be final": (with_false(c12, 5, "final", 5), 80, 16, 2),
        "false candidate that claims final in front of a one-block chain's end": (with_false(true_chain([70000]), 0, "final"), 66, 16, 0),
        "three false candidates": (f3, 80, 16, 2),
        "chain block not decoded": (_edit(c12, 5, flags=0), 80, 16, 1),
        "final block not decoded": (_edit(c12, 11, flags=FINAL), 80, 16, 1),
        "non-final block short by one byte": (_edit(c12, 3, len=BLK - 1), 80, 16, 1),
        "non-final block long by one byte": (_edit(c12, 3, len=BLK + 1), 80, 16, 1),
        "end bit one too far": (_edit(c12, 6, end=c12[6][1] + 1), 80, 16, 1),
        "end bit one short": (_edit(c12, 6, end=c12[6][1] - 1), 80, 16, 1),
        "end bit off behind a false candidate": (_edit(f1, 2, end=f1[2][1] + 1), 80, 16, 1),
        "no final block": (_edit(c12, 11, flags=OK), 80, 16, 1),
        "first candidate behind the expected bit": (_edit(c3, 0, start=17), 66, 16, 1),
        "expected first bit elsewhere": (c3, 66, 24, 1),
        "count above the cap": (c12, 11, 16, 1),
        "count at the cap": (c12, 12, 16, 0),
        "zero candidates": ([], 66, 16, 1),
        "zero candidates, zero cap": ([], 0, 16, 1),
        "early final block": (_edit(c12, 4, flags=OK | FINAL), 80, 16, 0),
        "early final block behind a false candidate": (_edit(f1, 9, flags=OK | FINAL), 80, 16, 2),
        "a piece's chain from a later first bit": ([(r[0] + 4000, r[1] + 4000, r[2], r[3]) for r in c3], 66, 4016, 0),
    }
    return cases
