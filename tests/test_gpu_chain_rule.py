"""The block-parallel inflate tier's acceptance rule (csrc/zes_chain.h) on the GPU: k_inf_chain against the host's
decision on the same candidate records, and accepted / declined / cut-off streams back to back in one context — through
the one-buffer call (the host walks the chain on the page-locked mirror) and through a batch (k_inf_chain decides)."""
import zlib as pz

import numpy as np
import pytest

import _chain_cases as cc

pytestmark = pytest.mark.gpu


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def test_device_and_host_decide_alike_on_every_case(z, gpu):
    """The fixed list and the 3000 generated cases of tests/test_chain_rule_cpu.py: status, total, aux and chain from
    k_inf_chain equal the host's, case by case."""
    cases = [(name, c[:3]) for name, c in cc.fixed_cases().items()] + [("seed %d" % s, cc.generated(s)) for s in range(3000)]
    seen = {0: 0, 1: 0, 2: 0}
    for name, (recs, cap, first_bit) in cases:
        host = z.stage_chain(recs, cap, first_bit)
        device = z.stage_chain(recs, cap, first_bit, on_device=True)
        for field, d, h in zip(("status", "total", "aux", "chain"), device, host):
            assert d == h, "%s: %s on the device %r, on the host %r" % (name, field, d, h)
        seen[host[0]] += 1
    print("verdicts:", seen)
    assert min(seen.values()) >= 300


def _expect(oracle, data):
    try:
        return 0, oracle.inflate(data)
    except oracle.OracleError as e:
        return e.code, None


@pytest.mark.parametrize("form", ["one buffer: the host walks the chain", "two buffers: the device chain"])
def test_accepted_declined_cut_accepted_back_to_back(z, oracle, gpu, form):
    """What a call leaves in the page-locked mirror and the device lists must not reach the next call's verdict: a
    reference-made stream (block-parallel tier), another encoder's stream of similar size (declined there, decoded by
    the segment-parallel tier), the reference-made stream cut at two thirds (the oracle's answer: nothing accepts it),
    the reference-made stream again."""
    import torch

    n = 3 << 20
    plain = z.gen("itext", 9001, n)
    ref = oracle.deflate(plain)
    foreign = np.frombuffer(pz.compress(plain.tobytes(), 6), dtype=np.uint8)
    assert 0.5 < foreign.size / ref.size < 2
    cut = ref[: ref.size * 2 // 3].copy()
    want_cut = _expect(oracle, cut)  # (the reference throws on it)
    calls = [("reference-made", ref, (0, plain), 1), ("another encoder's", foreign, (0, plain), 2), ("cut at two thirds", cut, want_cut, None),
             ("reference-made again", ref, (0, plain), 1)]
    for name, comp, (code, want), tier in calls:
        out = torch.zeros(2 * n + 32, dtype=torch.uint8, device=gpu)
        if form.startswith("one"):
            try:
                got_code, got = 0, z.inflate_tensor(dev(comp, gpu), out[:n]).cpu().numpy()
            except z.ZlibEsError as e:
                got_code, got = e.code, None
            results = [(got_code, got)]
        else:
            size = (comp.size + 15) // 16 * 16
            both = np.zeros(2 * size, dtype=np.uint8)
            both[: comp.size] = comp
            both[size: size + comp.size] = comp
            olen, st = z.inflate_batch_tensor(dev(both, gpu), [0, size], [comp.size] * 2, out, [0, n + 16], [n, n])
            host = out.cpu().numpy()
            results = [(st[k], host[off: off + olen[k]] if st[k] == 0 else None) for k, off in enumerate((0, n + 16))]
        print(form, "|", name, "| tier", z.last_inflate_tier(), "| status", [r[0] for r in results])
        for got_code, got in results:
            assert got_code == code, (name, got_code, code)
            if code == 0:
                assert got.size == want.size and np.array_equal(got, want), name
        if tier is not None:
            assert z.last_inflate_tier() == tier, (name, z.last_inflate_tier())
