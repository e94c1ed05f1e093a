"""The damage positions recorded in tests/_range_cases.py against the oracle, without a GPU: every recorded outcome is what
oracle.inflate gives today, every flip sits where its comment says, and the streams have the sizes the GPU tests count on."""
import pytest

import _range_cases as rc


@pytest.mark.parametrize("kind", sorted(rc.RANGE_STREAMS))
def test_range_flips(z, oracle, kind):
    s = rc.range_stream(z, oracle, kind)
    assert len({k for k, _, _ in rc.RANGE_FLIPS[kind]}) == 3
    for k, bit, want in rc.RANGE_FLIPS[kind]:
        assert 1 <= k < len(s.starts) - 1, "neither the first block nor the final one"
        lo, hi = s.starts[k], s.starts[k + 1]
        assert lo + (hi - lo) * 3 // 4 <= bit < hi, "in the last quarter of block k: its body"
        got, _ = rc.outcome(oracle, rc.flip(s.comp, bit))
        assert got == want, (kind, k, bit)
        assert got[0] == "err" or got[1] != s.n, "the flip must not pass for a valid stream of the same length"


@pytest.mark.parametrize("name", sorted(rc.PIPE_INPUTS))
def test_pipe_damage(z, oracle, name):
    kind, seed, n, c = rc.PIPE_INPUTS[name]
    a = z.gen(kind, seed, n)
    comp = oracle.deflate(a)
    assert len(comp) == c and c >= 8 << 20, "the pipelined host path starts at 8 MiB of stream"
    whole, back = rc.outcome(oracle, comp)
    assert whole[0] == "out" and back.tobytes() == a.tobytes()
    cases = [d for d in rc.PIPE_DAMAGE if d[0] == name]
    assert cases
    for _, dname, how, want in cases:
        if how[0] == "flip":
            byte = how[1] >> 3
            where = dname.split("_")[0]
            assert {"first": byte < 1 << 20, "middle": abs(byte - c // 2) <= 300000, "last": c - 600000 <= byte < c - 6}[where], dname
        got, _ = rc.outcome(oracle, rc.damaged(comp, how))
        assert got == want, (name, dname)
        if dname.endswith("_byte"):
            assert got[0] == "out" and got[1] == n and got != whole, dname
        if dname.endswith("_break"):
            assert got[0] == "err" or got[1] != n, dname
    if name == "xorshift13":
        assert dict((d[1], d[2]) for d in cases)["cut_two_thirds"][1] >= 8 << 20
