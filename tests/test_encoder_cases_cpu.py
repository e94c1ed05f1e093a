"""The encoder cases of tests/_encoder_cases.py against tests/golden/encoder_cases.json (made by running the reference,
tests/golden/make_encoder_cases.py): the builders still make the recorded bytes, the oracle writes the reference's stream
for them — which pins it to the reference at rules no other golden touches — and every rule of the issue's lists is
shown by a case.  The routes the cases are built for are checked here as far as they are integer decisions that can be
restated (k_lz_sort's filter and samples, k_lz_index's class sizes, k_lz_match's count); the rest is the GPU's record
(tests/test_gpu_encoder_cases.py)."""
import hashlib

import pytest

import _encoder_cases as ec
from conftest import golden

GOLD = golden("encoder_cases.json")
NAMES = sorted(GOLD)


@pytest.fixture(scope="module")
def cases(z):
    return ec.cases(z)


def test_cases_are_the_recorded_ones(cases):
    assert sorted(cases) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_case(name, cases, oracle):
    k, g = cases[name], GOLD[name]
    assert k.data.size == g["n"] and hashlib.sha256(k.data.tobytes()).hexdigest() == g["input_sha256"], "the builder makes other bytes than were recorded"
    comp = oracle.deflate(k.data)
    assert (comp.size, hashlib.sha256(comp.tobytes()).hexdigest()) == (g["deflate_len"], g["deflate_sha256"]), "the oracle's stream is not the reference's"
    census = ec.census(k.data, k.deep)
    assert census == g["census"]
    assert set(k.rules) <= set(census), "claimed but not shown: %s" % sorted(set(k.rules) - set(census))


def test_every_rule_has_a_case():
    shown = set().union(*(g["census"] for g in GOLD.values()))
    assert not set(ec.RULES) - shown, "no case shows %s" % sorted(set(ec.RULES) - shown)
    assert shown <= set(ec.RULES)


@pytest.mark.parametrize("name", NAMES)
def test_route_as_far_as_it_can_be_restated(name, cases):
    """What the case expects of the sort, of k_lz_index and of the eager matcher's count is what the restated decisions give."""
    k = cases[name]
    block = k.data[k.start: k.start + k.length]
    sort, kept = ec.sort_model(block)
    assert sort == k.route["sort"]
    if sort == "to_index":
        assert ec.index_model(block) == k.route["index"]
        kept = k.length - 2  # (handed back or not: every position is sorted)
    else:
        assert k.route["index"] is None
    if "kept" in k.route:
        assert kept == k.route["kept"]
    lazy = sort in ("dense", "to_index") or (sort == "one" and kept * 2 >= k.length - 2)
    assert lazy == (k.route["match"] == "lazy") == (k.route["lazy"] is not None)
    assert k.route["parse"] == ("mask" if lazy else "maps" if k.route["match"] == "overflow" else "list")
    if not lazy:
        assert (k.route["match"] == "list_only") == (kept <= ec.MLIST_CAP)
        if "nml" in k.route:
            assert k.route["nml"] == (ec.eager_matches(block) if kept else 0)


def test_routes_cover_the_list(cases):
    """Every route of the issue's list is the expected route of some case."""
    routes = [k.route for k in cases.values()]
    has = lambda **kw: any(all(r.get(f) == v for f, v in kw.items()) for r in routes)
    lazy = lambda *bits: has(lazy=bits)
    assert has(sort="nokeys") and has(sort="two", kept=0), "ns == 0"
    assert has(sort="two", match="list_only") and has(sort="one", match="overflow") and has(sort="one", match="lazy")
    assert has(sort="dense") and has(index="regs") and has(index="radix") and has(index="back:class") and has(index="back:group") and has(index="back:heavy")
    assert has(match="list_only") and has(match="listed") and has(match="listed", nml=4095) and has(match="overflow", nml=4096)
    assert lazy() and lazy("late_clear", "walk3") and lazy("guarded", "walk3") and lazy("guarded", "probed", "periodic", "walk3")
    assert lazy("guarded", "probed") and lazy("guarded", "probed", "periodic", "abort3", "walk3")
    assert has(parse="mask") and has(parse="list") and has(parse="maps")


def test_decode_route_reads_the_words():
    """decode_route on records written by hand from include/zes.h."""
    n = 131072
    r = ec.decode_route([2395, 0, 0, 1, 0, 57, 0, 0, 130000], n)
    assert (r["sort"], r["index"], r["match"], r["nml"], r["lazy"], r["parse"], r["kept"]) == ("two", None, "list_only", 57, None, "list", 2395)
    f = (n - 2) | 0xC0000000
    r = ec.decode_route([f, f, f, 0, 190, 0xFFFFFFFF, 1, 1 | 2 | 4 | 32, 600], n)
    assert (r["sort"], r["index"], r["match"], r["lazy"], r["parse"]) == ("to_index", "regs", "lazy", ("guarded", "probed", "periodic", "walk3"), "mask")
    r = ec.decode_route([f, (n - 2) | 0x20000000, (n - 2) | 0x80000000, 0, 5024, 0xFFFFFFFF, 1, 16 | 32, 600], n)
    assert (r["index"], r["lazy"]) == ("back:class", ("late_clear", "walk3"))
    r = ec.decode_route([60000, 0, 0, 0, 0, 4096, 0, 0, 9], n)
    assert (r["sort"], r["match"], r["parse"]) == ("one", "overflow", "maps")
