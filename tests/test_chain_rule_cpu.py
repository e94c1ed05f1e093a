"""The block-parallel inflate tier's acceptance rule (csrc/zes_chain.h) without a GPU: zes_stage_chain decided on the host
— the function a one-buffer inflate call decides with — against the rule restated in tests/_chain_cases.py."""
import collections

import pytest

import _chain_cases as cc


def test_fixed_cases_host_decision_is_the_restated_rule(z):
    for name, (recs, cap, first_bit, verdict) in cc.fixed_cases().items():
        want = cc.restate(recs, cap, first_bit)
        assert want[0] == verdict, name  # the case is what its name says
        got = z.stage_chain(recs, cap, first_bit)
        for field, g, w in zip(("status", "total", "aux", "chain"), got, want):
            assert g == w, "%s: %s %r, restated rule %r" % (name, field, g, w)


def test_early_final_block_is_accepted_with_the_shorter_total(z):
    recs, cap, first_bit, _ = cc.fixed_cases()["early final block"]
    assert z.stage_chain(recs, cap, first_bit) == (0, 5 * cc.BLK, 5, [0, 1, 2, 3, 4])


def test_generated_cases_host_decision_is_the_restated_rule(z):
    """3000 seeded cases, every one compared.  The generator's own verdict counts (restatement alone, seeds 0 - 2999):
    644 accepted, 1005 accepted with shifted slots, 1351 declined."""
    seen = collections.Counter()
    for seed in range(3000):
        recs, cap, first_bit = cc.generated(seed)
        want = cc.restate(recs, cap, first_bit)
        got = z.stage_chain(recs, cap, first_bit)
        for field, g, w in zip(("status", "total", "aux", "chain"), got, want):
            assert g == w, "seed %d: %s %r, restated rule %r" % (seed, field, g, w)
        seen[want[0]] += 1
    print("verdicts:", dict(seen))
    for status in (0, 1, 2):
        assert seen[status] >= 300, "verdict %d in %d of 3000 cases" % (status, seen[status])


def test_arguments_that_are_no_case_of_the_rule(z):
    c3 = cc.true_chain([300000, 280000, 90000])
    with pytest.raises(z.ZlibEsError) as e:
        z.stage_chain([c3[1], c3[0], c3[2]], 66)  # not ascending: the walk's binary search assumes the order
    assert e.value.code == z.ZES_E_ARG
    with pytest.raises(z.ZlibEsError):
        z.stage_chain([c3[0], c3[0]], 66)  # not strictly
    with pytest.raises(z.ZlibEsError):
        z.stage_chain([(8, 100, 1, 3)], 66, 8)  # in front of the zlib header's end
    L = z.lib()
    import ctypes as C

    st, tot, aux = C.c_int32(), C.c_uint64(), C.c_uint32()
    assert L.zes_stage_chain(None, None, None, None, 3, 66, 16, 0, C.byref(st), C.byref(tot), C.byref(aux), None) == z.ZES_E_ARG
    assert L.zes_stage_chain(None, None, None, None, 0, 66, 16, 0, C.byref(st), C.byref(tot), C.byref(aux), None) == 0 and st.value == 1
