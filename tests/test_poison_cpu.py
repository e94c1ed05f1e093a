"""tests/_poison_cases.py pinned without a GPU: every entry point include/zes.h declares is either called by a catalogue
entry (COVERS) or left out for a stated reason (EXEMPT), and every entry's expected value traces to the CPU oracle,
CPython's zlib / gzip or a file under tests/golden/ — the oracle- and zlib-backed ones are computed here once more, by a
second source where there is one (zlib reading the oracle's stream back, the oracle encoding what a golden hash was
recorded for), otherwise from builders run again."""
import fnmatch
import os
import re

import pytest

import _poison_cases as P
from conftest import ROOT


def declared_entry_points():
    text = open(os.path.join(ROOT, "include", "zes.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(zes_[a-z0-9_]+)\s*\(", text, flags=re.M)))


@pytest.fixture(scope="module")
def entries(z, oracle):
    return list(P.catalogue(z, oracle).values())


def test_every_entry_point_is_covered_or_exempt(entries):
    names = declared_entry_points()
    assert len(names) >= 60 and "zes_stage_poison" in names and "zes_inflate_dev" in names
    assert not set(P.COVERS) & set(P.EXEMPT)
    for n in names:
        assert n in P.COVERS or n in P.EXEMPT, "%s is neither in COVERS nor in EXEMPT" % n
    for n in list(P.COVERS) + list(P.EXEMPT):
        assert n in names, "%s is not declared in include/zes.h" % n
    for n, why in P.EXEMPT.items():
        assert isinstance(why, str) and len(why) > 10, n


def test_covers_names_entries_that_make_the_call(entries):
    for fn, patterns in P.COVERS.items():
        for pat in patterns:
            assert any(fn in e.calls for e in P.covering(entries, pat)), "%s: no catalogue entry that matches %r calls it" % (fn, pat)
        assert any(fn in e.calls for pat in patterns for e in P.covering(entries, pat)), "%s: none of %r calls it" % (fn, patterns)
    for e in entries:
        for fn in e.calls:
            assert fn in P.COVERS and any(fnmatch.fnmatchcase(e.name, p) for p in P.COVERS[fn]), "%s calls %s, which COVERS does not say" % (e.name, fn)


def test_the_named_lists_are_catalogue_entries(z, oracle, entries):
    have = {e.name for e in entries}
    assert len(P.SUBSET) == 12 and set(P.SUBSET) <= have
    assert len(P.spoilers(z, oracle)) == 4
    assert {small for _, _, small in P.shrinking(z, oracle)} <= have


def test_expected_values_trace_to_the_oracle_zlib_or_golden(z, oracle, entries):
    again = {e.name: e for e in P.build(z, oracle)}  # the builders once more: nothing depends on what ran before
    assert list(again) == [e.name for e in entries]
    checked = {"oracle": 0, "zlib": 0, "golden": 0}
    for e in entries:
        want = e.want()
        assert want is not None, e.name
        if e.recheck is not None:
            assert e.recheck() == want, "%s: a second source gives another value" % e.name
        elif e.source != "golden":
            assert again[e.name].want() == want, "%s: the builders give another value the second time" % e.name
        checked[e.source] += 1
    print(checked)
    assert min(checked.values()) >= 10
