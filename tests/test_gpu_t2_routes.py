"""Which launches the segment-parallel inflate tier makes, pinned: every case of tests/_t2_routes.py — status, tier, output
length, bytes, and the launch count per profiled name — against tests/golden/t2_routes.json, which was recorded from the
commit in front of the tier's host-side refactor (NOTES.md says which).  A reordering that sent every declined item to
the lone waves, or dropped the handover rounds, decodes the same bytes; here it shows as a count.

Every case runs twice in a row on the same context and the second record must equal the first: nothing a call leaves
behind (the survivor list, the page-locked area, the pools) reaches the next call's route.

Two routes have no small input and are kept by reading, their statements moved but not changed:
  * ratio == 0 — the symbol store does not fit (a group of more than 256 MiB of compressed data, or no memory for it);
  * the full-ring pass after a match that reaches behind the short marker ring from a segment that has outgrown its share
    of the symbol store (a stream that inflates by more than the store's symbols per compressed byte).
"""
import json

import pytest

import _t2_routes as R

pytestmark = pytest.mark.gpu

_FAILED = []


@pytest.fixture(scope="module")
def golden():
    with open(R.GOLDEN) as f:
        return json.load(f)


def test_golden_file_has_every_case(golden):
    assert sorted(golden) == sorted(R.CASES)


@pytest.mark.parametrize("name", [c for c in R.CASES if c != "pieces"])
def test_route(z, gpu, golden, name):
    try:
        first = R.run_case(z, gpu, name)
        second = R.run_case(z, gpu, name)
        print(name, first)
        assert first == golden[name], (name, first, golden[name])
        assert second == first, (name, "second run", second, first)
    except BaseException:
        _FAILED.append(name)
        raise


def test_route_pieces_in_child(golden):
    """ZES_SEG_PIECE_MB=1 is read once per process: a child, under a time limit of its own."""
    assert not _FAILED, "not started: %r failed before" % (_FAILED,)
    first, second = R.run_pieces_child()
    print("pieces", first)
    assert first == golden["pieces"], (first, golden["pieces"])
    assert second == first, ("second run", second, first)
