"""The rule the pooled scratch rests on, tested directly: the library never clears its pools between calls, so a call may
read only words that the same call wrote.  zes_stage_poison (include/zes.h) fills every pool, the page-locked read-back
area, the block decoder's mirror and the large batch's result array with a chosen word and forgets what was noted about
their contents; then every call of tests/_poison_cases.py's catalogue must give its known answer (the oracle's, CPython's
zlib's, a golden file's — never the library's own).

Words, in this order: 0x00000000 is the control (close to what a fresh allocation holds; it must pass before the others
mean anything), 0x00000001 reads as "the chain mask is there" (tmask[0] == 1) and as small plausible counts, 0xA5A5A5A5
as large counts and offsets, 0xFFFFFFFF is the match list's head sentinel, every flag bit set, and the 0xFF "empty
bucket" fill.  The name of every call is printed, flushed, before it runs: a log that stops short names the call."""
import sys

import pytest

import _poison_cases as P

pytestmark = pytest.mark.gpu

WORDS = [0x00000000, 0x00000001, 0xA5A5A5A5, 0xFFFFFFFF]
word_id = lambda w: "0x%08X" % w
FIXED_AREAS = (1 << 20) + 8192 * (16 + 4)  # the page-locked area (PINNED_BYTES) and the mirror (MIRROR_ITEMS candidate results and start bits)


@pytest.fixture(scope="module")
def entries(z, oracle):
    return P.catalogue(z, oracle)


def say(*what):
    print(*what)
    sys.stdout.flush()


def check(e, z, gpu, oracle, what):
    say(what, "|", e.name)
    got = e.run(z, gpu, oracle)
    assert got == e.want(), "%s | %s: got %r, %s has %r" % (what, e.name, got, e.source, e.want())


def test_catalogue_clean(z, gpu, oracle, entries):
    """Every entry gives its expected value with no poison: a failure here is not about poison."""
    for e in entries.values():
        check(e, z, gpu, oracle, "clean")


def test_hook(z, gpu, oracle, entries):
    e = entries["deflate_dev text_short"]
    check(e, z, gpu, oracle, "before the hook")
    held = z.pool_bytes()
    filled = z.stage_poison(0)
    assert held > 0 and filled > FIXED_AREAS
    assert z.pool_bytes() == held, "the hook changed what the pools hold"
    check(e, z, gpu, oracle, "directly after the hook")
    z.trim()
    assert z.pool_bytes() == 0
    fixed = z.stage_poison(0xFFFFFFFF)  # right after zes_trim: the fixed areas alone
    # (the result array of a deflate batch above 16384 buffers, page-locked and kept until shutdown, is one of them when an
    # earlier test of the process made such a call: whole 16-byte records; alone in its process this module sees none)
    assert fixed >= FIXED_AREAS and (fixed - FIXED_AREAS) % 16 == 0, fixed
    assert z.stage_poison(1) == fixed and z.pool_bytes() == 0
    assert fixed + held - 4 * 64 < filled <= fixed + held  # whole words of every pool: up to 3 bytes less each
    check(e, z, gpu, oracle, "after trim and the hook")


@pytest.mark.parametrize("word", WORDS, ids=word_id)
def test_each_call_after_poison(z, gpu, oracle, entries, word):
    for e in entries.values():
        z.stage_poison(word)
        check(e, z, gpu, oracle, word_id(word))


@pytest.mark.parametrize("word", WORDS, ids=word_id)
def test_after_an_error(z, gpu, oracle, entries, word):
    """poison -> a call that fails -> an entry: the state a failed call leaves half written."""
    for sname, spoil in P.spoilers(z, oracle).items():
        for name in P.SUBSET:
            z.stage_poison(word)
            say(word_id(word), "| spoiler:", sname)
            spoil(z, gpu)
            check(entries[name], z, gpu, oracle, "%s after %s" % (word_id(word), sname))


def test_shrinking_calls(z, gpu, oracle, entries):
    """No poison: a call of four blocks and more of each form, then the smaller catalogue entry of the same form, which
    finds the larger call's real results in the pools.  Forwards through the forms, then backwards."""
    forms = P.shrinking(z, oracle)
    for form, big, small in forms + forms[::-1]:
        say("shrinking |", form, "| the larger call")
        got, want = big(z, gpu)
        assert got == want, (form, got, want)
        check(entries[small], z, gpu, oracle, "shrinking")
