"""The hand-built DEFLATE writer (tests/_deflate_writer.py) checked against the reference's encoder, CPython's zlib and
the oracle: no GPU needed.  The GPU tests of tests/test_gpu_handbuilt_streams.py trust these streams."""
import time
import zlib

import numpy as np
import pytest

import _deflate_writer as W
import _handbuilt_cases as H

B = 131072


@pytest.mark.parametrize("kind", ["itext", "xorshift", "lowent4k"])
def test_reference_style_blocks_reproduce_the_oracle(z, oracle, kind):
    a = z.gen(kind, 17, 3 * B + 4321)
    for start, length, final in ((0, B, False), (B, B, True), (2 * B, B, False), (3 * B, 4321, True), (0, 3 * B + 4321, True)):
        want, nbits = oracle.deflate_range(a, start, length, final)
        w = W.BitWriter()
        for s in range(start, start + length, B):
            W.ref_block(w, a, s, min(B, start + length - s), final and s + B >= start + length)
        assert w.nbits == nbits and w.bytes() == want.tobytes(), (kind, start, length)


def test_bits_join_at_any_offset(oracle):
    a = np.frombuffer(H.text(B + 999, 3), dtype=np.uint8)
    piece, nbits = oracle.deflate_range(a, 0, B, False)
    tail, tbits = oracle.deflate_range(a, B, 999, True)
    for k in range(8):  # a fixed block of k literals in front: every bit phase
        w = W.BitWriter()
        W.fixed(w, W.literals(b"p" * k))
        w.raw(piece, nbits).raw(tail, tbits)
        assert w.nbits == 10 + 8 * k + nbits + tbits
        assert zlib.decompress(w.bytes(), -15) == b"p" * k + a.tobytes()


def test_token_encoding_is_fast():
    src = H.text(4 << 20, 4)
    rng = np.random.default_rng(1)
    n = 400000
    tok = W.cat([W.literals(src[: 3 << 20]), W.matches(rng.integers(3, 259, n), rng.integers(1, 32769, n))])
    ll, dl = H.lens_for(tok)
    t = time.perf_counter()
    w = W.BitWriter()
    W.dynamic(w, tok, ll, dl, True)
    raw = w.bytes()
    assert time.perf_counter() - t < 5.0  # ~1 s on a laptop-class core: numpy throughout, no loop over bits
    assert len(raw) > 2 << 20


def test_far_distance_stream(oracle):
    s = H.far_distance_stream()
    raw = s.raw()
    plain = bytes(s.plain)
    assert len(plain) >= 8 << 20
    assert zlib.decompress(raw, -15) == plain
    assert oracle.inflate_raw(raw).tobytes() == plain
    d = zlib.decompressobj(-15)
    d.decompress(raw + b"TRAILER")
    assert d.unused_data == b"TRAILER"


def test_far_distances_are_really_used():
    """The distances zlib never emits (32507..32768) are there, and at the start of blocks."""
    rng = np.random.default_rng(0)
    tok = H.far_tokens(rng, 8000, H.text(1 << 20, 2))
    assert tok.sym[0] >= 257 and W.DIST_BASE[tok.dsym[0]] + tok.dext[0] == 32768
    d = (W.DIST_BASE[tok.dsym[tok.dsym >= 0]] + tok.dext[tok.dsym >= 0])
    for far in H.FAR:
        assert (d == far).sum() > 10, far
    # zlib's own horizon: it finds a repeat at 32506 back and not at 32507
    x = np.random.default_rng(5).integers(0, 256, 32507, dtype=np.uint8).tobytes()
    assert len(zlib.compress(x[:32506] * 2, 9)) < 34000 and len(zlib.compress(x * 2, 9)) > 65000


@pytest.mark.parametrize("i", range(7))
def test_valid_shapes_agree_with_zlib_and_the_oracle(oracle, i):
    name, s = H.shape_cases()[i]
    raw, plain = s.raw(), bytes(s.plain)
    assert zlib.decompress(raw, -15) == plain, name
    assert oracle.inflate_raw(raw).tobytes() == plain, name
    d = zlib.decompressobj(-15)
    assert d.decompress(raw + b"\x01\x02tail") == plain and d.unused_data == b"\x01\x02tail", name
    assert len(raw) >= 32768, name


def test_shape_details():
    """The shapes hold what their names say."""
    cases = dict(H.shape_cases())
    assert len(cases) == 7
    # 258 as 284 + 31: zlib takes it, the bytes are 258 copies
    w = W.BitWriter()
    W.fixed(w, W.literals(b"a") + W.matches(258, 1, lcode=27), final=True)
    assert zlib.decompress(w.bytes(), -15) == b"a" * 259
    # stored blocks of 0 and 65535 bytes at every header bit phase
    w = W.BitWriter()
    phases = set()
    for k in range(8):
        W.fixed(w, W.literals(b"\xc8" * k))  # 9-bit literals: 10 + 9 k bits
        phases.add(w.nbits % 8)
        W.stored(w, b"\x00" * 65535 if k % 2 else b"")
    W.final_empty(w)
    assert phases == set(range(8)) and zlib.decompress(w.bytes(), -15) == b"".join(b"\xc8" * k + (b"\x00" * 65535 if k % 2 else b"") for k in range(8))


def test_bfinal_in_the_middle(oracle):
    raw, plain = H.bfinal_middle()
    d = zlib.decompressobj(-15)
    assert d.decompress(raw) == plain and d.eof and len(d.unused_data) > 1000
    assert oracle.inflate_raw(raw).tobytes() == plain


@pytest.mark.parametrize("n", [(1 << 27) - 1, 1 << 27, (1 << 27) + 1])
def test_one_block_of_2_to_the_27(oracle, n):
    raw = H.big_run_block(n)
    want = b"Z" * n
    assert zlib.decompress(raw, -15) == want
    blocks, ends = oracle.inflate_blocks(b"\x78\x9c" + raw)
    assert len(blocks) == 1 and ends == [n]


def _quirk_params():
    return [(i, where) for i, (_, _, _, anywhere) in enumerate(H.quirk_cases())
            for where in ("alone", "first", "last", "middle") if anywhere or where in ("alone", "first")]


@pytest.mark.parametrize("i,where", _quirk_params())
def test_quirk_cases_behave_as_claimed(oracle, i, where):
    name, fn, claim, _ = H.quirk_cases()[i]
    raw = H.quirk_stream(fn, where)
    with pytest.raises(zlib.error):  # outside what zlib accepts (so outside what any zlib-made stream holds)
        zlib.decompress(raw, -15)
    if where != "alone":
        return
    if isinstance(claim, int):
        with pytest.raises(oracle.OracleError) as ei:
            oracle.inflate_raw(raw)
        assert ei.value.code == claim, name
    else:
        assert oracle.inflate_raw(raw).tobytes() == claim, name


def test_quirk_results_carry_through_a_spliced_stream(oracle):
    """A quirk that does not stop the reference leaves the bytes around it as they would be alone."""
    for name, fn, claim, anywhere in H.quirk_cases():
        if isinstance(claim, int) or not anywhere:
            continue
        before, after = H.text(2 << 20, 50), H.text(200000, 60)
        got = oracle.inflate_raw(H.quirk_stream(fn, "middle")).tobytes()
        assert got == before + claim + after, name


@pytest.mark.parametrize("i", range(5))
def test_impostors_are_valid_deflate(oracle, i):
    name, raw, _ = H.impostor_cases()[i]
    d = zlib.decompressobj(-15)
    out = d.decompress(raw)
    assert d.eof, name
    assert oracle.inflate_raw(raw).tobytes() == out, name
