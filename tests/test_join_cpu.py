"""The host join (shard.join_host, shard.adler_combine) against the bit-level reference of tests/_bitref.py and CPython's
zlib.adler32, on the piece lists the device join gets in tests/test_gpu_join_seams.py.  No GPU."""
import numpy as np
import pytest

import _bitref
import _seam_cases as sc


@pytest.fixture(scope="module")
def shard():
    return sc.load_shard()


def test_bitref_on_a_stream_written_by_hand():
    """The reference itself, on bits small enough to write down: 101 | 1 | 0110 0000 1 -> 1011 0110 | 0000 1(000)."""
    pieces = [np.array([0b11111101], dtype=np.uint8), np.array([0xFF], dtype=np.uint8), np.array([0b00000110, 0xFF], dtype=np.uint8)]
    body, total = _bitref.concat_bits(pieces, [3, 1, 9])
    assert total == 13 and body.tolist() == [0b01101101, 0b00010000]
    assert _bitref.zlib_frame(body, 0x01020304).tolist() == [0x78, 0x9C, 0b01101101, 0b00010000, 1, 2, 3, 4]
    assert _bitref.concat_bits([], [])[0].size == 0


def _host_pieces(case):
    return [p if p is not None else np.zeros(0, dtype=np.uint8) for p in case.pieces]


def test_join_host_small_lists(shard):
    """Every shift against every tail, 300 short pieces, empty pieces, one piece: bits beyond a piece's nbits are set
    in what join_host is handed and must not reach the result."""
    cases = sc.small_cases()
    assert len(cases) == 32 * len(sc.TAILS) + 3 + 6 + 4
    for c in cases:
        got = shard.join_host(_host_pieces(c), c.nbits, c.adlers, c.lens)
        assert got.tobytes() == c.want.tobytes(), c.name


def test_join_host_long_piece(shard):
    c = sc.wrap_case()
    got = shard.join_host(_host_pieces(c), c.nbits, c.adlers, c.lens)
    assert got.tobytes() == c.want.tobytes()


def test_adler_combine(shard):
    lists = sc.adler_lists()
    assert len(lists) == 3 * (2 + 64) + 3 * (1 + 3 + 1)
    for name, parts, want in lists:
        assert shard.adler_combine(parts) == want, name


def test_adler_closed_forms_agree_with_zlib():
    """The closed forms the huge lengths are judged by, at lengths zlib can still be asked about."""
    import zlib

    for n in (0, 1, 65520, 65521, 65522, 200000):
        assert sc.adler_zero(n) == zlib.adler32(bytes(n))
        for head in (b"\xff" * 65521, b"abc"):
            assert sc.adler_append_zeros(zlib.adler32(head), n) == zlib.adler32(head + bytes(n))
