"""Surroundings for inputs handed to the deflate device forms at an unaligned address.

The deflate kernels read an unaligned block through fallbacks of their own (byte-wise assembly of the words the aligned
path loads 16 bytes at a time; include/zes.h: "any alignment").  A fallback can be wrong in three ways: it can put the
bytes into another order, it can start at the rounded-down address, and it can stop at another end than the input's.
The first shows in the tokens whatever lies around the input; the other two show only if what lies around it would change
the result.  So an input d (n bytes) with the misalignment a in 0..15 is laid out as

    front || d || behind         d at byte FRONT + a of an array whose first byte is 16-byte aligned

    front    d[:FRONT + a], tiled if n is shorter: a lookup that reaches in front of the input finds, for position 0, a
             candidate that matches for the whole of `front`, and a read from the rounded-down address sees d[FRONT:]
             where d[0:] belongs
    behind   BEHIND bytes (258, the longest match, and two 16-byte groups, rounded up to a multiple of 16), in two fills:
             "run"     d's last byte, repeated
             "period"  ext[i] = ext[i - dist] behind the input, dist = the distance of the last match the oracle takes in
                       the input's last block (last_match_dist; 1 without one): a compare that runs past the input's end
                       goes on matching

Every pointer a test hands to the library lies inside such an array, with these margins: a kernel that overruns reads
bytes of the same tensor.  tests/test_align_cases_cpu.py shows with the oracle that both surroundings would be noticed.
Pure numpy."""
import numpy as np

FRONT = 32
BEHIND = (258 + 32 + 15) // 16 * 16
FILLS = ("run", "period")
assert FRONT % 16 == 0 and FRONT >= 32 and BEHIND >= 258 + 32


def last_match_dist(tok):
    """Distance of the last match token of a block's tokens (the oracle's form), 1 when the block has no match."""
    m = tok[(tok & 0x80000000) != 0]
    return int(m[-1] & 0x7FFF) + 1 if m.size else 1


def front_of(d, a):
    """d[:FRONT + a], tiled if d is shorter."""
    need = FRONT + a
    return np.tile(d, (need + d.size - 1) // d.size)[:need]


def behind_of(d, fill, dist=1, length=BEHIND):
    """`length` bytes to stand behind d: its last byte repeated ("run"), or its last `dist` bytes repeated ("period")."""
    assert fill in FILLS and 1 <= dist <= d.size
    if fill == "run":
        return np.full(length, d[-1], dtype=np.uint8)
    return np.tile(d[d.size - dist:], (length + dist - 1) // dist)[:length]


def surround(d, a, fill, dist=1):
    """(front || d || behind, FRONT + a): d at byte FRONT + a of a new array."""
    assert 0 <= a < 16 and d.dtype == np.uint8 and d.size
    arr = np.concatenate([front_of(d, a), d, behind_of(d, fill, dist)])
    return arr, FRONT + a


def arena(items):
    """Many inputs in one array, for a batch call: items = [(d, a, fill, dist), ...] -> (array, in_off).  Every input stands
    in its own front and behind, each such piece starts on a 16-byte boundary of the array, and in_off[i] % 16 == a."""
    parts, in_off, at = [], [], 0
    for d, a, fill, dist in items:
        arr, off = surround(d, a, fill, dist)
        pad = -arr.size % 16
        parts += [arr, np.full(pad, arr[-1], dtype=np.uint8)]
        in_off.append(at + off)
        at += arr.size + pad
    return np.concatenate(parts), in_off
