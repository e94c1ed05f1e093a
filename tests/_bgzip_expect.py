"""The BGZF file zes_bgzip must write (include/zes.h), built from the CPU oracle and tests/_bgzf.py.  Plain Python, no GPU.

The input goes in chunks of 65280 bytes, a member each; a member's body is the reference's raw stream of that chunk alone,
or one stored block when that stream is longer than len + 5 bytes or the chunk is a single byte (the reference's encoder
throws on it); the end-of-file marker closes the file.
"""
import struct

import _bgzf
import _oracle

CHUNK = 65280
MEMBER_MAX = 18 + 5 + CHUNK + 8
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def chunks_of(data):
    data = bytes(data)
    return [data[i:i + CHUNK] for i in range(0, len(data), CHUNK)]


def stored_block(chunk):
    return b"\x01" + struct.pack("<HH", len(chunk), len(chunk) ^ 0xFFFF) + chunk


def body_of(chunk):
    """(body, stored?) of one chunk."""
    if len(chunk) == 1:
        return stored_block(chunk), True
    ref = _oracle.deflate_raw(chunk).tobytes()
    if len(ref) > len(chunk) + 5:
        return stored_block(chunk), True
    return ref, False


def plan(data):
    """(chunks, bodies, stored flags) of `data`."""
    chunks = chunks_of(data)
    made = [body_of(c) for c in chunks]
    return chunks, [b for b, _ in made], [s for _, s in made]


def expect(data):
    chunks, bodies, _ = plan(data)
    return _bgzf.bgzf(chunks, bodies=bodies)


def members(n):
    return (n + CHUNK - 1) // CHUNK + 1


def bound(n):
    tail = n % CHUNK
    return n // CHUNK * MEMBER_MAX + (tail + 31 if tail else 0) + 28
