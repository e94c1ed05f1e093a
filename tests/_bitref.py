"""Bit-level reference of the join of DEFLATE bit streams: plain numpy, one bit per array element.

Independent of shard.join_host and of zes_deflate_join_dev, which the tests hold against it.  Bit k of a stream is
bit k % 8 (from the least significant) of its byte k // 8 (src/utils/BitWriteStream.ts).
"""
import numpy as np


def concat_bits(pieces, nbits):
    """The first nbits[i] bits of every piece, one behind the other -> (bytes, zero padded to a byte; total bits)."""
    parts = []
    for p, n in zip(pieces, nbits):
        if n:
            parts.append(np.unpackbits(np.asarray(p, dtype=np.uint8)[: (n + 7) // 8], bitorder="little")[:n])
    bits = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return np.packbits(bits, bitorder="little"), int(bits.size)


def zlib_frame(body, adler):
    """78 9C | body (already padded to a byte) | Adler-32 big-endian (src/zlib.ts:28-46)."""
    head = np.array([0x78, 0x9C], dtype=np.uint8)
    tail = np.frombuffer(int(adler).to_bytes(4, "big"), dtype=np.uint8)
    return np.concatenate([head, np.asarray(body, dtype=np.uint8), tail])
