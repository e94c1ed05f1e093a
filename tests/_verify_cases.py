"""The batch that tests/test_gpu_inflate_batch_adler.py decodes with and without ZES_F_CHECK_ADLER: a zlib stream for
every inflate tier and path, each one intact, with one trailer bit flipped, and cut inside and in front of its trailer;
and buffers that fail for another reason, which must keep that reason."""
import zlib as pz

import numpy as np

OK, NOT_DEFLATE, NOSPACE, CHECKSUM = 0, -1, -16, -21
EMPTY = bytes.fromhex("789c030000000001")


class Case:
    def __init__(self, label, stream, raw, checked, cap=None):
        self.label = label
        self.stream = np.frombuffer(bytes(stream), dtype=np.uint8)
        self.raw = raw          # bytes the body decodes to, or the status it fails with
        self.checked = checked  # the status under ZES_F_CHECK_ADLER when the body decodes
        self.cap = cap          # output capacity (None: what the result needs)


def variants(label, stream, raw):
    """intact, one trailer bit flipped, cut to t + 3 bytes and to t bytes (t: where the trailer starts)"""
    stream = bytes(stream)
    t = len(stream) - 4
    assert pz.decompress(stream) == raw and pz.adler32(raw) == int.from_bytes(stream[t:], "big"), label
    flipped = bytearray(stream)
    flipped[t + 2] ^= 0x10
    return [Case(label + " intact", stream, raw, OK), Case(label + " trailer bit", flipped, raw, CHECKSUM),
            Case(label + " cut t+3", stream[:t + 3], raw, CHECKSUM), Case(label + " cut t", stream[:t], raw, CHECKSUM)]


def streams(z, oracle):
    """label -> (stream, raw) per tier or path"""
    text = z.gen("itext", 4242, 300000).tobytes()
    rnd = z.gen("xorshift", 9, 200000).tobytes()
    out = {"T1": (oracle.deflate(np.frombuffer(text, dtype=np.uint8)).tobytes(), text),  # reference-made: the block-parallel tier
           "T2": (pz.compress(text, 6), text),                                           # another encoder's: the segment-parallel tier
           "stored": (pz.compress(rnd, 0), rnd),
           "T3": (pz.compress(z.gen("itext", 5, 300).tobytes()), z.gen("itext", 5, 300).tobytes()),
           "empty": (EMPTY, b"")}
    for k in range(20):  # enough short streams for the side-by-side serial wavefront path
        raw = z.gen("itext", 100 + k, 2200 + 13 * k).tobytes()
        out["short%d" % k] = (pz.compress(raw), raw)
    return out


def full_batch(z, oracle):
    s = streams(z, oracle)
    assert len(s["T2"][0]) >= 4096 and len(s["stored"][0]) >= 65536  # SEG_MIN_C, STORED_MIN_C of zes_api.hip
    cases = []
    for label, (stream, raw) in s.items():
        cases += variants(label, stream, raw)
    # a stored stream whose payload differs in one byte: the body decodes cleanly, to other bytes
    stream, raw = s["stored"]
    other, oraw = bytearray(stream), bytearray(raw)
    other[2 + 5 + 1000] ^= 0x01  # (78 01, the first stored block's 5 header bytes, payload byte 1000)
    oraw[1000] ^= 0x01
    assert pz.decompressobj(-15).decompress(bytes(other[2:-4])) == bytes(oraw)  # (the raw stream between header and trailer)
    cases.append(Case("stored payload byte", other, bytes(oraw), CHECKSUM))
    cases += others(z, oracle, s)
    return cases


def others(z, oracle, s):
    """buffers that fail for a reason of their own"""
    damaged = bytearray(s["T1"][0])
    damaged[10] ^= 0x55  # (inside the first block's code lengths: the reference refuses the stream)
    try:
        want = oracle.inflate(np.frombuffer(bytes(damaged), dtype=np.uint8)).tobytes()
    except oracle.OracleError as e:
        want = e.code
    assert isinstance(want, int), "the damaged body still decodes"
    return [Case("damaged body", damaged, want, None), Case("no space", s["T2"][0], s["T2"][1], NOSPACE, cap=1000),
            Case("first byte 0x77", b"\x77" + s["T3"][0][1:], NOT_DEFLATE, None)]


def small_batch(z, oracle):
    """fewer than 16 short streams: each one goes through the per-buffer serial wavefront (T3)"""
    s = streams(z, oracle)
    return variants("T3", *s["T3"]) + variants("empty", *s["empty"]) + variants("short0", *s["short0"])


def expected(case, flagged):
    """(status, out_len or None, bytes or None)"""
    if isinstance(case.raw, int):
        return case.raw, None, None
    if case.cap is not None and case.cap < len(case.raw):
        return NOSPACE, len(case.raw), None
    return (case.checked if flagged else OK), len(case.raw), case.raw
