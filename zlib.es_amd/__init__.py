"""zlib.es_amd — Python host mirror of zlib.es's API over the MI355X DEFLATE engine.

The reference's public surface is two functions (``/root/reference/src/zlib.ts:11,25``):

    deflate(input: Uint8Array): Uint8Array
    inflate(input: Uint8Array): Uint8Array

both synchronous, both throwing plain ``Error`` with fixed messages.  This module keeps the
same names, argument meaning and error strings (``ZlibEsError.args[0]`` is the reference's
message) and routes every call through the C-ABI of ``include/zes.h`` (``libzes_hip.so``:
hand-written gfx950 kernels).  There is no CPU implementation here: if the library is missing
or no GPU is usable the call raises, it never falls back.

The directory name contains a dot, so it cannot be imported with a plain ``import``; load it
with ``importlib`` (see ``load()`` in ``__graft_entry__.py``) under the module name
``zlibes_amd``.

Host code in the reference's own language (TypeScript on Node over N-API) lives in
``zlib.es_amd/host/``; this Python mirror drives the same C-ABI for pytest, bench.py and
torch.distributed sharding.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("ZES_LIB") or os.path.join(_HERE, "libzes_hip.so")  # (ZES_LIB: development builds of the same library)
_lib = None

BLOCK_MAX_BUFFER_LEN = 131072  # src/const.ts:7

ZES_OK = 0
ZES_E_NOSPACE = -16
ZES_E_DEVICE = -17
ZES_E_ARG = -18
ZES_F_NO_FASTPATH = 1
ZES_F_LOOSE_CANDIDATES = 2
ZES_F_PIECES = 4
ZES_F_ALLOC_BOUND = 8
ZES_ALLOC_EARLY = 0x80000000  # in the allocator's index argument: an early request for an upper estimate (may be declined with NULL)
ZES_E_NOTRANGE = -19
ZES_E_GZIP = -20  # zes_gunzip*: not a valid gzip member (header, or a trailer cut short), or no input at all
ZES_E_CHECKSUM = -21  # a trailer does not match: gzip CRC-32 / ISIZE / FHCRC, zlib Adler-32 under ZES_F_CHECK_ADLER
ZES_E_ZIP = -22  # zes_zip_*: not a ZIP archive this reader accepts, or an entry whose local header or sizes do not fit its directory record
ZES_E_UNSUPPORTED = -23  # zes_zip_*: ZIP64, several disks, encryption, a method other than 0 or 8
ZES_E_PNG = -24  # zes_png_*: not a PNG file this reader accepts, or image data that does not fit its header
ZES_E_TIFF = -25  # zes_tiff_*: not a TIFF file this reader accepts, or image data that does not fit its directory
ZES_F_GZIP_SERIAL = 32  # zes_gunzip*: the members one after the other even where they could go as one batch (testing aid)
ZES_F_INDEX_WALK = 64  # zes_bgzf_index_dev: the members by k_gz_walk's serial chain instead of the parallel finder (testing aid, baseline)
ZES_F_PNG_INTERLACED = 128  # zes_png_decode*, zes_pngpix_dev, zes_pngpix_alloc: Adam7-interlaced files decode too (without it: ZES_E_UNSUPPORTED)
ZES_F_CHECK_ADLER = 16  # zes_inflate*, the batch forms included: the Adler-32 trailer behind the stream must be there and match

GEN_KINDS = {"xorshift": 0, "lowent4k": 1, "itext": 2}


class ZlibEsError(Exception):
    """Mirror of the reference's ``throw new Error(message)``; ``.code`` is the zes_status."""

    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


class ZesKTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_float), ("launches", C.c_uint32)]


# zes_zip_entry of include/zes.h: one record of a ZIP archive's index
ZIP_ENTRY = np.dtype([("hdr_off", "<u8"), ("name_pos", "<u8"), ("csize", "<u4"), ("usize", "<u4"), ("crc", "<u4"), ("name_off", "<u4"),
                      ("name_len", "<u2"), ("method", "<u2"), ("flags", "<u2"), ("pad", "<u2")])
assert ZIP_ENTRY.itemsize == 40

# zes_png_info of include/zes.h: what the PNG reader says about one file
PNG_INFO = np.dtype([("width", "<u4"), ("height", "<u4"), ("depth", "u1"), ("colour", "u1"), ("interlace", "u1"), ("channels", "u1"), ("bpp", "u1"),
                     ("pad", "u1", (3,)), ("rowbytes", "<u8"), ("out_size", "<u8"), ("idat_count", "<u4"), ("plte_len", "<u4"), ("idat_bytes", "<u8"),
                     ("plte_pos", "<u8"), ("trns_pos", "<u8"), ("trns_len", "<u4"), ("pad2", "<u4")])
assert PNG_INFO.itemsize == 72

# zes_pngw_image of include/zes.h: what the PNG writer is told about one image
PNGW_IMAGE = np.dtype([("width", "<u4"), ("height", "<u4"), ("depth", "u1"), ("colour", "u1"), ("filter", "u1"), ("pad", "u1"), ("plte_len", "<u2"),
                       ("trns_len", "<u2")])
assert PNGW_IMAGE.itemsize == 16
PNG_FILTER_BANDED = 5  # adaptive, rows 0, 64, 128, ... None or Sub: the reader's bands then decode in parallel
PNG_FILTER_ADAPTIVE = 6

# zes_tiff_image of include/zes.h: what the TIFF reader says about one image of a file
TIFF_IMAGE = np.dtype([("width", "<u4"), ("height", "<u4"), ("seg_w", "<u4"), ("seg_h", "<u4"), ("across", "<u4"), ("down", "<u4"), ("bits", "<u2"),
                       ("spp", "<u2"), ("compression", "<u2"), ("predictor", "<u2"), ("photometric", "<u2"), ("sample_format", "<u2"),
                       ("extra_samples", "<u2"), ("big_endian", "u1"), ("tiled", "u1"), ("out_size", "<u8")])
assert TIFF_IMAGE.itemsize == 48

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64)  # zes_alloc_fn of include/zes.h


def build(force=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcdir = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-s", "-C", srcdir, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", srcdir])
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                "zlib.es_amd: %s is missing — run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % _LIB_PATH)
        L = C.CDLL(_LIB_PATH)
        u64p, u32p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        L.zes_strerror.restype = C.c_char_p
        L.zes_strerror.argtypes = [C.c_int]
        L.zes_init.argtypes = [C.c_int]
        L.zes_init_devices.argtypes = [C.c_int]
        L.zes_partition.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        L.zes_device_info.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), u64p]
        L.zes_deflate_bound.argtypes = [C.c_uint64, u64p]
        for name in ("zes_deflate", "zes_deflate_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]
        for name in ("zes_inflate", "zes_inflate_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.c_uint32]
        L.zes_inflate_size.argtypes = [C.c_void_p, C.c_uint64, u64p, C.c_uint32]
        L.zes_inflate_alloc.argtypes = [C.c_void_p, C.c_uint64, ALLOC_FN, C.c_void_p, u64p, C.c_uint32]
        L.zes_deflate_batch.argtypes = [C.POINTER(C.c_void_p), u64p, C.POINTER(C.c_void_p), u64p, u64p, i32p, C.c_uint32]
        L.zes_inflate_batch_alloc.argtypes = [C.POINTER(C.c_void_p), u64p, ALLOC_FN, C.c_void_p, u64p, i32p, C.c_uint32, C.c_uint32]
        L.zes_host_alloc.argtypes = [C.c_uint64, C.POINTER(C.c_void_p)]
        L.zes_host_free.argtypes = [C.c_void_p]
        for name in ("zes_deflate_raw", "zes_deflate_raw_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]
        for name in ("zes_inflate_raw", "zes_inflate_raw_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.c_uint32]
        for name in ("zes_inflate_raw_used", "zes_inflate_raw_used_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, u64p, u64p, C.c_uint32]
        for name in ("zes_crc32", "zes_crc32_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, u32p]
        L.zes_crc32_batch_dev.argtypes = [C.c_void_p, u64p, u64p, u32p, C.c_uint32]
        L.zes_last_gunzip_members.argtypes = []
        L.zes_gzip_bound.argtypes = [C.c_uint64, u64p]
        for name in ("zes_gzip", "zes_gzip_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p]
        for name in ("zes_gunzip", "zes_gunzip_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.c_uint32]
        for name in ("zes_bgzip_members", "zes_bgzip_bound"):
            getattr(L, name).argtypes = [C.c_uint64, u64p]
        for name in ("zes_bgzip", "zes_bgzip_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, u64p, C.c_uint32]
        for name in ("zes_bgzf_index", "zes_bgzf_index_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_uint32]
        for name in ("zes_bgzf_read", "zes_bgzf_read_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                         u64p, C.c_uint32]
        for name in ("zes_zip_index", "zes_zip_index_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p, C.c_uint32]
        L.zes_zip_read_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_uint32]
        L.zes_zip_read_alloc.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, ALLOC_FN, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint32]
        L.zes_zipwrite_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, u64p]
        L.zes_zipwrite_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, u64p, C.c_void_p,
                                       C.c_uint32]
        L.zes_zipwrite.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint32]
        L.zes_png_info_get.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
        L.zes_png_decode_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint32]
        L.zes_png_decode_alloc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, ALLOC_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.zes_pngwrite_bound.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.zes_pngwrite_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_uint32]
        L.zes_pngwrite.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, ALLOC_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.zes_pngpix_dev.argtypes = L.zes_png_decode_dev.argtypes
        L.zes_pngpix_alloc.argtypes = L.zes_png_decode_alloc.argtypes
        L.zes_pngpix_expand_dev.argtypes = L.zes_pngwrite_dev.argtypes
        for name in ("zes_tiff_index", "zes_tiff_index_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p, u32p, C.c_uint32]
        L.zes_tiff_read_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_void_p,
                                        C.c_uint32]
        L.zes_tiff_read_alloc.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, ALLOC_FN, C.c_void_p, u64p, C.c_void_p, C.c_uint32]
        L.zes_last_tiff_read.argtypes = [u32p, C.c_void_p]
        L.zes_tiffwrite_bound.argtypes = [C.c_void_p, u64p, u64p]
        L.zes_tiffwrite_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.zes_tiffwrite.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, ALLOC_FN, C.c_void_p, u64p, C.c_uint32]
        L.zes_gunzip_alloc.argtypes = [C.c_void_p, C.c_uint64, ALLOC_FN, C.c_void_p, u64p, C.c_uint32]
        L.zes_gzip_batch_bound.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        for name in ("zes_gzip_batch_dev", "zes_gunzip_batch_dev"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint32]
        for name in ("zes_gzip_batch", "zes_gunzip_batch_alloc"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, ALLOC_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.zes_last_gunzip_batch.argtypes = [u32p, u32p]
        L.zes_adler32.argtypes = [C.c_void_p, C.c_uint64, u32p]
        L.zes_adler32_dev.argtypes = [C.c_void_p, C.c_uint64, u32p]
        L.zes_adler32_batch_dev.argtypes = [C.c_void_p, u64p, u64p, u32p, C.c_uint32]
        L.zes_deflate_batch_dev.argtypes = [C.c_void_p, u64p, u64p, C.c_void_p, u64p, u64p, u64p, i32p, C.c_uint32]
        L.zes_inflate_batch_dev.argtypes = [C.c_void_p, u64p, u64p, C.c_void_p, u64p, u64p, u64p, i32p, C.c_uint32,
                                            C.c_uint32]
        L.zes_deflate_range_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, u64p, u32p]
        L.zes_inflate_range_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, u64p, u64p, u64p,
                                            u32p, i32p]
        L.zes_deflate_join_dev.argtypes = [C.POINTER(C.c_void_p), u64p, u32p, u64p, C.c_uint32, C.c_void_p, C.c_uint64, u64p]
        L.zes_stage_lz77_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, u32p]
        L.zes_stage_lz77_route.argtypes = [C.c_void_p, C.c_uint32]
        L.zes_stage_huff_lengths_dev.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.zes_stage_chain.argtypes = [u32p, u64p, u32p, u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, i32p, u64p, u32p, u32p]
        L.zes_stage_poison.argtypes = [C.c_uint32, u64p]
        L.zes_selftest_lds_order.argtypes = [C.c_uint32, C.c_uint32, u64p, u64p]
        L.zes_last_kernel_times.argtypes = [C.POINTER(ZesKTime), C.c_int]
        L.zes_set_profiling.argtypes = [C.c_int]
        L.zes_pool_bytes.restype = C.c_uint64
        L.zes_pool_bytes.argtypes = []
        L.zes_gen.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
        _lib = L
    return _lib


def strerror(code):
    return lib().zes_strerror(code).decode()


def _raise(code):
    raise ZlibEsError(code, strerror(code))


def _raise_need(rc, n):
    """A device form's status: ZES_E_NOSPACE carries the size the result needs (``.need``, from the call's out_len ``n``)."""
    if rc == ZES_E_NOSPACE:
        err = ZlibEsError(rc, "%s (need %d bytes)" % (strerror(rc), n.value))
        err.need = n.value
        raise err
    if rc:
        _raise(rc)


def init(device=0):
    rc = lib().zes_init(int(device))
    if rc:
        _raise(rc)


def trim():
    """zes_trim: the pooled device scratch of every context goes back to the driver (the next call allocates again)."""
    rc = lib().zes_trim()
    if rc:
        _raise(rc)


def pool_bytes():
    """zes_pool_bytes: pooled device scratch held right now, all contexts."""
    return int(lib().zes_pool_bytes())


def init_devices(n=0):
    """One process, n GPUs (n <= 0: every visible one): the host batch forms then spread over all of them
    (zes_init_devices).  Returns the number of devices in use."""
    rc = lib().zes_init_devices(int(n))
    if rc:
        _raise(rc)
    return int(lib().zes_device_count())


def partition(sizes, parts):
    """owner[i] of buffer i among `parts` devices: the library's rule for host batches (zes_partition; no GPU needed)."""
    n = len(sizes)
    arr = (C.c_uint64 * max(n, 1))(*[int(x) for x in sizes])
    own = (C.c_uint32 * max(n, 1))()
    rc = lib().zes_partition(arr, n, int(parts), own)
    if rc:
        _raise(rc)
    return [int(own[i]) for i in range(n)]


def device_info():
    name = C.create_string_buffer(64)
    cus = C.c_int()
    hbm = C.c_uint64()
    rc = lib().zes_device_info(name, 64, C.byref(cus), C.byref(hbm))
    if rc:
        _raise(rc)
    return {"arch": name.value.decode(), "cus": cus.value, "hbm_bytes": hbm.value}


def gen(kind, seed, n):
    """Deterministic workload bytes (xorshift / lowent4k / itext), as a numpy uint8 array."""
    out = np.empty(n, dtype=np.uint8)
    rc = lib().zes_gen(out.ctypes.data, n, GEN_KINDS[kind] if isinstance(kind, str) else int(kind), int(seed) & 0xFFFFFFFF)
    if rc:
        _raise(rc)
    return out


def _as_u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def deflate_bound(n):
    cap = C.c_uint64()
    lib().zes_deflate_bound(n, C.byref(cap))
    return cap.value


# ---- host-buffer API: the drop-in pair ------------------------------------------------------
def deflate(data):
    """``deflate(input)`` of src/zlib.ts:25 — zlib-wrapped, bit-exact; returns a fresh uint8 array."""
    a = _as_u8(data)
    cap = deflate_bound(a.size)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_uint64()
    rc = lib().zes_deflate(a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc)
    return out[: n.value].copy() if n.value < (1 << 20) else out[: n.value]  # large results: a view, not a second copy


def inflate(data, flags=0):
    """``inflate(input)`` of src/zlib.ts:11 — same accept-set and errors as the reference.

    One library call: it decodes on the device, then asks (callback) for the exact-size result array and copies
    into it — the growable Uint8WriteStream of src/inflate.ts:17 without a second decode or hidden state.
    """
    a = _as_u8(data)
    got = []

    def alloc(_user, _index, n):
        got.append(np.empty(max(int(n), 1), dtype=np.uint8))
        return got[0].ctypes.data

    n = C.c_uint64()
    rc = lib().zes_inflate_alloc(a.ctypes.data, a.size, ALLOC_FN(alloc), None, C.byref(n), flags)
    if rc:
        _raise(rc)
    return got[0][: n.value]


def _ptr_array(arrs):
    return (C.c_void_p * len(arrs))(*[x.ctypes.data for x in arrs])


def deflate_batch(buffers):
    """Host-pointer batch: a list of independent buffers in one call → list of uint8 arrays or ZlibEsError (not raised)."""
    arrs = [_as_u8(b) for b in buffers]
    cnt = len(arrs)
    outs = [np.empty(deflate_bound(x.size), dtype=np.uint8) for x in arrs]
    lens = (C.c_uint64 * cnt)(*[x.size for x in arrs])
    caps = (C.c_uint64 * cnt)(*[o.size for o in outs])
    out_len = (C.c_uint64 * cnt)()
    status = (C.c_int32 * cnt)()
    rc = lib().zes_deflate_batch(_ptr_array(arrs), lens, _ptr_array(outs), caps, out_len, status, cnt)
    if rc:
        _raise(rc)
    return [outs[i][: out_len[i]].copy() if status[i] == 0 else ZlibEsError(status[i], strerror(status[i])) for i in range(cnt)]


def inflate_batch(buffers, flags=0):
    """Inflate independent zlib streams in one call (zes_inflate_batch_alloc); returns one uint8 array or one ZlibEsError
    per buffer.  With ZES_F_CHECK_ADLER in ``flags`` every stream's Adler-32 trailer must be there and match its result:
    a buffer that fails is a ZlibEsError(ZES_E_CHECKSUM) and no memory is asked for it."""
    arrs = [_as_u8(b) for b in buffers]
    cnt = len(arrs)
    got = {}

    def alloc(_user, index, n):
        got[index] = np.empty(max(int(n), 1), dtype=np.uint8)
        return got[index].ctypes.data

    lens = (C.c_uint64 * cnt)(*[x.size for x in arrs])
    out_len = (C.c_uint64 * cnt)()
    status = (C.c_int32 * cnt)()
    rc = lib().zes_inflate_batch_alloc(_ptr_array(arrs), lens, ALLOC_FN(alloc), None, out_len, status, cnt, flags)
    if rc:
        _raise(rc)
    return [got[i][: out_len[i]] if status[i] == 0 else ZlibEsError(status[i], strerror(status[i])) for i in range(cnt)]


def host_alloc(n):
    """A uint8 numpy array of n bytes in page-locked memory (zes_host_alloc); free with host_free(arr)."""
    p = C.c_void_p()
    rc = lib().zes_host_alloc(n, C.byref(p))
    if rc:
        _raise(rc)
    arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(n, 1),))[:n]
    return arr


def host_free(arr):
    rc = lib().zes_host_free(arr.ctypes.data)
    if rc:
        _raise(rc)


def deflate_raw(data):
    """Raw DEFLATE: ``deflate(input)`` of src/deflate.ts:14 (what the zlib wrapper of src/zlib.ts:25 encloses)."""
    a = _as_u8(data)
    cap = deflate_bound(a.size)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_uint64()
    rc = lib().zes_deflate_raw(a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc)
    return out[: n.value].copy()


def inflate_raw(data, offset=0, flags=0):
    """Raw inflate from byte ``offset``: ``inflate(input, offset)`` of src/inflate.ts:16."""
    a = _as_u8(data)
    cap = max(a.size * 8, 1 << 16)
    for _ in range(8):
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_uint64()
        rc = lib().zes_inflate_raw(a.ctypes.data, a.size, offset, out.ctypes.data, cap, C.byref(n), flags)
        if rc == ZES_E_NOSPACE and n.value > cap:
            cap = n.value
            continue
        if rc:
            _raise(rc)
        return out[: n.value].copy()
    _raise(ZES_E_DEVICE)


def inflate_raw_used(data, offset=0, flags=0):
    """Raw inflate from byte ``offset`` that also says where the stream ended: ``(out, used)``, ``used`` = bytes from
    ``offset`` up to and including the one that holds the final block's last bit (zes_inflate_raw_used)."""
    a = _as_u8(data)
    cap = max(a.size * 8, 1 << 16)
    for _ in range(8):
        out = np.empty(cap, dtype=np.uint8)
        n, used = C.c_uint64(), C.c_uint64()
        rc = lib().zes_inflate_raw_used(a.ctypes.data, a.size, offset, out.ctypes.data, cap, C.byref(n), C.byref(used), flags)
        if rc == ZES_E_NOSPACE and n.value > cap:
            cap = n.value
            continue
        if rc:
            _raise(rc)
        return out[: n.value].copy(), used.value
    _raise(ZES_E_DEVICE)


def crc32(data):
    """CRC-32 of gzip / zlib.crc32 (zes_crc32)."""
    a = _as_u8(data)
    out = C.c_uint32()
    rc = lib().zes_crc32(a.ctypes.data, a.size, C.byref(out))
    if rc:
        _raise(rc)
    return out.value


def gzip_bound(n):
    cap = C.c_uint64()
    lib().zes_gzip_bound(n, C.byref(cap))
    return cap.value


def gzip(data):
    """One gzip member: fixed 10-byte header, deflate_raw(data) as the body, CRC-32 and size (zes_gzip)."""
    a = _as_u8(data)
    cap = gzip_bound(a.size)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_uint64()
    rc = lib().zes_gzip(a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc)
    return out[: n.value].copy()


def bgzip_members(n):
    """Members of bgzip() of n bytes: one per 65280-byte chunk and the end-of-file marker (zes_bgzip_members; no GPU needed)."""
    m = C.c_uint64()
    rc = lib().zes_bgzip_members(n, C.byref(m))
    if rc:
        _raise(rc)
    return m.value


def bgzip_bound(n):
    """A capacity that always suffices for bgzip() of n bytes, exact for incompressible input (zes_bgzip_bound; no GPU needed)."""
    cap = C.c_uint64()
    rc = lib().zes_bgzip_bound(n, C.byref(cap))
    if rc:
        _raise(rc)
    return cap.value


def bgzip(data, flags=0, index=False):
    """A BGZF file (bgzip / htslib): a gzip member per 65280-byte chunk and the end-of-file marker (zes_bgzip).
    index=True: ``(bytes, offsets)``, ``offsets[k]`` the position of member k in the result, the marker's last."""
    a = _as_u8(data)
    cap = bgzip_bound(a.size)
    out = np.empty(cap, dtype=np.uint8)
    off = (C.c_uint64 * bgzip_members(a.size))()
    n = C.c_uint64()
    rc = lib().zes_bgzip(a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n), off, flags)
    if rc:
        _raise(rc)
    res = out[: n.value].copy()
    return (res, list(off)) if index else res


def _bgzf_index_call(fn, ptr, c, flags):
    """(coff, uoff) of a BGZF file through zes_bgzf_index / zes_bgzf_index_dev: the count first, then the arrays."""
    m = C.c_uint64()
    rc = fn(ptr, c, None, None, 0, C.byref(m), flags)
    if rc != ZES_E_NOSPACE:
        _raise(rc if rc else ZES_E_ARG)
    coff = np.empty(m.value + 1, dtype=np.uint64)
    uoff = np.empty(m.value + 1, dtype=np.uint64)
    rc = fn(ptr, c, coff.ctypes.data, uoff.ctypes.data, coff.size, C.byref(m), flags)
    if rc:
        _raise(rc)
    return coff, uoff


def _bgzf_index_arrays(index):
    coff = np.ascontiguousarray(index[0], dtype=np.uint64)
    uoff = np.ascontiguousarray(index[1], dtype=np.uint64)
    assert coff.ndim == 1 and coff.size == uoff.size and coff.size >= 1, "a BGZF index is (coff, uoff): two arrays of members + 1 entries"
    return coff, uoff


def bgzf_index(data):
    """The member index of a BGZF file (zes_bgzf_index; no GPU needed): ``(coff, uoff)``, numpy uint64 arrays of
    members + 1 entries — member k starts at byte ``coff[k]`` and its output at byte ``uoff[k]`` of the uncompressed data;
    the closing entries are the file's length and the uncompressed size."""
    a = _as_u8(data)
    return _bgzf_index_call(lib().zes_bgzf_index, a.ctypes.data, a.size, 0)


def bgzf_read(data, index, pos, length):
    """Bytes ``[pos, pos + length)`` of the uncompressed data of a BGZF file, clipped at its end, through ``index`` =
    ``bgzf_index(data)``: only the members that hold the range are uploaded and decoded (zes_bgzf_read)."""
    a = _as_u8(data)
    coff, uoff = _bgzf_index_arrays(index)
    total = int(uoff[-1])
    cap = max(min(int(length), max(total - int(pos), 0)), 0)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    n = C.c_uint64()
    rc = lib().zes_bgzf_read(a.ctypes.data, a.size, coff.ctypes.data, uoff.ctypes.data, coff.size - 1, pos, length, out.ctypes.data, cap, C.byref(n), 0)
    if rc:
        _raise(rc)
    return out[: n.value]


def _zip_index_call(fn, ptr, c):
    """(entries, names) of a ZIP archive through zes_zip_index / zes_zip_index_dev: the counts first, then the arrays."""
    n, nl = C.c_uint64(), C.c_uint64()
    rc = fn(ptr, c, None, 0, C.byref(n), None, 0, C.byref(nl), 0)
    if rc != ZES_E_NOSPACE:
        _raise(rc if rc else ZES_E_ARG)
    ent = np.zeros(n.value, dtype=ZIP_ENTRY)
    blob = np.zeros(max(nl.value, 1), dtype=np.uint8)
    if n.value:
        rc = fn(ptr, c, ent.ctypes.data, ent.size, C.byref(n), blob.ctypes.data, nl.value, C.byref(nl), 0)
        if rc:
            _raise(rc)
    raw = blob.tobytes()
    return ent, [raw[int(e["name_off"]) : int(e["name_off"]) + int(e["name_len"])] for e in ent]


def _zip_entries(index):
    ent = index[0] if isinstance(index, tuple) else index
    ent = np.ascontiguousarray(ent, dtype=ZIP_ENTRY)
    assert ent.ndim == 1, "a ZIP index is the structured array zip_index() returns (or its (entries, names) pair)"
    return ent


def _zip_sel(ent, sel):
    if sel is None:
        return None, ent.size
    s = np.ascontiguousarray(sel, dtype=np.uint32)
    assert s.ndim == 1
    return s, s.size


def zip_index(data):
    """The entries of a ZIP archive in directory order (zes_zip_index; no GPU needed): ``(entries, names)``, a numpy
    structured array with zes_zip_entry's layout (ZIP_ENTRY) and the names as a list of ``bytes``.  Nothing is decoded and
    no local header is looked at; ZlibEsError(ZES_E_ZIP / ZES_E_UNSUPPORTED) for what the reader does not accept."""
    a = _as_u8(data)
    return _zip_index_call(lib().zes_zip_index, a.ctypes.data if a.size else None, a.size)


def zip_read(data, index, sel=None):
    """Entries ``sel`` (all when None; any order, duplicates fine) of a ZIP archive extracted as one batch through
    ``index`` = ``zip_index(data)`` (zes_zip_read_alloc): a list with one uint8 array or one ZlibEsError per entry (not
    raised, as with inflate_batch).  Only the selected entries' bytes are uploaded."""
    a = _as_u8(data)
    ent = _zip_entries(index)
    s, cnt = _zip_sel(ent, sel)
    got = {}

    def alloc(_user, i, n):
        got[i] = np.empty(max(int(n), 1), dtype=np.uint8)
        return got[i].ctypes.data

    out_len = (C.c_uint64 * max(cnt, 1))()
    status = (C.c_int32 * max(cnt, 1))()
    rc = lib().zes_zip_read_alloc(a.ctypes.data if a.size else None, a.size, ent.ctypes.data if ent.size else None, ent.size,
                                  s.ctypes.data if s is not None and cnt else None, cnt, ALLOC_FN(alloc), None, out_len, status, 0)
    if rc:
        _raise(rc)
    return [got[i][: out_len[i]] if status[i] == 0 else ZlibEsError(status[i], strerror(status[i])) for i in range(cnt)]


def _ptr(a):
    return a.ctypes.data if a.size else None


def _zip_names(names):
    """(blob, name_len) of a list of ``bytes``: the names back to back and their lengths."""
    names = [bytes(n) for n in names]
    assert all(len(n) <= 65535 for n in names), "a ZIP entry's name has at most 65535 bytes"
    return np.frombuffer(b"".join(names), dtype=np.uint8), np.array([len(n) for n in names], dtype=np.uint16)


def zip_bound(lens, name_lens):
    """A capacity that always suffices for the archive of entries of ``lens`` bytes under names of ``name_lens`` bytes, exact
    when every entry is stored (zes_zipwrite_bound; no GPU needed)."""
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    nl = np.ascontiguousarray(name_lens, dtype=np.uint16)
    assert ln.ndim == 1 and ln.shape == nl.shape
    cap = C.c_uint64()
    rc = lib().zes_zipwrite_bound(_ptr(ln), _ptr(nl), ln.size, C.byref(cap))
    if rc:
        _raise(rc)
    return cap.value


def zip_write(entries, flags=0):
    """A ZIP archive of ``entries``, a list of ``(name: bytes, data)``: ``(archive, index)``, the archive as a uint8 array and
    ``index`` as zip_index() returns it (zes_zipwrite).  An entry is deflated when that is shorter, else stored; the same
    entries give the same bytes (date 1980-01-01)."""
    datas = [_as_u8(d) for _, d in entries]
    blob, nl = _zip_names([n for n, _ in entries])
    cnt = len(datas)
    ln = np.array([d.size for d in datas], dtype=np.uint64)
    cap = zip_bound(ln, nl)
    out = np.empty(cap, dtype=np.uint8)
    ent = np.zeros(cnt, dtype=ZIP_ENTRY)
    ptrs = (C.c_void_p * max(cnt, 1))(*[d.ctypes.data if d.size else None for d in datas])
    n = C.c_uint64()
    rc = lib().zes_zipwrite(ptrs, _ptr(ln), _ptr(blob), _ptr(nl), cnt, out.ctypes.data, cap, C.byref(n), _ptr(ent), flags)
    if rc:
        _raise(rc)
    raw = blob.tobytes()
    return out[: n.value].copy(), (ent, [raw[int(e["name_off"]) : int(e["name_off"]) + int(e["name_len"])] for e in ent])


def png_info(data):
    """What the PNG reader says about a file (zes_png_info_get; no GPU needed): one PNG_INFO record — size, bit depth, colour
    type, interlace method, the filter unit ``bpp``, ``rowbytes``, ``out_size`` and where the IDAT, PLTE and tRNS data lie.
    ZlibEsError(ZES_E_PNG / ZES_E_UNSUPPORTED) for a file the reader does not accept; no CRC is checked here."""
    a = _as_u8(data)
    info = np.zeros(1, dtype=PNG_INFO)
    rc = lib().zes_png_info_get(a.ctypes.data if a.size else None, a.size, info.ctypes.data, 0)
    if rc:
        _raise(rc)
    return info[0]


def _png_batch(pix, buffers, flags):
    """png_decode_batch (zes_png_decode_alloc) and, with ``pix``, png_pixels_batch (zes_pngpix_alloc): one call, the results
    shaped per image."""
    arrs = [_as_u8(b) for b in buffers]
    cnt = len(arrs)
    got = {}

    def alloc(_user, i, n):
        got[i] = np.empty(max(int(n), 1), dtype=np.uint8)
        return got[i].ctypes.data

    ptrs = (C.c_void_p * max(cnt, 1))(*[a.ctypes.data if a.size else None for a in arrs])
    ln = np.array([a.size for a in arrs], dtype=np.uint64)
    out_len = np.zeros(max(cnt, 1), dtype=np.uint64)
    status = np.zeros(max(cnt, 1), dtype=np.int32)
    info = np.zeros(max(cnt, 1), dtype=PNG_INFO)
    fn = lib().zes_pngpix_alloc if pix else lib().zes_png_decode_alloc
    rc = fn(ptrs, _ptr(ln), cnt, ALLOC_FN(alloc), None, out_len.ctypes.data, status.ctypes.data, info.ctypes.data, flags)
    if rc:
        _raise(rc)
    shape = lambda r: (int(r["height"]), int(r["width"]), 4) if pix else (int(r["height"]), int(r["rowbytes"]))
    return [(info[i], got[i][: int(out_len[i])].reshape(shape(info[i]))) if status[i] == 0
            else ZlibEsError(int(status[i]), strerror(int(status[i]))) for i in range(cnt)]


def png_decode_batch(buffers, flags=0):
    """PNG files decoded as one batch (zes_png_decode_alloc): a list with one ``(info, scanlines)`` pair or one ZlibEsError
    per file (not raised, as with zip_read).  ``scanlines`` is a uint8 array of ``height`` x ``rowbytes``: the samples as the
    file stores them (16-bit big-endian, sub-byte samples packed, palette indices), the filters undone.  An Adam7-interlaced
    file is ZlibEsError(ZES_E_UNSUPPORTED) unless ``flags`` has ZES_F_PNG_INTERLACED; with it, its scanlines are those of a
    non-interlaced file of the same pixels."""
    return _png_batch(False, buffers, flags)


def png_decode(data, flags=0):
    """One PNG file decoded: ``(info, scanlines)`` as png_decode_batch gives them; a file that fails raises.  ``flags``:
    ZES_F_PNG_INTERLACED to take an Adam7-interlaced file."""
    got = png_decode_batch([data], flags)[0]
    if isinstance(got, Exception):
        raise got
    return got


def png_pixels_batch(buffers, flags=0):
    """PNG files decoded to pixels as one batch (zes_pngpix_alloc): a list with one ``(info, rgba)`` pair or one ZlibEsError
    per file (not raised, as with png_decode_batch).  ``rgba`` is a uint8 array of ``height`` x ``width`` x 4: R, G, B, A by
    the conversion rule of include/zes.h (sub-byte samples scaled, 16-bit samples cut to their high byte, the palette looked
    up, tRNS applied).  ``flags``: ZES_F_PNG_INTERLACED to take Adam7-interlaced files too, as png_decode_batch does."""
    return _png_batch(True, buffers, flags)


def png_pixels(data, flags=0):
    """One PNG file decoded to pixels: ``(info, rgba)`` as png_pixels_batch gives them; a file that fails raises.  ``flags``:
    ZES_F_PNG_INTERLACED to take an Adam7-interlaced file."""
    got = png_pixels_batch([data], flags)[0]
    if isinstance(got, Exception):
        raise got
    return got


def png_bound(images):
    """A capacity per image that always suffices for its PNG file, exact when its zlib stream goes stored, and 0 for a record
    the writer rejects (zes_pngwrite_bound; no GPU needed).  ``images``: a PNGW_IMAGE array."""
    img = np.ascontiguousarray(images, dtype=PNGW_IMAGE).reshape(-1)
    cap = np.zeros(max(img.size, 1), dtype=np.uint64)
    rc = lib().zes_pngwrite_bound(_ptr(img), img.size, cap.ctypes.data)
    if rc:
        _raise(rc)
    return [int(x) for x in cap[: img.size]]


def _png_item(rows, width=None, colour=None, depth=8, filter=PNG_FILTER_BANDED, palette=b"", trns=b""):
    """(scanlines, PNGW_IMAGE fields, aux bytes) of one png_encode() argument list."""
    a = rows if isinstance(rows, np.ndarray) else np.asarray(rows)
    assert a.dtype == np.uint8 and a.ndim in (2, 3), "png_encode: rows is a uint8 array, height x rowbytes or height x width x channels"
    height = a.shape[0]
    if colour is None:
        colour = {1: 0, 2: 4, 3: 2, 4: 6}[a.shape[2]] if a.ndim == 3 else (3 if len(palette) else 0)
    channels = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}.get(colour, 1)
    flat = np.ascontiguousarray(a).reshape(height, -1)
    if width is None:
        assert depth >= 8, "png_encode: `width` is needed below 8 bits a sample"
        width = flat.shape[1] // (channels * depth // 8)
    palette, trns = bytes(palette), bytes(trns)
    assert len(palette) <= 65535 and len(trns) <= 65535
    return flat.reshape(-1), (width, height, depth, colour, filter, 0, len(palette), len(trns)), palette + trns


def png_encode_batch(items, flags=0):
    """Images written as PNG files in one batch (zes_pngwrite): ``items`` is a list of dicts of png_encode()'s arguments; the
    result has one uint8 array (the file) or one ZlibEsError per image (not raised, as with png_decode_batch)."""
    parts = [_png_item(**it) for it in items]
    cnt = len(parts)
    img = np.zeros(max(cnt, 1), dtype=PNGW_IMAGE)
    for i, (_, rec, _) in enumerate(parts):
        img[i] = rec
    aux = np.frombuffer(b"".join(x for _, _, x in parts), dtype=np.uint8)
    got = {}

    def alloc(_user, i, n):
        got[i] = np.empty(max(int(n), 1), dtype=np.uint8)
        return got[i].ctypes.data

    ptrs = (C.c_void_p * max(cnt, 1))(*[d.ctypes.data if d.size else None for d, _, _ in parts])
    ln = np.array([d.size for d, _, _ in parts], dtype=np.uint64)
    out_len = np.zeros(max(cnt, 1), dtype=np.uint64)
    status = np.zeros(max(cnt, 1), dtype=np.int32)
    rc = lib().zes_pngwrite(ptrs, _ptr(ln), img.ctypes.data, _ptr(aux), cnt, ALLOC_FN(alloc), None, out_len.ctypes.data, status.ctypes.data, flags)
    if rc:
        _raise(rc)
    return [got[i][: int(out_len[i])] if status[i] == 0 else ZlibEsError(int(status[i]), strerror(int(status[i]))) for i in range(cnt)]


def png_encode(rows, width=None, colour=None, depth=8, filter=PNG_FILTER_BANDED, palette=b"", trns=b"", flags=0):
    """One image as a PNG file (a uint8 array).  ``rows``: the scanlines as png_decode gives them, a uint8 array of ``height`` x
    ``rowbytes`` (or height x width x channels of 8-bit samples: the colour type then follows from the channels); ``width`` is
    needed below 8 bits a sample.  ``colour`` and ``depth`` as in IHDR; ``filter``: 0..4 that type on every row, 6 libpng's
    adaptive choice, 5 (the default) the same with rows 0, 64, 128, ... None or Sub, which lets png_decode work on the file's
    bands of 64 rows in parallel.  ``palette`` / ``trns``: the data of PLTE / tRNS.  An image that fails raises."""
    got = png_encode_batch([dict(rows=rows, width=width, colour=colour, depth=depth, filter=filter, palette=palette, trns=trns)], flags)[0]
    if isinstance(got, Exception):
        raise got
    return got


def gunzip(data, flags=0):
    """gzip.decompress: every member, their outputs concatenated (zes_gunzip_alloc: one decode, an exact-size result)."""
    a = _as_u8(data)
    got = []

    def alloc(_user, _index, n):
        got.append(np.empty(max(int(n), 1), dtype=np.uint8))
        return got[0].ctypes.data

    n = C.c_uint64()
    rc = lib().zes_gunzip_alloc(a.ctypes.data, a.size, ALLOC_FN(alloc), None, C.byref(n), flags)
    if rc:
        _raise(rc)
    return got[0][: n.value]


def gzip_batch_bound(lens):
    """zes_gzip_batch_bound: the room that file i of gzip_batch_tensor needs at most, ``18 + n + 5 * max(1, ceil(n / 65535))``."""
    ln = np.ascontiguousarray(lens, dtype=np.uint64).reshape(-1)
    cap = np.zeros(max(ln.size, 1), dtype=np.uint64)
    rc = lib().zes_gzip_batch_bound(_ptr(ln), ln.size, cap.ctypes.data)
    if rc:
        _raise(rc)
    return [int(x) for x in cap[: ln.size]]


def _host_batch(fn, buffers, flags):
    """zes_gzip_batch / zes_gunzip_batch_alloc over a list of buffers: one uint8 array or one ZlibEsError (not raised) per buffer."""
    arrs = [_as_u8(b) for b in buffers]
    cnt = len(arrs)
    got = {}

    def alloc(_user, i, n):
        got[i] = np.empty(max(int(n), 1), dtype=np.uint8)
        return got[i].ctypes.data

    ptrs = (C.c_void_p * max(cnt, 1))(*[a.ctypes.data if a.size else None for a in arrs])
    ln = np.array([a.size for a in arrs], dtype=np.uint64)
    out_len = np.zeros(max(cnt, 1), dtype=np.uint64)
    status = np.zeros(max(cnt, 1), dtype=np.int32)
    rc = fn(ptrs, _ptr(ln), cnt, ALLOC_FN(alloc), None, out_len.ctypes.data, status.ctypes.data, flags)
    if rc:
        _raise(rc)
    return [got[i][: int(out_len[i])] if status[i] == 0 else ZlibEsError(int(status[i]), strerror(int(status[i]))) for i in range(cnt)]


def gzip_batch(buffers, flags=0):
    """Independent buffers written as one gzip file each in one batch (zes_gzip_batch): the result has one uint8 array (the
    file: gzip()'s bytes, or the stored form where that is shorter or the encoder refuses the length) or one ZlibEsError per
    buffer (not raised).  ``flags``: ZES_F_PIECES for groups of four (same bytes)."""
    return _host_batch(lib().zes_gzip_batch, buffers, flags)


def gunzip_batch(buffers, flags=0):
    """Independent gzip files decoded in one batch (zes_gunzip_batch_alloc): per file what gunzip() gives for it alone, a uint8
    array or the ZlibEsError (not raised).  ``flags``: ZES_F_PIECES, ZES_F_GZIP_SERIAL (every file on the per-file route)."""
    return _host_batch(lib().zes_gunzip_batch_alloc, buffers, flags)


def last_gunzip_batch():
    """``(batched, serial)``: the files of the last gunzip batch call that finished as one batch and on the per-file route."""
    a, b = C.c_uint32(), C.c_uint32()
    lib().zes_last_gunzip_batch(C.byref(a), C.byref(b))
    return a.value, b.value


def adler32(data):
    a = _as_u8(data)
    out = C.c_uint32()
    rc = lib().zes_adler32(a.ctypes.data, a.size, C.byref(out))
    if rc:
        _raise(rc)
    return out.value


# ---- HBM-resident API (torch uint8 CUDA tensors; torch is plumbing for device memory) --------
def _aligned(t):
    """The inflate and range device forms need a 16-byte aligned input (include/zes.h); a sliced view such as t[3:] is
    copied once."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def deflate_tensor(t, out=None):
    """Compress a 1-D uint8 CUDA tensor, which may start at any byte (zes_deflate_dev reads an input at any alignment);
    returns a view of ``out`` (allocated if None)."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    cap = deflate_bound(t.numel())
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=t.device)
    assert out.numel() >= cap
    assert out.data_ptr() % 16 == 0, "deflate_tensor: `out` must start on a 16-byte boundary (include/zes.h: device forms)"
    torch.cuda.current_stream(t.device).synchronize()  # the library runs on its own stream
    n = C.c_uint64()
    rc = lib().zes_deflate_dev(t.data_ptr(), t.numel(), out.data_ptr(), out.numel(), C.byref(n))
    if rc:
        _raise(rc)
    return out[: n.value]


def inflate_tensor(t, out, flags=0):
    """Decompress a 1-D uint8 CUDA tensor into ``out``; returns the filled view of ``out``."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    t = _aligned(t)
    assert out.data_ptr() % 16 == 0, "inflate_tensor: `out` must start on a 16-byte boundary (include/zes.h: device forms)"
    torch.cuda.current_stream(t.device).synchronize()
    n = C.c_uint64()
    rc = lib().zes_inflate_dev(t.data_ptr(), t.numel(), out.data_ptr(), out.numel(), C.byref(n), flags)
    _raise_need(rc, n)
    return out[: n.value]


def adler32_tensor(t):
    import torch

    torch.cuda.current_stream(t.device).synchronize()
    out = C.c_uint32()
    rc = lib().zes_adler32_dev(t.data_ptr(), t.numel(), C.byref(out))
    if rc:
        _raise(rc)
    return out.value


def crc32_tensor(t):
    """CRC-32 of a uint8 CUDA tensor at any alignment (zes_crc32_dev)."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    torch.cuda.current_stream(t.device).synchronize()
    out = C.c_uint32()
    rc = lib().zes_crc32_dev(t.data_ptr(), t.numel(), C.byref(out))
    if rc:
        _raise(rc)
    return out.value


_len = len  # (the batch checksums have a parameter of that name, after the C entry points)


def _checksum_batch_tensor(fn, who, d_in, off, len):
    import torch

    assert d_in.is_cuda and d_in.dtype == torch.uint8 and d_in.is_contiguous()
    cnt = _len(off)
    assert _len(len) == cnt
    assert all(int(o) + int(n) <= d_in.numel() for o, n in zip(off, len)), "%s: a buffer reaches beyond d_in" % who
    torch.cuda.current_stream(d_in.device).synchronize()
    out = (C.c_uint32 * cnt)()
    rc = fn(d_in.data_ptr(), (C.c_uint64 * cnt)(*[int(x) for x in off]), (C.c_uint64 * cnt)(*[int(x) for x in len]), out, cnt)
    if rc:
        _raise(rc)
    return list(out)


def adler32_batch_tensor(d_in, off, len):
    """Adler-32 of every d_in[off[i] : off[i] + len[i]] of a uint8 CUDA tensor, any alignment and length, in one launch
    (zes_adler32_batch_dev); returns a list of ints."""
    return _checksum_batch_tensor(lib().zes_adler32_batch_dev, "adler32_batch_tensor", d_in, off, len)


def crc32_batch_tensor(d_in, off, len):
    """CRC-32 of every d_in[off[i] : off[i] + len[i]] of a uint8 CUDA tensor, any alignment and length, in one launch
    (zes_crc32_batch_dev); returns a list of ints."""
    return _checksum_batch_tensor(lib().zes_crc32_batch_dev, "crc32_batch_tensor", d_in, off, len)


def gzip_tensor(t, out=None):
    """gzip of a 1-D uint8 CUDA tensor (zes_gzip_dev); returns a view of ``out`` (allocated if None)."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    cap = gzip_bound(t.numel())
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=t.device)
    assert out.data_ptr() % 16 == 0, "gzip_tensor: `out` must start on a 16-byte boundary (include/zes.h: device forms)"
    torch.cuda.current_stream(t.device).synchronize()
    n = C.c_uint64()
    rc = lib().zes_gzip_dev(t.data_ptr(), t.numel(), out.data_ptr(), out.numel(), C.byref(n))
    if rc:
        _raise(rc)
    return out[: n.value]


def bgzip_tensor(t, out=None, flags=0, index=False):
    """BGZF file of a 1-D uint8 CUDA tensor (zes_bgzip_dev); returns a view of ``out`` (allocated if None), or with
    index=True ``(view, offsets)``.  ``t`` and ``out`` may start at any byte; only the result's bytes are written."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    if out is None:
        out = torch.empty(bgzip_bound(t.numel()), dtype=torch.uint8, device=t.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    torch.cuda.current_stream(t.device).synchronize()
    off = (C.c_uint64 * bgzip_members(t.numel()))()
    n = C.c_uint64()
    rc = lib().zes_bgzip_dev(t.data_ptr() if t.numel() else None, t.numel(), out.data_ptr(), out.numel(), C.byref(n), off, flags)
    _raise_need(rc, n)
    return (out[: n.value], list(off)) if index else out[: n.value]


def gunzip_tensor(t, out, flags=0):
    """gunzip of a 1-D uint8 CUDA tensor (any alignment) into ``out`` (zes_gunzip_dev); returns the filled view."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    assert out.data_ptr() % 16 == 0, "gunzip_tensor: `out` must start on a 16-byte boundary (include/zes.h: device forms)"
    torch.cuda.current_stream(t.device).synchronize()
    n = C.c_uint64()
    rc = lib().zes_gunzip_dev(t.data_ptr(), t.numel(), out.data_ptr(), out.numel(), C.byref(n), flags)
    _raise_need(rc, n)
    return out[: n.value]


def _gz_batch_tensor(fn, who, bound, d_in, in_off, in_len, out, off, cap, flags):
    """gzip_batch_tensor and gunzip_batch_tensor: the same arguments and placement; ``bound()``: every item's room when ``off``
    is not given."""
    import torch

    assert d_in.is_cuda and d_in.dtype == torch.uint8 and d_in.is_contiguous()
    ioff = np.ascontiguousarray(in_off, dtype=np.uint64)
    ilen = np.ascontiguousarray(in_len, dtype=np.uint64)
    cnt = ilen.size
    assert ioff.ndim == 1 and ioff.shape == ilen.shape, "%s: one offset and one length per file" % who
    assert all(int(o) + int(n) <= d_in.numel() for o, n in zip(ioff, ilen)), "%s: a file reaches beyond `d_in`" % who
    torch.cuda.current_stream(d_in.device).synchronize()
    out_len = np.zeros(max(cnt, 1), dtype=np.uint64)
    status = np.zeros(max(cnt, 1), dtype=np.int32)
    src = d_in.data_ptr() if d_in.numel() else None

    def call(dst, o, c):
        rc = fn(src, _ptr(ioff), _ptr(ilen), cnt, dst, _ptr(o), _ptr(c), out_len.ctypes.data, status.ctypes.data, flags)
        if rc:
            _raise(rc)

    if off is None:
        sizes = (np.array(bound(call, cnt, status, out_len), dtype=np.uint64).reshape(-1)[:cnt] + np.uint64(15)) & ~np.uint64(15)
        off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(sizes, dtype=np.uint64)])[:cnt]
        if out is None:
            out = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=d_in.device)
        if cap is None:
            cap = sizes
    off = np.ascontiguousarray(off, dtype=np.uint64)
    assert off.size == cnt, "%s: one offset per file" % who
    if cap is None:
        cap = np.array([max((out.numel() if out is not None else 0) - int(o), 0) for o in off], dtype=np.uint64)
    cap = np.ascontiguousarray(cap, dtype=np.uint64)
    assert cap.size == cnt, "%s: one capacity per file" % who
    if out is not None:
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        assert all(int(o) + int(c) <= out.numel() for o, c in zip(off, cap)), "%s: a place reaches beyond `out`" % who
    call(out.data_ptr() if out is not None and out.numel() else None, off, cap)
    return out, off, [int(x) for x in out_len[:cnt]], [int(x) for x in status[:cnt]]


def gzip_batch_tensor(d_in, in_off, in_len, out=None, off=None, cap=None, flags=0):
    """Buffers in a 1-D uint8 CUDA tensor written as one gzip file each in one batch (zes_gzip_batch_dev): buffer i is
    ``d_in[in_off[i] : in_off[i] + in_len[i]]``.  Returns ``(out, off, out_len, status)``: file i is
    ``out[off[i] : off[i] + out_len[i]]`` when ``status[i]`` is 0, and nothing else of ``out`` is written.  ``d_in``, ``out`` and
    every offset may be any byte.  Without ``off`` the files are placed at 16-byte boundaries with gzip_batch_bound()'s room
    each and ``out`` is allocated when it is None.  ``cap``: the capacity of every file's place (default: the bound, or up to
    the end of ``out`` with ``off``); a file that needs more is ZES_E_NOSPACE with its ``out_len`` the size needed, so a call
    with ``out=None`` and zero capacities is a sizing pass."""
    return _gz_batch_tensor(lib().zes_gzip_batch_dev, "gzip_batch_tensor", lambda call, cnt, status, out_len: gzip_batch_bound(in_len), d_in, in_off,
                            in_len, out, off, cap, flags)


def gunzip_batch_tensor(d_in, in_off, in_len, out=None, off=None, cap=None, flags=0):
    """gzip files in a 1-D uint8 CUDA tensor decoded in one batch (zes_gunzip_batch_dev): file i is
    ``d_in[in_off[i] : in_off[i] + in_len[i]]``.  Returns ``(out, off, out_len, status)``: per file what gunzip_tensor gives for
    it alone with ``cap[i]`` as its capacity; output i is ``out[off[i] : off[i] + out_len[i]]`` when ``status[i]`` is 0.  ``d_in``,
    ``out`` and every offset may be any byte.  Without ``off`` a sizing pass comes first and the outputs are packed at 16-byte
    boundaries from the start of ``out``, which is allocated when it is None.  ``cap``: as in gzip_batch_tensor.  ``flags``:
    ZES_F_PIECES, ZES_F_GZIP_SERIAL (every file on the per-file route)."""

    def sizes(call, cnt, status, out_len):
        zeros = np.zeros(max(cnt, 1), dtype=np.uint64)
        call(None, zeros, zeros)
        return np.where(status[:cnt] == ZES_E_NOSPACE, out_len[:cnt], 0)

    return _gz_batch_tensor(lib().zes_gunzip_batch_dev, "gunzip_batch_tensor", sizes, d_in, in_off, in_len, out, off, cap, flags)


def bgzf_index_tensor(t, flags=0):
    """bgzf_index of a 1-D uint8 CUDA tensor (any alignment; zes_bgzf_index_dev): the members are found on the device by
    the parallel finder, or with ZES_F_INDEX_WALK by the serial walk."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    torch.cuda.current_stream(t.device).synchronize()
    return _bgzf_index_call(lib().zes_bgzf_index_dev, t.data_ptr() if t.numel() else None, t.numel(), flags)


def bgzf_read_tensor(t, index, pos, length, out, flags=0):
    """bgzf_read of a 1-D uint8 CUDA tensor into ``out`` (zes_bgzf_read_dev); returns the filled view.  ``t`` and ``out`` may
    start at any byte; only the result's bytes are written."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    coff, uoff = _bgzf_index_arrays(index)
    torch.cuda.current_stream(t.device).synchronize()
    n = C.c_uint64()
    rc = lib().zes_bgzf_read_dev(t.data_ptr(), t.numel(), coff.ctypes.data, uoff.ctypes.data, coff.size - 1, pos, length, out.data_ptr(), out.numel(),
                                 C.byref(n), flags)
    _raise_need(rc, n)
    return out[: n.value]


def zip_index_tensor(t):
    """zip_index of a 1-D uint8 CUDA tensor (any alignment; zes_zip_index_dev): two copies to the host — the file's last
    65557 bytes, then the directory — and no launch."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    torch.cuda.current_stream(t.device).synchronize()
    return _zip_index_call(lib().zes_zip_index_dev, t.data_ptr() if t.numel() else None, t.numel())


def zip_read_tensor(t, index, sel=None, out=None, off=None, flags=0):
    """zip_read of a 1-D uint8 CUDA tensor (zes_zip_read_dev): ``(out, off, out_len, status)``.  Entry i of the selection is
    written to ``out[off[i] : off[i] + usize]`` and nothing else is; ``t``, ``out`` and every offset may be any byte.  Without
    ``off`` the entries are packed at 16-byte boundaries from the start of ``out``, which is allocated when it is None."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    ent = _zip_entries(index)
    s, cnt = _zip_sel(ent, sel)
    if s is not None and cnt and int(s.max()) >= ent.size:
        _raise(ZES_E_ARG)
    picked = ent if s is None else ent[s]
    if off is None:  # packed at 16-byte boundaries
        sizes = (picked["usize"].astype(np.uint64) + np.uint64(15)) & ~np.uint64(15)
        off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(sizes, dtype=np.uint64)])[: picked.size]
        if out is None:
            out = torch.empty(int(sizes.sum()) if picked.size else 0, dtype=torch.uint8, device=t.device)
    assert out is not None and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    assert off.size == cnt, "zip_read_tensor: one offset per selected entry"
    assert all(int(o) + int(e["usize"]) <= out.numel() for o, e in zip(off, picked)), "zip_read_tensor: an entry reaches beyond `out`"
    torch.cuda.current_stream(t.device).synchronize()
    out_len = np.zeros(max(cnt, 1), dtype=np.uint64)
    status = np.zeros(max(cnt, 1), dtype=np.int32)
    rc = lib().zes_zip_read_dev(t.data_ptr() if t.numel() else None, t.numel(), ent.ctypes.data if ent.size else None, ent.size,
                                s.ctypes.data if s is not None and cnt else None, cnt, out.data_ptr() if out.numel() else None,
                                off.ctypes.data if cnt else None, out_len.ctypes.data, status.ctypes.data, flags)
    if rc:
        _raise(rc)
    return out, off, [int(x) for x in out_len[:cnt]], [int(x) for x in status[:cnt]]


def zip_write_tensor(d_in, in_off, in_len, names, out=None, flags=0):
    """zip_write of entries in a 1-D uint8 CUDA tensor (zes_zipwrite_dev): entry i is ``d_in[in_off[i] : in_off[i] + in_len[i]]``
    under ``names[i]``.  Returns ``(view, index)``: the filled view of ``out`` (allocated to zip_bound() if None) and the index
    as zip_index() returns it.  ``d_in``, ``out`` and every offset may be any byte; only the result's bytes are written."""
    import torch

    assert d_in.is_cuda and d_in.dtype == torch.uint8 and d_in.is_contiguous()
    off = np.ascontiguousarray(in_off, dtype=np.uint64)
    ln = np.ascontiguousarray(in_len, dtype=np.uint64)
    blob, nl = _zip_names(names)
    cnt = ln.size
    assert off.ndim == 1 and off.shape == ln.shape and nl.size == cnt, "zip_write_tensor: one offset, one length and one name per entry"
    assert all(int(o) + int(n) <= d_in.numel() for o, n in zip(off, ln)), "zip_write_tensor: an entry reaches beyond `d_in`"
    if out is None:
        out = torch.empty(zip_bound(ln, nl), dtype=torch.uint8, device=d_in.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    torch.cuda.current_stream(d_in.device).synchronize()
    ent = np.zeros(cnt, dtype=ZIP_ENTRY)
    n = C.c_uint64()
    rc = lib().zes_zipwrite_dev(d_in.data_ptr() if d_in.numel() else None, _ptr(off), _ptr(ln), _ptr(blob), _ptr(nl), cnt,
                                out.data_ptr() if out.numel() else None, out.numel(), C.byref(n), _ptr(ent), flags)
    _raise_need(rc, n)
    raw = blob.tobytes()
    return out[: n.value], (ent, [raw[int(e["name_off"]) : int(e["name_off"]) + int(e["name_len"])] for e in ent])


def png_decode_tensor(d_in, in_off, in_len, out=None, off=None, flags=0, cap=None):
    """PNG files in a 1-D uint8 CUDA tensor decoded as one batch (zes_png_decode_dev): file i is
    ``d_in[in_off[i] : in_off[i] + in_len[i]]``.  Returns ``(out, off, out_len, status, info)``: image i's scanlines are
    ``out[off[i] : off[i] + out_len[i]]`` when ``status[i]`` is 0, and nothing else of ``out`` is written; ``info`` is a PNG_INFO
    array.  ``d_in``, ``out`` and every offset may be any byte.  Without ``off`` a sizing pass (the chunk walk alone) comes
    first and the images are packed at 16-byte boundaries from the start of ``out``, which is allocated when it is None.
    ``cap``: the capacity of every image's place (default: up to the end of ``out``); an image that needs more is
    ZES_E_NOSPACE with its ``out_len`` the size needed.  ``flags``: ZES_F_PNG_INTERLACED to take Adam7-interlaced files too
    (ZES_E_UNSUPPORTED without it); their sizes and scanlines are those of non-interlaced files of the same pixels."""
    return _png_tensor(False, d_in, in_off, in_len, out, off, flags, cap)


def _png_tensor(_pix, d_in, in_off, in_len, out, off, flags, cap):
    """png_decode_tensor and, with ``_pix``, png_pixels_tensor: the same arguments, sizing pass and placement."""
    import torch

    assert d_in.is_cuda and d_in.dtype == torch.uint8 and d_in.is_contiguous()
    ioff = np.ascontiguousarray(in_off, dtype=np.uint64)
    ilen = np.ascontiguousarray(in_len, dtype=np.uint64)
    cnt = ilen.size
    assert ioff.ndim == 1 and ioff.shape == ilen.shape, "png_decode_tensor: one offset and one length per file"
    assert all(int(o) + int(n) <= d_in.numel() for o, n in zip(ioff, ilen)), "png_decode_tensor: a file reaches beyond `d_in`"
    torch.cuda.current_stream(d_in.device).synchronize()
    out_len = np.zeros(max(cnt, 1), dtype=np.uint64)
    status = np.zeros(max(cnt, 1), dtype=np.int32)
    info = np.zeros(max(cnt, 1), dtype=PNG_INFO)
    src = d_in.data_ptr() if d_in.numel() else None

    def call(dst, o, c):
        fn = lib().zes_pngpix_dev if _pix else lib().zes_png_decode_dev
        rc = fn(src, _ptr(ioff), _ptr(ilen), cnt, dst, _ptr(o), _ptr(c), out_len.ctypes.data, status.ctypes.data, info.ctypes.data, flags)
        if rc:
            _raise(rc)

    if off is None:  # the sizes first, then packed at 16-byte boundaries
        zeros = np.zeros(max(cnt, 1), dtype=np.uint64)
        call(None, zeros, zeros)
        sizes = (np.where(status[:cnt] == ZES_E_NOSPACE, out_len[:cnt], 0).astype(np.uint64) + np.uint64(15)) & ~np.uint64(15)
        off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(sizes, dtype=np.uint64)])[:cnt]
        if out is None:
            out = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=d_in.device)
        if cap is None:
            cap = sizes
    assert out is not None and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
    off = np.ascontiguousarray(off, dtype=np.uint64)
    assert off.size == cnt, "png_decode_tensor: one offset per file"
    if cap is None:
        cap = np.array([max(out.numel() - int(o), 0) for o in off], dtype=np.uint64)
    cap = np.ascontiguousarray(cap, dtype=np.uint64)
    assert cap.size == cnt and all(int(o) + int(c) <= out.numel() for o, c in zip(off, cap)), "png_decode_tensor: a place reaches beyond `out`"
    call(out.data_ptr() if out.numel() else None, off, cap)
    return out, off, [int(x) for x in out_len[:cnt]], [int(x) for x in status[:cnt]], info[:cnt]


def png_pixels_tensor(d_in, in_off, in_len, out=None, off=None, flags=0, cap=None):
    """PNG files in a 1-D uint8 CUDA tensor decoded to pixels as one batch (zes_pngpix_dev): png_decode_tensor's arguments and
    result, ``(out, off, out_len, status, info)``, with image i's ``width * height * 4`` bytes of R, G, B, A at
    ``out[off[i] : off[i] + out_len[i]]`` (the conversion rule of include/zes.h).  ``flags``: ZES_F_PNG_INTERLACED as in
    png_decode_tensor."""
    return _png_tensor(True, d_in, in_off, in_len, out, off, flags, cap)


def png_encode_tensor(d_in, in_off, in_len, images, aux=b"", out=None, off=None, cap=None, flags=0):
    """Images in a 1-D uint8 CUDA tensor written as PNG files in one batch (zes_pngwrite_dev): image i's scanlines are
    ``d_in[in_off[i] : in_off[i] + in_len[i]]`` and ``images[i]`` (a PNGW_IMAGE array) says what they are; ``aux`` holds every
    image's PLTE then tRNS data, back to back.  Returns ``(out, off, out_len, status)``: file i is
    ``out[off[i] : off[i] + out_len[i]]`` when ``status[i]`` is 0, and nothing else of ``out`` is written.  ``d_in``, ``out`` and
    every offset may be any byte.  Without ``off`` the files are placed at 16-byte boundaries with png_bound()'s room each and
    ``out`` is allocated when it is None.  ``cap``: the capacity of every file's place (default: png_bound(), or up to the end
    of ``out`` with ``off``); a file that needs more is ZES_E_NOSPACE with its ``out_len`` the size needed."""
    import torch

    assert d_in.is_cuda and d_in.dtype == torch.uint8 and d_in.is_contiguous()
    ioff = np.ascontiguousarray(in_off, dtype=np.uint64)
    ilen = np.ascontiguousarray(in_len, dtype=np.uint64)
    img = np.ascontiguousarray(images, dtype=PNGW_IMAGE).reshape(-1)
    cnt = ilen.size
    assert ioff.ndim == 1 and ioff.shape == ilen.shape and img.size == cnt, "png_encode_tensor: one offset, one length and one record per image"
    ok = np.array(png_bound(img), dtype=np.uint64) != 0
    assert all(int(o) + int(n) <= d_in.numel() for o, n, k in zip(ioff, ilen, ok) if k), "png_encode_tensor: an image reaches beyond `d_in`"
    a = np.frombuffer(bytes(aux), dtype=np.uint8)
    if off is None:
        sizes = (np.array(png_bound(img), dtype=np.uint64) + np.uint64(15)) & ~np.uint64(15)
        off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(sizes, dtype=np.uint64)])[:cnt]
        if out is None:
            out = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=d_in.device)
        if cap is None:
            cap = sizes
    off = np.ascontiguousarray(off, dtype=np.uint64)
    assert off.size == cnt, "png_encode_tensor: one offset per image"
    if cap is None:
        cap = np.array([max((out.numel() if out is not None else 0) - int(o), 0) for o in off], dtype=np.uint64)
    cap = np.ascontiguousarray(cap, dtype=np.uint64)
    if out is not None:
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        assert cap.size == cnt and all(int(o) + int(c) <= out.numel() for o, c in zip(off, cap)), "png_encode_tensor: a place reaches beyond `out`"
    torch.cuda.current_stream(d_in.device).synchronize()
    out_len = np.zeros(max(cnt, 1), dtype=np.uint64)
    status = np.zeros(max(cnt, 1), dtype=np.int32)
    rc = lib().zes_pngwrite_dev(d_in.data_ptr() if d_in.numel() else None, _ptr(ioff), _ptr(ilen), _ptr(img), _ptr(a), cnt,
                                out.data_ptr() if out is not None and out.numel() else None, _ptr(off), _ptr(cap), out_len.ctypes.data,
                                status.ctypes.data, flags)
    if rc:
        _raise(rc)
    return out, off, [int(x) for x in out_len[:cnt]], [int(x) for x in status[:cnt]]


def png_expand_tensor(d_in, in_off, in_len, images, aux=b"", out=None, off=None, cap=None):
    """Scanlines in a 1-D uint8 CUDA tensor turned into pixels in one launch (zes_pngpix_expand_dev): png_encode_tensor's
    arguments — image i's scanlines are ``d_in[in_off[i] : in_off[i] + in_len[i]]`` as png_decode_tensor leaves them,
    ``images[i]`` (a PNGW_IMAGE array, its ``filter`` ignored) says what they are, ``aux`` holds every image's PLTE then tRNS
    data.  Returns ``(out, off, out_len, status)``: image i's ``width * height * 4`` bytes of R, G, B, A are
    ``out[off[i] : off[i] + out_len[i]]`` when ``status[i]`` is 0, and nothing else of ``out`` is written.  Without ``off`` the
    images are packed at 16-byte boundaries and ``out`` is allocated when it is None; ``cap`` as in png_encode_tensor."""
    import torch

    assert d_in.is_cuda and d_in.dtype == torch.uint8 and d_in.is_contiguous()
    ioff = np.ascontiguousarray(in_off, dtype=np.uint64)
    ilen = np.ascontiguousarray(in_len, dtype=np.uint64)
    img = np.ascontiguousarray(images, dtype=PNGW_IMAGE).reshape(-1)
    cnt = ilen.size
    assert ioff.ndim == 1 and ioff.shape == ilen.shape and img.size == cnt, "png_expand_tensor: one offset, one length and one record per image"
    plain = img.copy()
    plain["filter"] = 0
    ok = np.array(png_bound(plain), dtype=np.uint64) != 0  # (the writer's rule on the records: the call's own check)
    assert all(int(o) + int(n) <= d_in.numel() for o, n, k in zip(ioff, ilen, ok) if k), "png_expand_tensor: an image reaches beyond `d_in`"
    a = np.frombuffer(bytes(aux), dtype=np.uint8)
    if off is None:
        sizes = np.where(ok, img["width"].astype(np.uint64) * img["height"].astype(np.uint64) * np.uint64(4), np.uint64(0)).astype(np.uint64)
        sizes = (sizes + np.uint64(15)) & ~np.uint64(15)
        off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(sizes, dtype=np.uint64)])[:cnt]
        if out is None:
            out = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=d_in.device)
        if cap is None:
            cap = sizes
    off = np.ascontiguousarray(off, dtype=np.uint64)
    assert off.size == cnt, "png_expand_tensor: one offset per image"
    if cap is None:
        cap = np.array([max((out.numel() if out is not None else 0) - int(o), 0) for o in off], dtype=np.uint64)
    cap = np.ascontiguousarray(cap, dtype=np.uint64)
    if out is not None:
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        assert cap.size == cnt and all(int(o) + int(c) <= out.numel() for o, c in zip(off, cap)), "png_expand_tensor: a place reaches beyond `out`"
    torch.cuda.current_stream(d_in.device).synchronize()
    out_len = np.zeros(max(cnt, 1), dtype=np.uint64)
    status = np.zeros(max(cnt, 1), dtype=np.int32)
    rc = lib().zes_pngpix_expand_dev(d_in.data_ptr() if d_in.numel() else None, _ptr(ioff), _ptr(ilen), _ptr(img), _ptr(a), cnt,
                                     out.data_ptr() if out is not None and out.numel() else None, _ptr(off), _ptr(cap), out_len.ctypes.data,
                                     status.ctypes.data, 0)
    if rc:
        _raise(rc)
    return out, off, [int(x) for x in out_len[:cnt]], [int(x) for x in status[:cnt]]


def _batch_call(fn, d_in, in_off, in_len, d_out, out_off, out_cap, *extra):
    import torch

    cnt = len(in_off)
    arr = lambda v: (C.c_uint64 * cnt)(*[int(x) for x in v])
    out_len = (C.c_uint64 * cnt)()
    status = (C.c_int32 * cnt)()
    torch.cuda.current_stream(d_in.device).synchronize()
    rc = fn(d_in.data_ptr(), arr(in_off), arr(in_len), d_out.data_ptr(), arr(out_off), arr(out_cap), out_len, status, cnt, *extra)
    if rc:
        _raise(rc)
    return list(out_len), list(status)


def deflate_batch_tensor(d_in, in_off, in_len, d_out, out_off, out_cap):
    """Independent buffers inside one arena: every in_off may be any byte, every out_off (and d_out) 16-byte aligned;
    returns (out_len[], status[])."""
    return _batch_call(lib().zes_deflate_batch_dev, d_in, in_off, in_len, d_out, out_off, out_cap)


def inflate_batch_tensor(d_in, in_off, in_len, d_out, out_off, out_cap, flags=0):
    """Independent zlib streams inside one arena (offsets 16-byte aligned); returns (out_len[], status[]).  With
    ZES_F_CHECK_ADLER in ``flags`` a stream whose Adler-32 trailer is missing or does not match its result gets the status
    ZES_E_CHECKSUM; its out_len stays the decoded length and its bytes stay written."""
    return _batch_call(lib().zes_inflate_batch_dev, d_in, in_off, in_len, d_out, out_off, out_cap, flags)


def deflate_range_tensor(t, lo, hi, final, out=None):
    """Raw bit stream of the block range [lo, hi) of the CUDA tensor ``t`` (one buffer split over several GPUs,
    SURVEY §8e-ii) -> (bytes view, nbits, adler32 of the range).  The 258-byte halo behind ``hi`` is read from ``t``."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and lo % BLOCK_MAX_BUFFER_LEN == 0
    view = _aligned(t[lo:])  # (lo is a block boundary: aligned whenever t is)
    n = hi - lo
    cap = deflate_bound(n)
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=t.device)
    torch.cuda.current_stream(t.device).synchronize()
    bits, ad = C.c_uint64(), C.c_uint32()
    rc = lib().zes_deflate_range_dev(view.data_ptr(), n, min(view.numel(), n + 258), 1 if final else 0, out.data_ptr(), out.numel(),
                                     C.byref(bits), C.byref(ad))
    if rc:
        _raise(rc)
    return out[: (bits.value + 7) // 8], bits.value, ad.value


def deflate_join_tensors(pieces, bits, adlers, lens, out=None):
    """zlib stream of one buffer from the bit streams of its consecutive block ranges (CUDA tensors on this device)."""
    import torch

    cnt = len(pieces)
    total = 2 + (sum(bits) + 7) // 8 + 4
    if out is None:
        out = torch.empty((total + 15) // 16 * 16, dtype=torch.uint8, device=pieces[0].device)
    torch.cuda.current_stream(out.device).synchronize()
    n = C.c_uint64()
    rc = lib().zes_deflate_join_dev((C.c_void_p * cnt)(*[p.data_ptr() for p in pieces]), (C.c_uint64 * cnt)(*bits),
                                    (C.c_uint32 * cnt)(*adlers), (C.c_uint64 * cnt)(*lens), cnt, out.data_ptr(), out.numel(), C.byref(n))
    if rc:
        _raise(rc)
    return out[: n.value]


def inflate_range_tensor(t, lo_bit, own_bit, exact, out):
    """The blocks of a reference-made zlib stream (CUDA tensor ``t``, the whole stream) that start at bits
    lo_bit <= s < own_bit of it, decoded into ``out`` (block k of the range at k * 131072) -> (out_len, first_bit,
    end_bit, nblocks, final) with bit positions relative to the stream, or None when the range is not a clean chain
    of reference-made blocks (zes_inflate_range_dev; one stream split over several GPUs)."""
    import torch

    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and out.is_cuda
    lo_bit = max(16, int(lo_bit))
    byte0 = (lo_bit >> 3) & ~15  # (t1_piece_origin of csrc/zes_api.hip, restated: the C ABI takes the piece, not the stream)
    if byte0 >= 16:
        byte0 -= 16  # (the search starts 16 bits into what it is given)
    end = min(t.numel(), (int(own_bit) + 7) // 8 + (1 << 20))  # the last block's bytes and the header behind it
    view = _aligned(t[byte0:end])
    torch.cuda.current_stream(t.device).synchronize()
    n, fb, eb, nb, fin = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_int32()
    rc = lib().zes_inflate_range_dev(view.data_ptr(), view.numel(), lo_bit - 8 * byte0, int(own_bit) - 8 * byte0, 1 if exact else 0,
                                     out.data_ptr(), out.numel(), C.byref(n), C.byref(fb), C.byref(eb), C.byref(nb), C.byref(fin))
    if rc == ZES_E_NOTRANGE:
        return None
    if rc:
        _raise(rc)
    return n.value, fb.value + 8 * byte0, eb.value + 8 * byte0, nb.value, bool(fin.value)


def last_inflate_tier():
    """1 block-parallel, 2 segment-parallel (any stream), 3 sequential wavefront, 4 exact restatement."""
    return int(lib().zes_last_inflate_tier())


def last_gunzip_members():
    """Members the member-parallel path decoded in this thread's last gunzip call (0: the member-by-member path answered),
    or the members the last bgzf_read decoded."""
    return int(lib().zes_last_gunzip_members())


# ---- TIFF reader (include/zes.h: "zes_tiff_*") -------------------------------------------------
def _tiff_dict(img, dirs):
    d = {k: int(img[k]) for k in TIFF_IMAGE.names}
    d["dirs"] = int(dirs)
    return d


def _tiff_index(fn, ptr, size, dir):
    """Both index forms: the sizing call, then the arrays.  (record, seg_off, seg_len, dirs)."""
    img = np.zeros(1, dtype=TIFF_IMAGE)
    nseg, dirs = C.c_uint64(), C.c_uint32()
    rc = fn(ptr, size, int(dir), img.ctypes.data, None, None, 0, C.byref(nseg), C.byref(dirs), 0)
    if rc not in (ZES_OK, ZES_E_NOSPACE):
        err = ZlibEsError(rc, strerror(rc))
        err.dirs = dirs.value
        raise err
    off, ln = np.zeros(nseg.value, dtype=np.uint64), np.zeros(nseg.value, dtype=np.uint64)
    rc = fn(ptr, size, int(dir), img.ctypes.data, _ptr(off), _ptr(ln), off.size, C.byref(nseg), C.byref(dirs), 0)
    if rc:
        _raise(rc)
    return img[0].copy(), off, ln, dirs.value


def tiff_index(data, dir=0):
    """The index of directory ``dir`` of a TIFF file (zes_tiff_index; no GPU needed): ``(info, seg_off, seg_len)`` — the
    record as tiff_info gives it, and the file positions and byte counts of its tiles or strips in row-major order."""
    a = _as_u8(data)
    img, off, ln, dirs = _tiff_index(lib().zes_tiff_index, _ptr(a), a.size, dir)
    return _tiff_dict(img, dirs), off, ln


def tiff_info(data, dir=0):
    """What the TIFF reader says about directory ``dir`` of a file (no GPU needed): the zes_tiff_image record as a dict —
    width, height, seg_w, seg_h, across, down, bits, spp, compression, predictor, photometric, sample_format, extra_samples,
    big_endian, tiled, out_size — plus ``dirs``, the length of the file's directory chain.  A file the rule refuses raises
    (``.dirs`` on the error when the chain was walked)."""
    return tiff_index(data, dir)[0]


def _tiff_rect(rect):
    if rect is None:
        return None, None
    r = (C.c_uint32 * 4)(*[int(v) for v in rect])
    return r, C.cast(r, C.c_void_p)


def tiff_dtype(info):
    """The numpy dtype of an image's samples: from ``bits`` and ``sample_format`` (2: signed, 3 at 32 bits: float32, else
    unsigned), little-endian as the reader writes them."""
    bits, fmt = int(info["bits"]), int(info["sample_format"])
    if fmt == 3 and bits == 32:
        return np.dtype("<f4")
    return np.dtype("<%s%d" % ("i" if fmt == 2 else "u", bits // 8))


def tiff_read(data, dir=0, rect=None, flags=0):
    """A rectangle ``(x, y, w, h)`` of directory ``dir`` of a TIFF file (None: the whole image) as a numpy array of shape
    ``(h, w, spp)`` (zes_tiff_read_alloc: only the tiles or strips under the rectangle are uploaded and decoded).  The dtype
    is tiff_dtype()'s.  A file the rule refuses, or a touched segment that fails, raises."""
    a = _as_u8(data)
    got = []

    def alloc(_user, _index, n):
        got.append(np.empty(max(int(n), 1), dtype=np.uint8))
        return got[0].ctypes.data

    img = np.zeros(1, dtype=TIFF_IMAGE)
    n = C.c_uint64()
    keep, r = _tiff_rect(rect)
    rc = lib().zes_tiff_read_alloc(_ptr(a), a.size, int(dir), r, ALLOC_FN(alloc), None, C.byref(n), img.ctypes.data, flags)
    if rc:
        _raise(rc)
    info = img[0]
    w, h = (int(info["width"]), int(info["height"])) if rect is None else (int(rect[2]), int(rect[3]))
    return got[0][: n.value].view(tiff_dtype(info)).reshape(h, w, int(info["spp"]))


def last_tiff_read():
    """``(segments, bytes_up)``: the segments the last tiff_read call's rectangle touched and the bytes it uploaded."""
    a, b = C.c_uint32(), C.c_uint64()
    lib().zes_last_tiff_read(C.byref(a), C.byref(b))
    return a.value, b.value


def tiff_index_tensor(t, dir=0):
    """tiff_index for a file in a 1-D uint8 CUDA tensor (zes_tiff_index_dev: only the header, the directories and the two
    arrays come down).  The result is what tiff_read_tensor takes as ``index``."""
    assert t.is_cuda and t.dtype.itemsize == 1 and t.dim() == 1 and t.is_contiguous(), "tiff_index_tensor: a 1-D uint8 CUDA tensor"
    img, off, ln, dirs = _tiff_index(lib().zes_tiff_index_dev, t.data_ptr() if t.numel() else None, t.numel(), dir)
    return _tiff_dict(img, dirs), off, ln


def tiff_read_tensor(t, index, rect=None, out=None, flags=0):
    """A rectangle of an indexed image decoded on the device (zes_tiff_read_dev): ``(pixels, seg_status, status)``.
    ``pixels`` is a uint8 tensor of shape ``(h, w, spp * bits / 8)`` — a view of ``out`` (a 1-D uint8 CUDA tensor, any
    alignment) when that is given — samples little-endian; ``seg_status`` has one status per segment (0 for one that was
    decoded or not touched) and ``status`` is the call's: 0, or the first failing segment's (the good segments' pixels are
    written all the same).  Anything else the call refuses raises."""
    import torch

    info, off, ln = index
    assert t.is_cuda and t.dtype.itemsize == 1 and t.dim() == 1 and t.is_contiguous(), "tiff_read_tensor: a 1-D uint8 CUDA tensor"
    img = np.zeros(1, dtype=TIFF_IMAGE)
    for k in TIFF_IMAGE.names:
        img[0][k] = info[k]
    w, h = (int(info["width"]), int(info["height"])) if rect is None else (int(rect[2]), int(rect[3]))
    ps = int(info["spp"]) * int(info["bits"]) // 8
    if out is None:
        out = torch.empty(max(w * h * ps, 1), dtype=torch.uint8, device=t.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous(), "tiff_read_tensor: `out` is a 1-D uint8 CUDA tensor"
    off, ln = np.ascontiguousarray(off, dtype=np.uint64), np.ascontiguousarray(ln, dtype=np.uint64)
    nseg = int(info["across"]) * int(info["down"])
    assert off.size == nseg and ln.size == nseg, "tiff_read_tensor: one offset and one length per segment"
    st = np.zeros(max(nseg, 1), dtype=np.int32)
    n = C.c_uint64()
    keep, r = _tiff_rect(rect)
    rc = lib().zes_tiff_read_dev(t.data_ptr() if t.numel() else None, t.numel(), img.ctypes.data, _ptr(off), _ptr(ln), r, out.data_ptr(), out.numel(),
                                 C.byref(n), st.ctypes.data, flags)
    if rc in (ZES_E_ARG, ZES_E_DEVICE, ZES_E_NOSPACE):
        _raise_need(rc, n)
    return out[: n.value].view(h, w, ps), st[:nseg], rc


# ---- TIFF writer (include/zes.h: "zes_tiffwrite*") ---------------------------------------------
def tiff_image(width, height, bits=8, spp=1, tile=None, rows=None, compression=8, predictor=2, photometric=None, sample_format=1, extra_samples=None,
               big_endian=False):
    """A consistent zes_tiff_image record (a dict, as tiff_info gives it without ``dirs``) for tiff_write: ``tile=(w, h)`` for
    tiles, else strips of ``rows`` rows (default: one strip).  photometric defaults to 2 (RGB) from 3 samples on, else 1;
    extra_samples to 2 (unassociated alpha) when there are samples beyond the photometric's.  Nothing is checked here: the
    write call does that."""
    width, height, spp = int(width), int(height), int(spp)
    assert tile is None or rows is None, "tiff_image: tiles or strips, not both"
    if tile is not None:
        seg_w, seg_h, tiled = int(tile[0]), int(tile[1]), 1
    else:
        seg_w, seg_h, tiled = width, min(int(rows), height) if rows is not None else height, 0
    if photometric is None:
        photometric = 2 if spp >= 3 else 1
    base = 3 if photometric == 2 else 1
    if extra_samples is None:
        extra_samples = 2 if spp > base else 0
    return dict(width=width, height=height, seg_w=seg_w, seg_h=seg_h, across=-(-width // seg_w) if seg_w else 0, down=-(-height // seg_h) if seg_h else 0,
                bits=int(bits), spp=spp, compression=int(compression), predictor=int(predictor), photometric=int(photometric),
                sample_format=int(sample_format), extra_samples=int(extra_samples), big_endian=int(bool(big_endian)), tiled=tiled,
                out_size=width * height * spp * (int(bits) // 8))


def _tiff_record(record):
    img = np.zeros(1, dtype=TIFF_IMAGE)
    for k in TIFF_IMAGE.names:
        img[0][k] = record[k]
    return img


def tiff_bound(record):
    """``(cap, segments)``: a capacity that always suffices for the file tiff_write makes of ``record`` - exact when every
    segment goes stored - and the number of its segments (zes_tiffwrite_bound; no GPU needed)."""
    img = _tiff_record(record)
    cap, nseg = C.c_uint64(), C.c_uint64()
    rc = lib().zes_tiffwrite_bound(img.ctypes.data, C.byref(cap), C.byref(nseg))
    if rc:
        _raise(rc)
    return cap.value, nseg.value


def tiff_write(pixels, record, flags=0):
    """The TIFF file of one image as ``bytes`` (zes_tiffwrite).  ``pixels``: what tiff_read gives for the whole image - an
    array of ``record["out_size"]`` bytes in all, rows from the top, samples little-endian - and ``record`` a tiff_image() or a
    tiff_info() of a file this writer accepts."""
    a = pixels if isinstance(pixels, np.ndarray) else np.frombuffer(bytes(pixels), dtype=np.uint8)
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    img = _tiff_record(record)
    got = []

    def alloc(_user, _index, n):
        got.append(np.empty(max(int(n), 1), dtype=np.uint8))
        return got[0].ctypes.data

    n = C.c_uint64()
    rc = lib().zes_tiffwrite(_ptr(a), a.size, img.ctypes.data, ALLOC_FN(alloc), None, C.byref(n), flags)
    if rc:
        _raise(rc)
    return got[0][: n.value].tobytes()


def tiff_write_tensor(t, record, out=None, flags=0):
    """The TIFF file of an image that lies in a 1-D uint8 CUDA tensor, written on the device (zes_tiffwrite_dev):
    ``(file, seg_off, seg_len)`` - the file a uint8 tensor (a view of ``out``, a 1-D uint8 CUDA tensor at any alignment, when
    that is given; else a tensor of tiff_bound()'s size is made) and the positions and byte counts of its segments, what
    tiff_index would give for it.  A capacity below the file's size raises with ``.need``."""
    import torch

    assert t.is_cuda and t.dtype.itemsize == 1 and t.dim() == 1 and t.is_contiguous(), "tiff_write_tensor: a 1-D uint8 CUDA tensor"
    img = _tiff_record(record)
    bound, nseg = tiff_bound(record)  # (raises for a record the writer refuses, before anything is sized by it)
    if out is None:
        out = torch.empty(bound, dtype=torch.uint8, device=t.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous(), "tiff_write_tensor: `out` is a 1-D uint8 CUDA tensor"
    off, ln = np.zeros(nseg, dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
    n = C.c_uint64()
    torch.cuda.current_stream(t.device).synchronize()  # the library runs on its own stream
    rc = lib().zes_tiffwrite_dev(t.data_ptr() if t.numel() else None, t.numel(), img.ctypes.data, out.data_ptr() if out.numel() else None, out.numel(),
                                 C.byref(n), off.ctypes.data, ln.ctypes.data, flags)
    if rc:
        _raise_need(rc, n)
    return out[: n.value], off, ln


def set_profiling(on):
    lib().zes_set_profiling(1 if on else 0)


def last_kernel_times():
    arr = (ZesKTime * 64)()
    n = lib().zes_last_kernel_times(arr, 64)
    return [(arr[i].name.decode(), float(arr[i].ms), int(arr[i].launches)) for i in range(n)]


# ---- stage-level entries used by the kernel parity tests -------------------------------------
def stage_lz77_tensor(t, start, length):
    tok = np.empty(length + 4, dtype=np.uint32)
    nt = C.c_uint32()
    rc = lib().zes_stage_lz77_dev(t.data_ptr(), t.numel(), start, length, tok.ctypes.data, C.byref(nt))
    if rc:
        _raise(rc)
    return tok[: nt.value].copy()


def stage_lz77_route():
    """zes_stage_lz77_route: the nine route words of this thread's last stage_lz77_tensor call (include/zes.h)."""
    w = np.zeros(9, dtype=np.uint32)
    rc = lib().zes_stage_lz77_route(w.ctypes.data, w.size)
    if rc:
        _raise(rc)
    return w


def stage_poison(word):
    """zes_stage_poison: every pool, the page-locked areas and the mirror of every ready context filled with the 32-bit
    ``word`` (include/zes.h); returns the bytes filled."""
    n = C.c_uint64(0)
    rc = lib().zes_stage_poison(int(word) & 0xFFFFFFFF, C.byref(n))
    if rc:
        _raise(rc)
    return int(n.value)


def selftest_lds_order(iters=200, seed=1):
    """zes_selftest_lds_order: (values out of lane order, values checked) of returning LDS adds on this device."""
    bad, n = C.c_uint64(0), C.c_uint64(0)
    rc = lib().zes_selftest_lds_order(iters, seed, C.byref(bad), C.byref(n))
    if rc:
        _raise(rc)
    return int(bad.value), int(n.value)


def stage_huff_lengths(hist, maxlen):
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    lens = np.zeros(h.size, dtype=np.uint8)
    rc = lib().zes_stage_huff_lengths_dev(h.ctypes.data, h.size, maxlen, lens.ctypes.data)
    if rc:
        _raise(rc)
    return lens


def stage_chain(records, cap, first_bit=16, on_device=False):
    """zes_stage_chain: T1's acceptance rule on candidate records [(start_bit, end_bit, out_len, flags), ...], decided on
    the host (no GPU needed) or by k_inf_chain.
    Returns (status, total, aux, chain): 0 accepted / 2 accepted, slots shifted / 1 declined (chain then [])."""
    n = len(records)
    cols = [np.ascontiguousarray([r[i] for r in records], dtype=dt) for i, dt in enumerate((np.uint32, np.uint64, np.uint32, np.uint32))]
    chain = np.zeros(max(n, 1), dtype=np.uint32)
    status, total, aux = C.c_int32(), C.c_uint64(), C.c_uint32()
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    ptr = lambda a, t: a.ctypes.data_as(t) if n else None
    rc = lib().zes_stage_chain(ptr(cols[0], u32p), ptr(cols[1], u64p), ptr(cols[2], u32p), ptr(cols[3], u32p), n, int(cap), int(first_bit),
                               1 if on_device else 0, C.byref(status), C.byref(total), C.byref(aux), chain.ctypes.data_as(u32p))
    if rc:
        _raise(rc)
    return int(status.value), int(total.value), int(aux.value), [int(x) for x in chain[: aux.value]] if status.value != 1 else []
