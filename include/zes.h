/*
 * zes.h — C-ABI of the MI355X-native DEFLATE engine (drop-in for zlib.es's hot path).
 *
 * Every entry point replaces one interface of the reference (zprodev/zlib.es v0.6.0);
 * the citation after "replaces:" is the reference file:line the entry point stands in for.
 * Plain pointers and sizes only, no exceptions across the boundary: every function returns
 * ZES_OK (0) or a negative zes_status.  zes_strerror() returns, for the reference-defined
 * codes, the exact message string the reference throws, so a binding can rethrow it verbatim
 * (see INTEGRATION.md for the N-API / ctypes stubs).
 *
 * Two families:
 *   zes_*      — host pointers (what an FFI binding hands over); the library stages through
 *                its own device buffers (H2D, kernels, D2H).
 *   zes_*_dev  — device pointers (HBM-resident in/out); nothing crosses PCIe except a few
 *                scalars.  This is what bench.py times.
 *
 * The product path is HIP only.  There is no CPU fallback in this library: without a usable
 * gfx950 device every compute entry point returns ZES_E_DEVICE.
 */
#ifndef ZES_H
#define ZES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum zes_status {
  ZES_OK = 0,
  /* reference-defined errors (message strings identical to the reference's `throw new Error`) */
  ZES_E_NOT_DEFLATE = -1,   /* 'Not compressed by deflate'     src/zlib.ts:15               */
  ZES_E_BTYPE3 = -2,        /* 'Not supported BTYPE : 3'       src/inflate.ts:32            */
  ZES_E_CORRUPT = -3,       /* 'Data is corrupted'             src/inflate.ts:50,88,166,247,276; src/deflate.ts:172,190,202,216,224 */
  ZES_E_INSUFFICIENT = -4,  /* 'Data length is insufficient'   src/inflate.ts:35            */
  ZES_E_LACK = -5,          /* 'Lack of data length'           src/utils/BitReadStream.ts:15, BitWriteStream.ts:15 */
  /* engine-defined errors (no reference counterpart) */
  ZES_E_NOSPACE = -16,      /* caller's output capacity too small; *out_len holds the size needed when known */
  ZES_E_DEVICE = -17,       /* HIP runtime error / no gfx950 device */
  ZES_E_ARG = -18,          /* bad argument (null pointer, size overflow) */
  ZES_E_NOTRANGE = -19,     /* zes_inflate_range_dev: the range does not hold a clean chain of reference-made blocks */
  ZES_E_GZIP = -20,         /* zes_gunzip*: not a gzip member (magic, CM, reserved flags, a header cut short), c == 0, or a trailer cut short */
  ZES_E_CHECKSUM = -21,     /* a trailer does not match the data: gzip CRC-32 / ISIZE / FHCRC, or zlib Adler-32 with ZES_F_CHECK_ADLER;
                               zes_zip_read*: an entry's size, stream end or CRC-32 is not what its directory record says */
  ZES_E_ZIP = -22,          /* zes_zip_*: not a ZIP archive this reader accepts, or an entry whose local header or sizes do not fit its
                               directory record */
  ZES_E_UNSUPPORTED = -23,  /* zes_zip_*: a valid archive or entry that uses something this reader does not implement: ZIP64, several
                               disks, encryption, a method other than 0 (stored) or 8 (DEFLATE); zes_png_*: a valid file with a
                               critical chunk this reader does not know, filtered data of more than 0xFFFFFFFF bytes, or (the
                               decode calls without ZES_F_PNG_INTERLACED) Adam7 interlace */
  ZES_E_PNG = -24,          /* zes_png_*: not a PNG file this reader accepts, or image data that does not fit its header */
  ZES_E_TIFF = -25          /* zes_tiff_*: not a TIFF file this reader accepts, or image data that does not fit its directory */
} zes_status;

/* Geometry of the reference format (src/const.ts:7). */
#define ZES_BLOCK_LEN 131072u

/* flags for zes_inflate*: */
#define ZES_F_DEFAULT 0u
#define ZES_F_NO_FASTPATH 1u   /* force the general (serial, any-stream) decoder: testing aid */
#define ZES_F_PIECES 4u        /* decode a reference-made stream piece by piece (1 MiB pieces) as streams of 512 MiB and more are
                                  * (256 MiB pieces): testing aid for that path; same results.  zes_bgzip*: encode the members in
                                  * groups of 4 instead of 1024, as inputs of more than 1024 chunks are encoded group by group:
                                  * testing aid for the seams between groups; same bytes */
#define ZES_F_ALLOC_BOUND 8u   /* zes_inflate_alloc: the allocator may be asked EARLY for an upper estimate of the result's size (the
                                 result is then a prefix of what it returned: *out_len says how long), and a second time for the exact
                                 size if the estimate fell short — the last pointer it returned holds the result.  For callers whose
                                 memory can show a prefix (the N-API addon's pooled blocks): the download then runs beside the decode
                                 instead of behind it (64 MiB of random bytes: 18 -> 25 GiB/s).  The early request carries
                                 ZES_ALLOC_EARLY in its index argument; the allocator may answer it with NULL ("not now": no block of
                                 that size at hand) and is then asked once, later, for the exact size as without the flag */
#define ZES_ALLOC_EARLY 0x80000000u
#define ZES_F_CHECK_ADLER 16u  /* zes_inflate, zes_inflate_dev, zes_inflate_size, zes_inflate_alloc, zes_inflate_batch_dev,
                                  zes_inflate_batch_alloc: the 4 bytes behind the stream must exist and hold the Adler-32 of the
                                  result (big-endian), else ZES_E_CHECKSUM.  In the batch forms that is the status of the buffer
                                  alone: its out_len stays the decoded length, a buffer with any other status keeps it, and
                                  zes_inflate_batch_alloc does not ask for memory for a buffer that fails.  All trailers of a batch
                                  are checked by one segmented launch (zes_adler32_batch_dev's kernel).  Without the flag the
                                  trailer is ignored, as the reference ignores it (src/zlib.ts:11-23) */
#define ZES_F_GZIP_SERIAL 32u   /* zes_gunzip*: decode the members one after the other even where they could go as one batch:
                                  testing aid, same results */
#define ZES_F_INDEX_WALK 64u    /* zes_bgzf_index_dev: find the members with k_gz_walk's serial chain instead of the
                                  parallel finder: testing aid and the baseline of the measurement; same results */
#define ZES_F_PNG_INTERLACED 128u /* zes_png_decode_dev, zes_png_decode_alloc, zes_pngpix_dev, zes_pngpix_alloc: decode files of
                                  interlace method 1 (Adam7) too, instead of answering ZES_E_UNSUPPORTED for them ("Interlaced
                                  images" below).  Files of interlace method 0 decode as without the flag */
#define ZES_F_LOOSE_CANDIDATES 2u /* block-start search without the reference's run-length-coding rules: more false
                                  * candidates reach the block decoder (testing aid for that path; same results) */

/* Exact reference message for a status (engine-defined codes get a descriptive string). */
const char* zes_strerror(int status);

/* Library/device lifecycle.  zes_init(device) binds the process to one HIP device (one process per GPU;
 * bench.py passes LOCAL_RANK).  Idempotent; a second call with another device returns ZES_E_ARG.  Every entry
 * point may be called from any thread: calls on one device are serialised by that device's lock and each makes the device
 * current on its calling thread for the duration of the call (HIP's current device is per thread).
 * replaces: nothing (the reference has no state); required because device scratch is pooled across calls. */
int zes_init(int device);
int zes_shutdown(void);
/* Gives the pooled device scratch back to the driver (every context's; ~10 bytes per input byte after a deflate call,
 * ~3 GB after another encoder's long stream) and keeps the contexts, streams and pinned staging: the next call
 * allocates what it needs again.  For a long-lived host that has had one large call.  replaces: nothing (the
 * reference's buffers are garbage collected). */
int zes_trim(void);
/* Bytes of pooled device scratch the library holds right now, over all contexts (what zes_trim would give back;
 * bench.py reports it per workload).  replaces: nothing. */
uint64_t zes_pool_bytes(void);
/* Several GPUs from ONE process (what a Node host is: SURVEY §8b `zes_init(int ngpus)`, "the batch API is where
 * multi-GPU concurrency lives").  zes_init_devices(n) gives the library n contexts, context i on device i (n <= 0: every
 * visible device) — its own stream, scratch pools, staging and lock each.  From then on the host-pointer entry points use
 * all of them: zes_deflate_batch / zes_inflate_batch_alloc partition their buffers by size (zes_partition) and run
 * every share on its own host thread against its own device, results straight into the caller's memory (the allocator
 * callback may then be called from several threads at once, always for distinct buffers); single host calls take the
 * devices in turn, so concurrent deflateAsync() calls land on different GPUs; device-pointer entry points run on the
 * device that holds their memory.  Results are identical to the one-device ones, buffer for buffer.  zes_init(device)
 * keeps meaning "this process drives that one device" (one process per GPU under torch.distributed).
 * zes_partition: owner[i] in [0, parts) for buffer i — longest first onto the lightest part so far, ties to the lower
 * index (the rule of zlib.es_amd/shard.py's partition()); no GPU involved.  zes_device_count: contexts in use.
 * replaces: the caller's own loop over buffers, README.md:28-42 (the reference is single-threaded). */
int zes_init_devices(int n);
int zes_device_count(void);
int zes_partition(const uint64_t* sizes, uint32_t count, uint32_t parts, uint32_t* owner);
/* Fills name (<= cap bytes) with the device's gcnArchName, *cus with its CU count. */
int zes_device_info(char* name, int cap, int* cus, uint64_t* hbm_bytes);

/* Page-locked host memory the DMA engines can read and write directly.  The host-pointer entry points accept any
 * memory (pageable buffers of 4 MiB and more are copied by the runtime's own call, shorter ones through a ring of pinned
 * chunks); buffers from here are handed to the DMA engines as they are, whatever their size.
 * A binding exposes it as an allocator for its callers' arrays (`allocPinned`).  Free before
 * zes_shutdown.  replaces: nothing (the reference works on ordinary Uint8Arrays). */
int zes_host_alloc(uint64_t n, void** p);
int zes_host_free(void* p);

/* Output capacity sufficient for zes_deflate of an n-byte input.
 * replaces: the `streamHeap` sizing in src/deflate.ts:16 (+6 for the zlib wrapper, src/zlib.ts:42). */
int zes_deflate_bound(uint64_t n, uint64_t* cap);

/* zlib-wrapped compress: out = 78 9C | raw deflate | Adler-32 BE.  Bit-exact with
 * replaces: `export function deflate(input)` src/zlib.ts:25-49 (→ src/deflate.ts:14-39, src/lz77.ts, src/huffman.ts:55-153, src/adler32.ts).
 * n == 0, n == 1 and n % 131072 == 1 return ZES_E_CORRUPT exactly as the reference throws.
 * Device forms (here and below): d_out, and in the batch forms every out_off, must be 16-byte aligned — results are
 * written as whole 16-byte groups — else ZES_E_ARG; the inflate device forms ask the same of d_in / in_off.  The
 * deflate device forms read an input at any alignment (the kernels fall back to narrower loads for an unaligned
 * block); zes_deflate_range_dev alone asks for an aligned d_in, see there.  The host forms take any alignment. */
int zes_deflate(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len);
int zes_deflate_dev(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len);

/* zlib-wrapped decompress.
 * replaces: `export function inflate(input)` src/zlib.ts:11-23 (→ src/inflate.ts:16-292, src/huffman.ts:8-53, src/utils/BitReadStream.ts).
 * Same accept-set and the same error for every malformed stream (checks only the CM nibble,
 * ignores FCHECK/FDICT and the Adler-32 trailer).  On ZES_E_NOSPACE *out_len = bytes needed. */
int zes_inflate(const uint8_t* in, uint64_t c, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags);
int zes_inflate_dev(const uint8_t* d_in, uint64_t c, uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint32_t flags);
/* Size-only pass (decodes, writes nothing to the caller, keeps nothing). */
int zes_inflate_size(const uint8_t* in, uint64_t c, uint64_t* n, uint32_t flags);
/* Decode once, then let the caller allocate the exact result: after the stream has been decoded on the device,
 * alloc(user, index, n) is called once, on the calling thread, for the n result bytes (n may be 0) and the bytes
 * are copied into what it returns; NULL from alloc → ZES_E_ARG.  The whole call holds the library's lock: there is
 * no state between calls.  index is 0 here (the batch form passes the buffer's index).
 * replaces: the growable Uint8WriteStream of src/inflate.ts:17,39 (src/utils/Uint8WriteStream.ts:1-25). */
typedef uint8_t* (*zes_alloc_fn)(void* user, uint32_t index, uint64_t n);
int zes_inflate_alloc(const uint8_t* in, uint64_t c, zes_alloc_fn alloc, void* user, uint64_t* out_len, uint32_t flags);

/* Raw DEFLATE, without the zlib wrapper, for callers that embed DEFLATE in another container.
 * zes_deflate_raw*  replaces: `export function deflate(input)` of src/deflate.ts:14-39 (what src/zlib.ts:35 wraps):
 *                   the same bytes as zes_deflate minus the 2-byte header and the 4-byte Adler-32 trailer.
 * zes_inflate_raw*  replaces: `export function inflate(input, offset = 0)` of src/inflate.ts:16-40: decodes the raw
 *                   stream that starts at byte `offset` of the c-byte buffer (bytes after the stream stay readable,
 *                   exactly as for the reference, whose zlib wrapper calls this with offset 2, src/zlib.ts:21).
 * Same statuses as the wrapped forms; there is no CM-nibble check on this path. */
int zes_deflate_raw(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len);
int zes_deflate_raw_dev(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len);
int zes_inflate_raw(const uint8_t* in, uint64_t c, uint64_t offset, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags);
int zes_inflate_raw_dev(const uint8_t* d_in, uint64_t c, uint64_t offset, uint8_t* d_out, uint64_t cap, uint64_t* out_len,
                        uint32_t flags);

/* Where a raw stream ends: zes_inflate_raw* that also report *in_used = the bytes from `offset` up to and including the
 * byte that holds the final block's last bit (behind its end-of-block code, or its last stored byte) — the count of
 * len(body) - len(zlib.decompressobj(-15).unused_data).  For containers that put DEFLATE streams back to back (gzip
 * members, ZIP entries, PDF object streams).  Statuses and results are those of zes_inflate_raw*; *in_used is set
 * on ZES_OK only.
 * replaces: nothing (src/inflate.ts:16-40 does not say where it stopped). */
int zes_inflate_raw_used(const uint8_t* in, uint64_t c, uint64_t offset, uint8_t* out, uint64_t cap, uint64_t* out_len, uint64_t* in_used,
                         uint32_t flags);
int zes_inflate_raw_used_dev(const uint8_t* d_in, uint64_t c, uint64_t offset, uint8_t* d_out, uint64_t cap, uint64_t* out_len,
                             uint64_t* in_used, uint32_t flags);

/* CRC-32 of a buffer: the checksum of gzip, zlib's crc32() and PNG (reflected polynomial 0xEDB88320, initial value and
 * final XOR 0xFFFFFFFF).  The device form reads d_in at any alignment.
 * replaces: nothing (the reference has no CRC-32). */
int zes_crc32(const uint8_t* in, uint64_t n, uint32_t* crc);
int zes_crc32_dev(const uint8_t* d_in, uint64_t n, uint32_t* crc);
/* CRC-32 of many buffers of device memory in one launch: crc[i] = the CRC-32 of d_in[off[i], off[i] + len[i]), i < count.
 * Any alignment, any length (0 gives 0), buffers may overlap; off, len and crc are host arrays.  count == 0 is ZES_OK.
 * Made for many short, unaligned buffers (the members of a BGZF file), which zes_crc32_dev would take one launch each. */
int zes_crc32_batch_dev(const uint8_t* d_in, const uint64_t* off, const uint64_t* len, uint32_t* crc, uint32_t count);

/* gzip (RFC 1952) compress: one member whose
 *   header  is exactly 1f 8b 08 00 00 00 00 00 00 ff (FLG 0, MTIME 0, XFL 0, OS 255: the output is deterministic),
 *   body    is exactly the bytes of zes_deflate_raw (the reference's stream), and
 *   trailer is the CRC-32 of the input, then ISIZE = n mod 2^32, both little-endian.
 * zes_gzip_bound: a capacity that always suffices (zes_deflate_bound(n) - 6 + 18).
 * n == 0, n == 1 and n % 131072 == 1 return ZES_E_CORRUPT before the device is touched: the body is the reference's
 * encoder, which throws on those sizes.  d_out must be 16-byte aligned, as for zes_deflate_dev.
 * replaces: nothing for the container; the body is `export function deflate(input)` of src/deflate.ts:14-39. */
int zes_gzip_bound(uint64_t n, uint64_t* cap);
int zes_gzip(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len);
int zes_gzip_dev(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len);

/* BGZF compress (the blocked gzip of bgzip / htslib): valid gzip whose members state their own size, so that htslib can
 * index the file and zes_gunzip* decodes it as one batch.  The format is fixed, so the output is deterministic:
 *   chunks   the input is cut into chunks of ZES_BGZF_CHUNK = 65280 bytes (htslib's BGZF_BLOCK_SIZE), the last one may be
 *            shorter; each chunk becomes one member, member k holding input bytes [k * 65280, ...)
 *   header   18 bytes, exactly 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 | BSIZE (LE16), BSIZE = member size - 1
 *   body     exactly the bytes of zes_deflate_raw of that chunk alone (an independent buffer: no match reaches into the
 *            next chunk) — unless that stream is longer than len + 5 bytes or the chunk is 1 byte long (the reference's
 *            encoder throws on it): then one stored block, 01 | LEN | NLEN | the chunk's bytes (BFINAL 1, BTYPE 00), len + 5
 *            bytes.  A stream of exactly len + 5 bytes is kept.  So a member has at most 65311 bytes and BSIZE fits its
 *            16 bits (the reference's encoder has no stored blocks: its output on incompressible data has no usable bound)
 *   trailer  the CRC-32 of the chunk, then ISIZE = len, both little-endian
 *   marker   behind the last member the 28-byte end-of-file marker
 *            1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00
 * Every n is valid; n == 0 gives the marker alone.
 * zes_bgzip_members: ceil(n / 65280) + 1 (the marker); zes_bgzip_bound: full chunks * 65311 + (tail ? tail + 31 : 0) + 28, a
 * capacity that always suffices and is exact for incompressible input.  Neither touches a device.
 * member_off: NULL, or a host array with room for zes_bgzip_members(n) entries that receives the byte position of every
 * member in the output, the marker's last — what BGZF virtual offsets and a .gzi index are made of.
 * The device form takes d_in and d_out at ANY alignment and writes exactly *out_len bytes and no byte behind them (the other
 * device forms write whole 16-byte groups); the caller's input is read only inside the aligned 16-byte groups that hold
 * its bytes.  The host form stages through the library's buffers as zes_gzip does.
 *   ZES_E_NOSPACE  cap is too small: *out_len = the size needed; bytes at and behind d_out + cap are untouched, what lies
 *                  below cap is unspecified
 *   ZES_E_ARG      a null pointer with n != 0, a null out_len, flag bits other than ZES_F_PIECES
 * Members are encoded in groups (1024; ZES_F_PIECES: 4 — same bytes) so that the pooled scratch stays bounded whatever n
 * is: what zes_deflate_dev pools for 128 MiB.
 * replaces: nothing (the reference has no gzip container); the bodies are `deflate` of src/deflate.ts:14-39 per chunk. */
#define ZES_BGZF_CHUNK 65280u
int zes_bgzip_members(uint64_t n, uint64_t* members);
int zes_bgzip_bound(uint64_t n, uint64_t* cap);
int zes_bgzip(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len, uint64_t* member_off, uint32_t flags);
int zes_bgzip_dev(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint64_t* member_off, uint32_t flags);

/* gzip (RFC 1952) decompress, as CPython 3.10's gzip.decompress: any number of members back to back, their outputs
 * concatenated; zero bytes between and after members are skipped.  Header: 1f 8b, CM 8; FEXTRA, FNAME and FCOMMENT are
 * skipped, FHCRC is checked against the low 16 bits of the header's CRC-32.  Each body is decoded as by
 * zes_inflate_raw_used (every tier: a reference-made body takes the block-parallel one); the 8 bytes behind it must
 * hold the CRC-32 and ISIZE of the member's output.
 *   ZES_E_GZIP      bad magic, CM != 8, reserved FLG bits 5-7 set (CPython ignores them; zlib does not), a header cut
 *                   short, c == 0 (CPython returns b""), fewer than 8 bytes behind a body, non-zero bytes behind a
 *                   member that do not start a valid member
 *   ZES_E_CHECKSUM  CRC-32 or ISIZE mismatch, or a wrong FHCRC (CPython does not check FHCRC)
 *   an error inside a body: the status zes_inflate_raw returns on those bytes
 *   ZES_E_NOSPACE   as for zes_inflate: *out_len = the size needed
 * Header errors of the host forms are decided before the device is touched.  The device form writes whole 16-byte
 * groups as zes_inflate_dev does (d_out 16-byte aligned; d_in at any alignment).  zes_gunzip_alloc: as
 * zes_inflate_alloc (one alloc call, index 0, for the exact size).
 *
 * Member-parallel reading.  A file whose members all state their own size (BGZF, the format of bgzip / htslib) is decoded
 * as one batch: its members are found without decoding, all bodies go through the inflate tiers in one call, and one
 * segmented CRC-32 launch checks all outputs.  A member qualifies when its header is 1f 8b 08 with FLG exactly 04
 * (FEXTRA only) and at most 256 bytes long, its extra field, walked subfield by subfield, ends exactly with a subfield and
 * holds a subfield 'B','C' of SLEN 2 (others before or after it are fine), and with size = BSIZE + 1: hlen + 8 <= size and
 * the member lies inside the input.  The batch is tried when members follow each other directly from byte 0 to the
 * input's last byte, every one of them qualifies and there are at least two.  It answers only with ZES_OK: when every
 * member decodes to exactly its ISIZE bytes, its stream ends in the last byte in front of its trailer and its CRC-32
 * matches.  Anything else (padding, a plain member, a BSIZE that lies, any error, a result beyond the device form's cap)
 * is decided by the member-by-member path run from the start, so results and statuses are the same either way, and the
 * allocator of zes_gunzip_alloc is still called exactly once.  ZES_F_GZIP_SERIAL forces the member-by-member path.
 * replaces: nothing (the reference has no gzip container). */
int zes_gunzip(const uint8_t* in, uint64_t c, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags);
int zes_gunzip_dev(const uint8_t* d_in, uint64_t c, uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint32_t flags);
int zes_gunzip_alloc(const uint8_t* in, uint64_t c, zes_alloc_fn alloc, void* user, uint64_t* out_len, uint32_t flags);

/* zes_gzip_batch*: many independent buffers, one gzip file each, in one call whose launches, copies and synchronisations do
 * not grow with the number of files.  File i is one member:
 *   header   zes_gzip's: 1f 8b 08 00 00 00 00 00 00 ff
 *   body     the bytes of zes_deflate_raw when the encoder accepts the length (not 0, 1 or 1 mod 131072) and that stream is
 *            shorter than the stored form; otherwise the stored form: blocks of 65535 bytes, 00 | LEN | NLEN | the bytes,
 *            BFINAL (01) on the last one; length 0 is the one block 01 00 00 ff ff.  So every length below 2^32 writes, and
 *            where the stream is kept the file is byte for byte zes_gzip's.  The same inputs give the same bytes
 *   trailer  the CRC-32 of the input, then ISIZE, both little-endian
 * in_off, in_len, out_off, out_cap, out_len and status are host arrays of `count` values.  The return value is non-zero only
 * when the call as a whole could not run; count == 0 is ZES_OK without device work.
 *   status[i]  ZES_OK: out_len[i] bytes written
 *              ZES_E_UNSUPPORTED: in_len[i] >= 2^32 (ISIZE stays exact), decided before any launch; out_len[i] = 0
 *              ZES_E_NOSPACE (device form): out_cap[i] is too small or d_out is null; the file is still encoded, out_len[i] is
 *              the size needed and nothing of it is written — a call with every capacity 0 is a sizing pass
 *              ZES_E_ARG (host form): alloc returned NULL for the file
 *   ZES_E_ARG for the whole call: a null array with count != 0, a null d_in / in[i] with a non-zero length, a null alloc,
 *              flag bits other than ZES_F_PIECES
 * zes_gzip_batch_bound: cap[i] = 18 + n + 5 * max(1, ceil(n / 65535)), exact when the file is stored and always enough (0 for
 * a length of 2^32 and more); it touches no device.
 * The device form takes d_in, d_out and every offset at ANY alignment, writes exactly out_len[i] bytes for a file at ZES_OK
 * and no byte outside the ranges [out_off[i], out_off[i] + out_cap[i]), which must not overlap, and reads the input only
 * inside the aligned 16-byte groups that hold it.  The host form calls alloc(user, i, n) once per file at ZES_OK, behind the
 * device work.  Everything runs on one context.
 * Launches: the files are encoded in groups (1024 files whose encoder slots take up to 256 MiB; ZES_F_PIECES: 4 and 1 MiB —
 * same bytes); a group costs one segmented CRC-32 launch, one batch encode with its one read-back of the sizes, and one
 * k_gz_pack launch that writes headers, bodies and trailers.  Nothing is launched per file.
 * replaces: nothing (the reference has no gzip container); the bodies are `deflate` of src/deflate.ts:14-39 per buffer. */
int zes_gzip_batch_bound(const uint64_t* in_len, uint32_t count, uint64_t* cap /* count values */);
int zes_gzip_batch_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out,
                       const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t flags);
int zes_gzip_batch(const uint8_t* const* in, const uint64_t* in_len, uint32_t count, zes_alloc_fn alloc, void* user,
                   uint64_t* out_len, int32_t* status, uint32_t flags);

/* zes_gunzip_batch*: many independent gzip files decoded in one call.  status[i], out_len[i] and the bytes are exactly what
 * zes_gunzip_dev (zes_gunzip_alloc) gives for file i alone with out_cap[i] as its capacity, for every file, good or bad: the
 * batch is a route, not a second rule.  Arrays, return value and count == 0 as for zes_gzip_batch*.
 *   1. One k_gz_heads launch (the host forms: the same rule on the caller's memory) judges every file a candidate or not; it
 *      never gives a status.  A candidate has in_len >= 18, starts 1f 8b 08, has FLG bits 5-7 and FHCRC clear, a header
 *      (FEXTRA, FNAME, FCOMMENT walked by RFC 1952) that ends within 256 bytes and at least 8 bytes before the file's end,
 *      no subfield 'B','C' of SLEN 2 that states a member size below in_len (a BGZF file keeps its member-parallel route
 *      through step 3), and an ISIZE (the file's last 4 bytes) of at most out_cap[i] (device form) and at most 1032 times
 *      the body's length (a lying trailer cannot grow the scratch).
 *   2. The candidates' bodies [hlen, in_len - 8) go as one batch: one gather, one pass through the inflate tiers, one
 *      segmented CRC-32 launch.  A candidate is done when its stream ends in the body's last byte, its output is exactly
 *      ISIZE bytes and the CRC-32 matches: zes_gunzip's checks for a single-member file.
 *   3. Every other file — no candidate, or a candidate that step 2 did not pass: two members, padding, a corrupt body, a
 *      wrong trailer — goes through zes_gunzip_dev's path, in order; that path decides its status, size and bytes.
 *      ZES_F_GZIP_SERIAL sends every file this way (testing aid, yardstick).
 * flags: ZES_F_PIECES, ZES_F_GZIP_SERIAL; others are ZES_E_ARG for the whole call, as are a null array with count != 0, a null
 * d_in / in[i] with a non-zero length, a null d_out with a non-zero capacity and a null alloc.
 * The device form takes d_in, d_out and every offset at ANY alignment, writes exactly out_len[i] bytes for a file at ZES_OK
 * and no byte outside the ranges [out_off[i], out_off[i] + out_cap[i]), which must not overlap (a file that fails may leave
 * bytes inside its own range), and reads the input only inside the aligned 16-byte groups that hold it.
 * zes_gunzip_batch_alloc verifies every file first, then calls alloc(user, i, n) once per file at ZES_OK, in order, and
 * never for a failed one; NULL from alloc is that file's ZES_E_ARG.  Everything runs on one context.
 * zes_last_gunzip_batch: how many files of this thread's last zes_gunzip_batch* call finished in step 2 and in step 3.
 * replaces: nothing (the reference has no gzip container). */
int zes_gunzip_batch_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out,
                         const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t flags);
int zes_gunzip_batch_alloc(const uint8_t* const* in, const uint64_t* in_len, uint32_t count, zes_alloc_fn alloc, void* user,
                           uint64_t* out_len, int32_t* status, uint32_t flags);
int zes_last_gunzip_batch(uint32_t* batched, uint32_t* serial);   /* files of the last batch call by route */

/* BGZF random access: the member index of a BGZF file, and reads of any range of its uncompressed data that decode only
 * the members holding that range (what htslib does with a .gzi index).
 *
 * zes_bgzf_index*: the file must be BGZF from its first byte to its last: members follow each other directly from byte 0
 * to byte c, and every one qualifies under the rule of "Member-parallel reading" above (1f 8b 08, FLG exactly 04, a header
 * of at most 256 bytes, an extra field that walks to its exact end and holds a 'B','C' subfield of SLEN 2, hlen + 8 <= size
 * <= the bytes left).  One member is enough.  On ZES_OK *members is the member count (the end-of-file marker included when
 * there is one) and members + 1 entries are written to each host array: coff[k] = member k's byte position, uoff[k] = the
 * sum of the ISIZE fields in front of it, and the closing entry coff[members] = c, uoff[members] = the uncompressed size.
 * Nothing is decoded: a wrong CRC-32 or a damaged body does not concern the index.
 *   ZES_E_GZIP     c == 0, or not such a chain to its last byte: padding, a plain member, a BSIZE that lies, a header or
 *                  trailer cut short, garbage behind the file
 *   ZES_E_NOSPACE  cap < members + 1: *members is set, nothing is written to coff or uoff (coff == uoff == NULL with
 *                  cap == 0 asks for the count)
 *   ZES_E_ARG      a null members, a null in with c != 0, flag bits other than ZES_F_INDEX_WALK, only one of coff / uoff
 *                  null, both null with cap != 0
 * The host form walks the caller's memory on the host and touches no device (it works without one, and ignores
 * ZES_F_INDEX_WALK).  The device form takes d_in at any alignment and reads only inside the aligned 16-byte groups that
 * hold its bytes: k_bgzf_mark tests every byte position for a member's first four bytes and judges each hit by the rule
 * above, and the host follows the chain from byte 0 through the list of those that qualify (at most c / 256 + 1024 of
 * them; with more, or with ZES_F_INDEX_WALK, k_gz_walk's serial chain answers — the same result by the same rule).
 *
 * zes_bgzf_read*: bytes [pos, pos + n) of the uncompressed data, n = min(len, total - pos), total = uoff[members], through
 * an index as zes_bgzf_index* writes it (coff, uoff: host arrays of members + 1 entries).  The members whose output
 * overlaps the range are found by binary search in uoff (members inside the range whose ISIZE is 0 are skipped), and only
 * their index entries are looked at: a call costs O(log members + touched).  Every touched member is decoded whole and
 * checked as the member-parallel reader checks it; members the range does not touch are never looked at.
 *   ZES_E_ARG       a null pointer, members == 0, pos > total, flag bits other than ZES_F_PIECES (passed on to the inflate
 *                   tiers)
 *   ZES_E_NOSPACE   n > cap: *out_len = n; decided from the index alone, nothing is decoded or written
 *   ZES_OK with *out_len = 0 when len == 0 or pos == total: no device work
 *   ZES_E_GZIP      a stale or foreign index: a touched member does not lie inside [0, c) with coff[k] < coff[k + 1], its
 *                   header, read again from the file, does not qualify, its size is not coff[k + 1] - coff[k], or its
 *                   ISIZE is not uoff[k + 1] - uoff[k]
 *   an error inside a touched body: the status zes_inflate_raw returns on it (the first such member in file order decides)
 *   ZES_E_CHECKSUM  a touched member's output is not ISIZE bytes long (one that would outgrow its slot included), its
 *                   stream does not end in the last byte in front of the trailer, or its CRC-32 does not match
 * The device form takes d_in and d_out at any alignment and writes exactly *out_len bytes and no byte in front of or behind
 * them, as zes_bgzip_dev does; after an error the bytes below cap are unspecified.  The host form uploads only the file
 * bytes [coff[first touched], coff[last touched + 1]) and downloads n bytes.  Scratch grows with the range (the touched
 * bodies and the outputs that cannot be decoded in place), as it does with the file for zes_gunzip_dev.
 * zes_last_gunzip_members() reports the members the call decoded.
 * replaces: nothing (the reference has no gzip container). */
int zes_bgzf_index(const uint8_t* in, uint64_t c, uint64_t* coff, uint64_t* uoff, uint64_t cap, uint64_t* members, uint32_t flags);
int zes_bgzf_index_dev(const uint8_t* d_in, uint64_t c, uint64_t* coff, uint64_t* uoff, uint64_t cap, uint64_t* members, uint32_t flags);
int zes_bgzf_read(const uint8_t* in, uint64_t c, const uint64_t* coff, const uint64_t* uoff, uint64_t members, uint64_t pos, uint64_t len,
                  uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags);
int zes_bgzf_read_dev(const uint8_t* d_in, uint64_t c, const uint64_t* coff, const uint64_t* uoff, uint64_t members, uint64_t pos, uint64_t len,
                      uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint32_t flags);

/* ZIP archives (PKWARE APPNOTE 6.3): the entry index out of the central directory, and batch extraction through it.
 * The reader takes no ZIP64, no archive over several disks, no encryption and no method other than 0 and 8
 * (ZES_E_UNSUPPORTED); the writer (zes_zipwrite*, below) makes none of them.
 *
 * zes_zip_index*: the archive's entries in directory order, from the end record and the central directory alone; local
 * headers are not looked at and nothing is decoded (as CPython's zipfile, the reader meets them when an entry is opened).
 * Method and flags are copied as they are, so an archive with a bzip2 or an encrypted entry still lists.  The rule:
 *   end record   scanning backwards from c - 22 over at most 65535 further positions, the first position p whose four bytes
 *                are 50 4b 05 06 and for which p + 22 + comment length == c.  None, or c < 22: ZES_E_ZIP.  Stricter than
 *                CPython 3.10 in one place (CPython accepts bytes behind the comment) and more lenient in another (CPython
 *                takes the last signature even when it lies inside the comment, and then fails or lists nothing)
 *   unsupported  either disk number non-zero, the two entry counts different, a count of 0xFFFF, a directory size or
 *                offset of 0xFFFFFFFF, a ZIP64 locator 50 4b 06 07 at p - 20: ZES_E_UNSUPPORTED
 *   directory    cd_size + cd_off > p: ZES_E_ZIP.  Else base = p - cd_size - cd_off is the length of whatever stands in
 *                front of the archive (a self-extractor's stub), and the directory is [base + cd_off, p)
 *   records      walked from the directory's first byte to exactly p: each starts with 50 4b 01 02, its 46 bytes plus name,
 *                extra field and comment lie inside the directory, and there are as many as the end record says; else
 *                ZES_E_ZIP.  A record's csize, usize or offset of 0xFFFFFFFF or a non-zero disk number: ZES_E_UNSUPPORTED.
 *                hdr_off = base + offset must leave room for a local header in front of the directory,
 *                hdr_off + 30 <= base + cd_off, else ZES_E_ZIP.  The first record in directory order that fails decides
 * On ZES_OK `*entries` records are written to ent and the names, back to back, to names (`*names_len` bytes in all).
 *   ZES_E_NOSPACE  cap < *entries or names_cap < *names_len: both counts are set, nothing is written.  ent == names == NULL
 *                  with both capacities 0 asks for the counts: ZES_E_NOSPACE on every valid archive
 *   ZES_E_ARG      a null entries or names_len, a null in with c != 0, any flag bit, ent or names null while its capacity
 *                  is not 0
 * The host form touches no device and works without one.  The device form takes d_in at any alignment, makes two
 * device-to-host copies — the last min(c, 65557) bytes, then the directory — and runs the same host function on them; it
 * launches no kernel.
 * replaces: nothing (the reference has no ZIP container) */
typedef struct zes_zip_entry {   /* 40 bytes, all little-endian host values */
  uint64_t hdr_off;    /* the local header's position in the file (any prefix in front of the archive already added) */
  uint64_t name_pos;   /* where the central directory's copy of the name lies in the file */
  uint32_t csize, usize, crc;
  uint32_t name_off;   /* the name inside the names blob the index call fills */
  uint16_t name_len, method, flags, pad;   /* pad 0 */
} zes_zip_entry;
int zes_zip_index(const uint8_t* in, uint64_t c, zes_zip_entry* ent, uint64_t cap, uint64_t* entries, uint8_t* names, uint64_t names_cap,
                  uint64_t* names_len, uint32_t flags);
int zes_zip_index_dev(const uint8_t* d_in, uint64_t c, zes_zip_entry* ent, uint64_t cap, uint64_t* entries, uint8_t* names, uint64_t names_cap,
                      uint64_t* names_len, uint32_t flags);

/* zes_zip_read*: `count` entries of the index `ent[0, nent)` extracted as one batch: entry sel[i], or entry i when sel is NULL
 * (then count <= nent).  Any order, duplicates included.  status[i] and out_len[i] are filled per entry (out_len[i] = usize on
 * ZES_OK, else 0); the return value is non-zero only when the call as a whole could not run.
 *   ZES_E_ARG   a null array with count != 0, a null file with c != 0, sel[i] >= nent, count > nent without sel, flag bits other
 *               than ZES_F_PIECES (passed on to the inflate tiers)
 *   count == 0  ZES_OK, no device work; zes_last_kernel_times then reports no launch and zes_last_inflate_tier 0, as after a
 *               call that decoded nothing
 * An entry's status, decided in this order:
 *   1. from the entry alone, without a launch for it: flags & 0x61 (encrypted, patched data, strong encryption) or a method
 *      other than 0 or 8: ZES_E_UNSUPPORTED; method 0 with csize != usize: ZES_E_ZIP; hdr_off + 30 > c or
 *      name_pos + name_len > c (a stale or foreign index): ZES_E_ZIP; so is an entry whose name and csize bytes cannot lie
 *      between hdr_off + 30 and c (step 2's last test, with an extra field of no bytes)
 *   2. the local header, read from the file by k_zip_stage: ZES_E_ZIP unless its signature is 50 4b 03 04, its method is the
 *      entry's, its flag bit 0 the entry's, its name length name_len, its name the name_len bytes at name_pos, and
 *      hdr_off + 30 + name_len + extra length + csize <= c.  Its own CRC and size fields are not compared (with a data
 *      descriptor, flag bit 3, they are zero)
 *   3. method 8: the body decoded as by zes_inflate_raw_used, all bodies of the call in one pass through the inflate tiers; a
 *      body that fails keeps its inflate status; ZES_E_CHECKSUM when the result is not usize bytes long, the stream does not
 *      end in the body's last byte, or the CRC-32 differs
 *   4. method 0: a copy, then the same CRC-32 check.  One segmented CRC-32 launch checks all results of both methods.
 * The device form writes entry i to d_out + out_off[i] at any alignment: exactly usize bytes for an entry that checks out, and
 * no byte outside the selected entries' ranges [out_off[i], out_off[i] + usize), which must not overlap; a failed entry's range
 * is unspecified.  d_in at any alignment; it is read only inside the aligned 16-byte groups that hold bytes of [0, c).
 * The alloc form calls alloc(user, i, usize) once per entry with ZES_OK, after it is checked (usize may be 0), never for a
 * failed one (NULL from alloc: that entry is ZES_E_ARG); it uploads only the selected entries' header, name and data bytes, not
 * the file, and runs on one context as the other single host calls do.
 * replaces: nothing (the reference has no ZIP container) */
int zes_zip_read_dev(const uint8_t* d_in, uint64_t c, const zes_zip_entry* ent, uint64_t nent, const uint32_t* sel, uint32_t count,
                     uint8_t* d_out, const uint64_t* out_off, uint64_t* out_len, int32_t* status, uint32_t flags);
int zes_zip_read_alloc(const uint8_t* in, uint64_t c, const zes_zip_entry* ent, uint64_t nent, const uint32_t* sel, uint32_t count,
                       zes_alloc_fn alloc, void* user, uint64_t* out_len, int32_t* status, uint32_t flags);

/* zes_zipwrite*: a ZIP archive of `count` entries, entry i the in_len[i] bytes at d_in + in_off[i] (in[i], host form) under the
 * name of name_len[i] bytes that stands in `names` behind the names before it.  in_off, in_len, name_len and names are host
 * memory; the entries' bytes may overlap and repeat; duplicate and empty names are the caller's business.  The result is
 * deterministic, the same inputs give the same bytes:
 *   local header  50 4b 03 04, version needed 20, flags 0x0800 when the name holds a byte >= 0x80 (names are taken as UTF-8,
 *                 CPython's rule) else 0, method, time 0, date 33 (1980-01-01), CRC-32, csize, usize, name length, extra
 *                 length 0; then the name, then the body.  No data descriptor, no extra field, no bytes between entries
 *   method        let s be zes_deflate_raw of the entry's bytes alone.  Method 8 with body s when the encoder accepts the
 *                 length (not 0, not 1, not = 1 mod 131072) and s is shorter than the entry; otherwise method 0 with the
 *                 bytes themselves as the body (a stream of exactly in_len[i] bytes is not kept)
 *   directory     in entry order, 46 bytes and the name each: 50 4b 01 02, made-by 20, needed 20, the local header's flags,
 *                 method, time, date, CRC and sizes, name length, extra, comment, disk and both attribute fields 0, the
 *                 local header's offset
 *   end record    50 4b 05 06, disks 0, both counts, the directory's size and offset, comment length 0.  count == 0 gives
 *                 the end record alone: 22 bytes
 * zes_zipwrite_bound: sum(30 + name + len) + sum(46 + name) + 22 — exact when every entry is stored, and always enough, as
 * method 8 is chosen only when it is shorter.  It touches no device.
 * ent: NULL, or room for `count` records, which on ZES_OK are what zes_zip_index lists for the result (name_off: the running
 * sum of name_len).  Statuses, for the whole call:
 *   ZES_E_ARG          a null array with count != 0, a null out_len, a null d_out / out with cap != 0, a null d_in / in[i]
 *                      with a non-zero length, flag bits other than ZES_F_PIECES
 *   ZES_E_UNSUPPORTED  from the arguments alone, before any device work and before a byte of the data is read: count > 65534,
 *                      an in_len[i] > 0xFFFFFFFE; once known: a local header's offset, the directory's offset or its size
 *                      reaches 0xFFFFFFFF (no ZIP64 is written)
 *   ZES_E_NOSPACE      the result does not fit cap (or d_out is NULL with cap 0: a size query): *out_len = the size needed;
 *                      every entry is still encoded, as for zes_bgzip*, and nothing at or behind cap is touched
 * The entries go in groups, in order: up to 1024 of them whose encoder slots take up to 256 MiB (4 of them and 1 MiB under
 * ZES_F_PIECES, a testing aid for both seams: same bytes), and one entry at least.  An entry's slot is zes_deflate_bound of its
 * length, about twice the length, so the scratch is bounded by the larger of 256 MiB of slots and the longest entry's slot
 * (about 8 GiB for an entry of 4 GiB), with the encoder's per-block tables for as many blocks, however many entries the
 * archive holds.  Per group one
 * segmented CRC-32 launch, one batch encode, one read-back of the sizes and one k_zip_pack launch that writes headers, names
 * and bodies; the directory and the end record are made on the host and go up in one copy.  No launch, copy or
 * synchronisation per entry.
 * The device form takes d_in, every in_off and d_out at any alignment, writes exactly *out_len bytes and no byte in front of or
 * behind them, and reads the input only inside the aligned 16-byte groups that hold its bytes (zes_bgzip_dev's contract).
 * The host form stages the entries (one upload per entry: "nothing per entry" is the device form's), downloads the result
 * once and runs on one context as the other single host calls do;
 * count == 0 is answered without a device.
 * replaces: nothing (the reference has no ZIP container) */
int zes_zipwrite_bound(const uint64_t* in_len, const uint16_t* name_len, uint32_t count, uint64_t* cap);
int zes_zipwrite_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, const uint8_t* names, const uint16_t* name_len,
                     uint32_t count, uint8_t* d_out, uint64_t cap, uint64_t* out_len, zes_zip_entry* ent, uint32_t flags);
int zes_zipwrite(const uint8_t* const* in, const uint64_t* in_len, const uint8_t* names, const uint16_t* name_len, uint32_t count,
                 uint8_t* out, uint64_t cap, uint64_t* out_len, zes_zip_entry* ent, uint32_t flags);

/* PNG images (PNG specification, second edition): the header of a file, and batch decoding of files to their scanlines.
 * The reader undoes the container, the zlib stream and the scanline filters and nothing else: samples stay as stored (16-bit
 * big-endian, sub-byte samples packed, palette indices as indices).  Adam7 interlace is refused without ZES_F_PNG_INTERLACED ("Interlaced images" below); no APNG.  The writer, zes_pngwrite* below, is the same in reverse.
 *
 * zes_png_info: what a decode call works from.  All values are little-endian host values; pad fields are 0.
 * The file rule.  A file in[0, c) is judged chunk by chunk from byte 8; the first failure in file order decides:
 *   signature   c >= 8 and the bytes are 89 50 4e 47 0d 0a 1a 0a, else ZES_E_PNG
 *   chunk chain chunks start at byte 8: a big-endian length L <= 0x7fffffff, four type bytes that are all ASCII letters, L data
 *               bytes and 4 CRC bytes, all inside [0, c); the chain must reach an IEND; else ZES_E_PNG
 *   IHDR        the first chunk, L == 13; width and height in 1 .. 2^31 - 1; (colour, depth) one of 0:{1,2,4,8,16}, 2:{8,16},
 *               3:{1,2,4,8}, 4:{8,16}, 6:{8,16}; compression 0, filter 0, interlace 0 or 1; a second IHDR; else ZES_E_PNG
 *   IDAT        at least one (decided at IEND), all of them consecutive; colour type 3 needs a PLTE in front of the first
 *               one (decided there); else ZES_E_PNG
 *   PLTE        at most once, in front of the IDATs, L % 3 == 0 and 3 <= L <= 768, else ZES_E_PNG
 *   IEND        L == 0 and its CRC field ends exactly at byte c, else ZES_E_PNG; the walk ends here
 *   others      any other chunk whose type starts with an upper-case letter (a critical chunk): ZES_E_UNSUPPORTED; ancillary
 *               chunks are passed over (tRNS is noted when it stands in front of the first IDAT: the first such one)
 *   size        behind a sound chain: the filtered size F = height * (1 + rowbytes) > 0xFFFFFFFF is ZES_E_UNSUPPORTED
 * zes_png_info_get applies the rule to the caller's memory on the host and touches no device, so it checks no CRC.  It
 * answers ZES_OK for an interlaced file and reports the method (as zes_zip_index lists entries it cannot extract); the
 * decode calls answer ZES_E_UNSUPPORTED for one unless ZES_F_PNG_INTERLACED is set.  With a status the record is all zeros.  ZES_E_ARG: a null info, a null in
 * with c != 0, any flag bit.
 * replaces: nothing (the reference has no PNG container) */
typedef struct zes_png_info {   /* 72 bytes */
  uint32_t width, height;
  uint8_t depth, colour, interlace, channels;   /* channels: 1, 2, 3 or 4 samples a pixel (a palette index is one) */
  uint8_t bpp;          /* the filter unit: max(1, channels * depth / 8) */
  uint8_t pad[3];
  uint64_t rowbytes;    /* ceil(width * channels * depth / 8) */
  uint64_t out_size;    /* height * rowbytes */
  uint32_t idat_count;  /* IDAT chunks ... */
  uint32_t plte_len;    /* PLTE's data bytes (0: none) */
  uint64_t idat_bytes;  /* ... and their data bytes in all: the zlib stream */
  uint64_t plte_pos;    /* PLTE's data in the file (0: none) */
  uint64_t trns_pos;    /* the data of a tRNS in front of the first IDAT (0: none) ... */
  uint32_t trns_len;    /* ... and its length */
  uint32_t pad2;
} zes_png_info;
int zes_png_info_get(const uint8_t* in, uint64_t c, zes_png_info* info, uint32_t flags);

/* zes_png_decode*: `count` files decoded as one batch, file i the in_len[i] bytes at d_in + in_off[i] (in[i], alloc form).
 * status[i] and out_len[i] are filled per image (out_len[i] = out_size on ZES_OK and on ZES_E_NOSPACE, else 0), and info[i]
 * when info is not NULL (zeros for a file the rule rejects); the return value is non-zero only when the call as a whole could
 * not run.  in_off, in_len, out_off, out_cap, out_len, status and info are host arrays.
 *   ZES_E_ARG   a null array with count != 0, a null d_in / in[i] with a non-zero length, a null d_out while an image has
 *               bytes to write, flag bits other than ZES_F_PIECES (passed on to the inflate tiers) and ZES_F_PNG_INTERLACED
 *   count == 0  ZES_OK, no device work; zes_last_kernel_times then reports no launch and zes_last_inflate_tier 0
 * An image's status, decided in this order; an image with a status costs no later launch for itself:
 *   1. the file rule above (device form: k_png_walk, one lane a file, which also lists every chunk; alloc form: the host's
 *      function), then interlace 1: ZES_E_UNSUPPORTED (without ZES_F_PNG_INTERLACED; with it: "Interlaced images"), then (device form) out_cap[i] < out_size: ZES_E_NOSPACE.  A call whose
 *      capacities are all 0 is the sizing pass and costs the walk alone.
 *   2. chunk CRCs: one segmented CRC-32 launch over type and data of every chunk of every image still at ZES_OK; any
 *      mismatch, ancillary chunks included, is ZES_E_CHECKSUM
 *   3. the IDAT payloads gathered into one zlib stream an image (one segmented copy for the batch), all streams decoded in one
 *      pass through the inflate tiers into scratch slots of F bytes, their Adler-32 trailers checked by one segmented
 *      launch.  A stream that fails keeps its inflate status; a result that is not exactly F bytes, one that would outgrow
 *      its slot included, is ZES_E_PNG; a wrong or missing Adler-32 is ZES_E_CHECKSUM; bytes behind the trailer inside the
 *      IDATs are ignored
 *   4. one k_png_unfilter launch for the batch writes the scanlines without their filter bytes.  A filter byte above 4 makes
 *      the image ZES_E_PNG
 * The device form writes image i to d_out + out_off[i] at any alignment: exactly out_size bytes for an image that checks out,
 * and no byte outside the ranges [out_off[i], out_off[i] + out_size) of the images that reach step 4, which must not overlap;
 * a failed image's range is unspecified (zes_zip_read_dev's contract).  d_in and every in_off may have any alignment.  The
 * walk is launched at most twice (a file with more chunks than its share of the chunk table, 16 + in_len / 4096, makes it run
 * once more with the exact sizes); there is no launch, copy or synchronisation per image.
 * The alloc form walks the caller's memory with the host function, uploads the files that pass, runs the same steps on one
 * context and calls alloc(user, i, out_size) once per image that checks out, never for one that fails (NULL from alloc: that
 * image is ZES_E_ARG).
 * Scratch grows with the batch, as it does for zes_zip_read_dev: the gathered streams, a slot of F bytes an image, the chunk
 * table; the alloc form also holds the files and the results.
 * Known limit: the filters of Up, Average and Paeth rows depend on the row above, so an image is unfiltered by one wave from
 * each row of filter None or Sub that starts a band of 64 rows (and from row 0) to the next such row.  An image without such
 * rows is unfiltered by a single wave: the design point is a batch of images, not one large image.
 *
 * Interlaced images.  With ZES_F_PNG_INTERLACED in flags (zes_png_decode_dev, zes_png_decode_alloc, zes_pngpix_dev and
 * zes_pngpix_alloc take it, alone or with ZES_F_PIECES; no other call does) a file of interlace method 1 (Adam7) is decoded
 * too; without the flag, and for every file of interlace method 0 with it, statuses, bytes and launches are what they are
 * above.  Pass p = 1..7 of a width x height image holds the pixels (x0 + k * dx, y0 + m * dy):
 *            pass   1  2  3  4  5  6  7
 *            x0     0  4  0  2  0  1  0
 *            y0     0  0  4  0  2  0  1
 *            dx     8  8  4  4  2  2  1
 *            dy     8  8  8  4  4  2  2
 * It has pw = ceil((width - x0) / dx) pixels a row and ph = ceil((height - y0) / dy) rows, each 0 when the difference is not
 * positive.  A pass with pw == 0 or ph == 0 has no byte in the stream, not even filter bytes; any other one has ph rows of
 * 1 + ceil(pw * channels * depth / 8) bytes, filtered as an image of its own: the row above its row 0 is zeros, the filter
 * unit is the image's bpp.  The passes stand back to back; Fi, the interlaced filtered size, is the sum of their bytes.  The
 * steps above apply with these differences:
 *   1. Fi > 0xFFFFFFFF (computed in 64 bits: Fi can exceed the F of the file rule) is ZES_E_UNSUPPORTED, in the alloc forms on
 *      the host as the rule is.  out_size, out_len and zes_png_info are unchanged: the result is height * rowbytes bytes (the
 *      pixel forms: width * height * 4)
 *   3. the stream must inflate to exactly Fi bytes, else ZES_E_PNG
 *   4. the same single k_png_unfilter launch, an interlaced image's passes being up to seven images of it, unfiltered into
 *      pooled scratch; a filter byte above 4 in any pass makes the image ZES_E_PNG
 *   4b. one k_png_deinterlace launch for the batch, only when an interlaced image is still at ZES_OK (the tiles of an
 *      interlaced image that step 4 made ZES_E_PNG are then part of that launch and exit at once, writing nothing: the
 *      launch is the batch's, and its table went up before step 4), gathers the passes into
 *      the scanlines exactly as a non-interlaced file of the same pixels decodes: 16-bit samples big-endian, sub-byte samples
 *      packed from the high bits, palette indices as indices.  The pad bits behind a row's last pixel (depths below 8) are
 *      zeros: the pad bits of the pass rows in the file may hold anything and do not reach the output
 * The contracts above stay: no launch, copy or synchronisation per image or per pass; exactly out_size bytes an image, no byte
 * outside the ranges of the images that reach the last step, at any alignment.  Scratch grows by a slot for the unfiltered
 * passes of every interlaced image.  Writing interlaced files is out of scope (zes_pngwrite* writes interlace 0).
 * replaces: nothing (the reference has no PNG container) */
int zes_png_decode_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out,
                       const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, zes_png_info* info, uint32_t flags);
int zes_png_decode_alloc(const uint8_t* const* in, const uint64_t* in_len, uint32_t count, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                         int32_t* status, zes_png_info* info, uint32_t flags);

/* zes_pngwrite*: `count` images written as one batch, each to a PNG file of its own.  Image i is in_len[i] bytes of scanlines
 * at d_in + in_off[i] (in[i], alloc form), exactly as zes_png_decode* writes them: no filter bytes, 16-bit samples big-endian,
 * sub-byte samples packed, palette indices as indices; img[i] says what they are.  aux is host memory: image i's PLTE data,
 * then its tRNS data, behind those of the images before it (as `names` in zes_zipwrite*).  img, in_off, in_len, out_off,
 * out_cap, out_len and status are host arrays; the return value is non-zero only when the call as a whole could not run.
 * The file is deterministic, the same inputs give the same bytes: signature; IHDR with compression 0, filter method 0,
 * interlace 0; PLTE when plte_len != 0; tRNS when trns_len != 0; IDAT chunks of exactly 65536 data bytes, the last one
 * shorter and never empty; IEND; nothing else.
 *   zlib stream  over the F = height * (1 + rowbytes) filtered bytes.  It is what zes_deflate gives for them when the encoder
 *                accepts the length (not = 1 mod 131072; F >= 2 always) and that stream is shorter than the stored form;
 *                otherwise the stored form: 78 01, stored blocks of 65535 bytes, the last one shorter and final, the Adler-32
 *   filter       0..4: that filter type on every row.  6: adaptive, every row takes the type whose filtered bytes have the
 *                smallest sum of min(x, 256 - x) (libpng's heuristic; the sum exact in 64 bits, a tie to the lowest type
 *                number, the row above row 0 zeros).  5: as 6, but a row r with r % 64 == 0 chooses between None and Sub only,
 *                so that every band of zes_png_decode*'s unfilter step starts at a restart row and the bands of the file
 *                decode in parallel.  Under 5 and 6 an image of colour type 3 or of a depth below 8 takes None on every row
 * An image's status, decided in this order; an image with a status from step 1 or 2 costs no launch and has out_len[i] = 0:
 *   1. ZES_E_ARG: a (colour, depth) pair outside the reader's table; width or height outside 1 .. 2^31 - 1; filter > 6; a
 *      non-zero pad; in_len[i] != height * rowbytes; colour 3 with plte_len not a multiple of 3 in 3 .. 3 << depth;
 *      plte_len != 0 for colour 0 or 4 (for colour 2 or 6: not a multiple of 3, or above 768); trns_len other than 0 or 2 for colour 0,
 *      other than 0 or 6 for colour 2, not within 0 .. plte_len / 3 for colour 3, not 0 for colour 4 or 6
 *   2. ZES_E_UNSUPPORTED: F > 0xFFFFFFFF
 *   3. ZES_E_NOSPACE: the file does not fit out_cap[i], or d_out is NULL; out_len[i] is the size needed, the image is still
 *      encoded and nothing of it is written
 * For the whole call, ZES_E_ARG: a null array with count != 0, a null d_in / in[i] with a non-zero length, a null aux with
 * PLTE or tRNS bytes to read, a null alloc, flag bits other than ZES_F_PIECES.  count == 0, and a batch in which no image
 * passes steps 1 and 2, are ZES_OK without device work.
 * zes_pngwrite_bound: cap[i] = the size of image i's file with the stored stream — exact when the image goes stored, and
 * always enough — and 0 for an image that step 1 or 2 rejects (in_len taken as height * rowbytes).  It touches no device.
 * The images go in groups, in order, as zes_zipwrite*'s entries do: up to 1024 of them whose encoder slots take up to 256 MiB
 * (4 and 1 MiB under ZES_F_PIECES: same bytes), one image at least; the scratch (a filtered buffer and an encoder slot an
 * image) is bounded by the group.  Launches per group:
 *   k_png_filter  once: the filters chosen and applied, every row of every image of the group
 *   the encoder   one batch encode over the filtered buffers (no CRC-32 launch over them); its read-back of the sizes is the
 *                 group's one read-back
 *   k_adler_seg   once, only in a group with lengths the encoder refuses: their Adler-32s, which the host finishes (so a group
 *                 with such an image has this second read-back, and a group of nothing else this one alone)
 *   k_png_pack    once: signature, IHDR / PLTE / tRNS, IDAT lengths and types, stream bytes or the stored form, IEND
 *   k_crc32_seg   once: type and data of every chunk as they lie in the output, the sums left on the device
 *   k_crc32_put   once: the chunk CRCs finished and stored
 * (the last three only when an image of the group is written; aux goes up once per group).  No launch, copy or
 * synchronisation per image.
 * The device form takes d_in, every in_off, d_out and every out_off at any alignment, writes exactly out_len[i] bytes for an
 * image at ZES_OK and no byte outside the ranges of the images that are written, and reads the input only inside the aligned
 * 16-byte groups that hold it (zes_png_decode_dev's contract).  The alloc form stages the inputs (one upload per image), runs
 * the same steps with the bound's room per image and calls alloc(user, i, out_len[i]) once per image that succeeds (NULL from
 * alloc: that image is ZES_E_ARG).
 * replaces: nothing (the reference has no PNG container) */
typedef struct zes_pngw_image {  /* 16 bytes */
  uint32_t width, height;
  uint8_t depth, colour, filter, pad;   /* pad 0 */
  uint16_t plte_len, trns_len;          /* bytes of PLTE / tRNS data in `aux` */
} zes_pngw_image;
int zes_pngwrite_bound(const zes_pngw_image* img, uint32_t count, uint64_t* cap /* count values */);
int zes_pngwrite_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, const zes_pngw_image* img, const uint8_t* aux,
                     uint32_t count, uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                     uint32_t flags);
int zes_pngwrite(const uint8_t* const* in, const uint64_t* in_len, const zes_pngw_image* img, const uint8_t* aux, uint32_t count,
                 zes_alloc_fn alloc, void* user, uint64_t* out_len, int32_t* status, uint32_t flags);

/* zes_pngpix*: PNG files decoded to pixels, width * height * 4 bytes of R, G, B, A an image, row by row from the top, as one
 * batch on the device: what a texture or an image tensor takes.  Adam7 interlace is refused without ZES_F_PNG_INTERLACED;
 * no gamma, no colour management, no output format other than 8-bit RGBA.
 * The conversion rule.  A stored sample s of depth d becomes 8 bits: d = 1: s * 255; 2: s * 85; 4: s * 17; 8: s; 16: s >> 8
 * (the high byte: libpng's strip_16).  Per colour type:
 *   0 (grey)        R = G = B = the 8-bit grey, A = 255.  With a tRNS of 2 bytes, A = 0 exactly where the stored sample, at its
 *                   full depth before the reduction, equals the big-endian key (all 16 bits of it: a key above the depth's
 *                   range matches nothing)
 *   2 (RGB)         R, G, B reduced, A = 255.  With a tRNS of 6 bytes, A = 0 where all three stored samples equal the three
 *                   keys at full depth (all 16 bits at depth 16)
 *   3 (palette)     index i gives PLTE entry i; A = tRNS[i] for i < trns_len, else 255.  An index at or beyond plte_len / 3
 *                   gives (0, 0, 0, 255), as PIL and browsers do: decided here so that a pixel needs no status and the call no
 *                   read-back for one
 *   4 (grey, alpha) the grey replicated, A the alpha sample reduced
 *   6 (RGBA)        all four samples reduced; at depth 8 a copy
 * A tRNS whose length does not fit the colour type — other than 2 for colour 0, other than 6 for colour 2, above
 * plte_len / 3 for colour 3, any for colours 4 and 6 — is ignored as if the file had none: the file rule lets such files
 * through, and these calls do not refuse them.
 *
 * zes_pngpix_dev / zes_pngpix_alloc take the arguments of zes_png_decode_dev / zes_png_decode_alloc, fill the same
 * zes_png_info, and answer the same statuses from the same steps 1 to 4 in the same order (flags: ZES_F_PIECES and ZES_F_PNG_INTERLACED only),
 * with these differences:
 *   size    the size of image i is width * height * 4: what out_len[i] reports (on ZES_OK and ZES_E_NOSPACE), what out_cap[i]
 *           is compared with and what alloc is asked for.  A call whose capacities are all 0 is the sizing pass and costs the
 *           walk alone
 *   step 4  writes the unfiltered scanlines into pooled scratch, a 16-byte aligned and padded slot an image (zes_trim,
 *           zes_pool_bytes and zes_stage_poison cover it), not into the caller's memory; step 4b (ZES_F_PNG_INTERLACED) writes
 *           an interlaced image's scanlines into the same kind of slot, and step 5 runs over plain and deinterlaced images
 *           together
 *   step 5  one k_png_expand launch for the batch writes the pixels of the images still at ZES_OK.  PLTE and tRNS are read on
 *           the device from the file bytes at plte_pos / trns_pos, at any alignment (step 2 has checked their CRCs)
 * An image with a status costs no later launch for itself; there is no launch, copy or synchronisation per image.  A call
 * over one file launches the kernels that a call over many files of the same kind launches (in step 3 the block-parallel
 * tier follows a single stream's block chain with its chain kernel as it follows a batch's, where the decode calls let
 * the host follow it).
 * The device form writes image i to d_out + out_off[i] at any alignment: exactly width * height * 4 bytes for an image at
 * ZES_OK and no byte outside the ranges of the images that reach step 5, which must not overlap.  Stores are 16 bytes wide
 * from the first 16-byte boundary of a row's output, whole pixels in front of it and at the row's end; an output that is
 * not 4-byte aligned is stored byte by byte (slower, the same bytes).
 *
 * zes_pngpix_expand_dev is step 5 alone, over scanlines that lie in device memory already (kept from zes_png_decode_dev,
 * say): image i is in_len[i] bytes at d_in + in_off[i], described by img[i] and the aux bytes exactly as zes_pngwrite_dev
 * takes them; the filter field is ignored.  Statuses:
 *   per image   ZES_E_ARG and ZES_E_UNSUPPORTED by steps 1 and 2 of zes_pngwrite* (one check serves both), out_len[i] = 0;
 *               ZES_E_NOSPACE when out_cap[i] < width * height * 4 or d_out is NULL, out_len[i] the size needed
 *   whole call  ZES_E_ARG as for zes_pngwrite_dev (flag bits other than ZES_F_PIECES, which changes nothing here)
 *   count == 0, and a batch with nothing to write, are ZES_OK without device work
 * It costs one upload (the job table and the aux bytes of the images that are written) and one launch, and reads nothing
 * back: a status can only come from the host's checks.  d_in, d_out and every offset may have any alignment; exactly
 * width * height * 4 bytes are written for an image at ZES_OK and none outside those ranges; the input is read only inside
 * the aligned 16-byte groups that hold it (zes_pngwrite_dev's rule for its input).
 * replaces: nothing (the reference has no PNG container) */
int zes_pngpix_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out,
                   const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, zes_png_info* info, uint32_t flags);
int zes_pngpix_alloc(const uint8_t* const* in, const uint64_t* in_len, uint32_t count, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                     int32_t* status, zes_png_info* info, uint32_t flags);
int zes_pngpix_expand_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, const zes_pngw_image* img, const uint8_t* aux,
                          uint32_t count, uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                          uint32_t flags);

/* TIFF images (TIFF 6.0; Compression 8 and 32946 of TIFF Technical Note 2): the index of one image of a file, and a rectangle
 * of that image decoded as one batch (zes_tiffwrite*, below, is the other direction).  The tiles or strips of an image ("segments")
 * are independent zlib streams that state their own sizes, as BGZF members are, and Predictor 2 chains within a row, never
 * across rows: every row of every segment is independent work, and a rectangle needs only the segments it touches.
 *
 * zes_tiff_image: what a read call works from.  All values are little-endian host values; there are no pad fields.
 * The file rule (one host function, used by both index forms), the first failure in this order deciding; all arithmetic in
 * 64 bits:
 *   header      c >= 8 and the bytes are 49 49 2a 00 or 4d 4d 00 2a, else ZES_E_TIFF; 49 49 2b 00 / 4d 4d 00 2b (BigTIFF):
 *               ZES_E_UNSUPPORTED
 *   chain       every directory lies at an offset o >= 8 with o + 2 + 12 n + 4 <= c (n its entry count), else ZES_E_TIFF; more
 *               than 65536 hops: ZES_E_TIFF; the chain ends at a next-offset of 0.  *dirs = the chain's length; dir >= *dirs:
 *               ZES_E_ARG (with *dirs filled)
 *   entries     of directory `dir`, in file order, need not be sorted; the first occurrence of a tag counts.  A tag the reader
 *               uses (256-259, 262, 266, 273, 277-279, 284, 317, 322-325, 338, 339) must be SHORT (3) or LONG (4) with a count
 *               >= 1, its values inline when count * size <= 4, else at an offset with offset + count * size <= c; else
 *               ZES_E_TIFF.  Other tags are not looked at
 *   geometry    ImageWidth and ImageLength present and >= 1; either StripOffsets and StripByteCounts (RowsPerStrip >= 1 when
 *               present), or TileWidth, TileLength, TileOffsets and TileByteCounts (both dimensions non-zero multiples of 16);
 *               both kinds, neither, or a missing partner: ZES_E_TIFF.  Both arrays hold exactly across * down values and every
 *               segment has off + len <= c, else ZES_E_TIFF
 *   defaults    SamplesPerPixel 1, Compression 1, Predictor 1, PlanarConfiguration 1, FillOrder 1, SampleFormat 1,
 *               RowsPerStrip the height, BitsPerSample one value of 1 (a bilevel file: unsupported below); Photometric and
 *               ExtraSamples are reported as 0 when absent
 *   kinds       SamplesPerPixel 0 or a BitsPerSample count != SamplesPerPixel: ZES_E_TIFF.  Then ZES_E_UNSUPPORTED for: unequal
 *               bit depths or one outside {8, 16, 32}; more than 4 samples; PlanarConfiguration other than 1 with more than one
 *               sample; FillOrder other than 1; Compression other than 1 (none), 8 and 32946 (both zlib); Predictor 3;
 *               Predictor 2 with Compression 1 (libtiff ignores the tag there, other readers apply it: the file is ambiguous);
 *               a segment of more than 0xFFFFFFFF decoded bytes; more than 2^31 - 1 segments.  A Predictor other than 1, 2 and
 *               3: ZES_E_TIFF
 * With any status but ZES_E_NOSPACE the record is all zeros.  compression, predictor, photometric, sample_format (its first
 * value) and extra_samples (its first value) are reported; the last three are not interpreted: palette, colour and orientation
 * are the caller's.
 *
 * zes_tiff_index applies the rule to the caller's memory on the host and touches no device.  seg_off and seg_len receive the
 * across * down file positions and byte counts, row-major in segment order; *segments = across * down.  cap < *segments:
 * ZES_E_NOSPACE with *segments, *dirs and *img filled (cap == 0 is the sizing call; seg_off and seg_len may be null then).
 * ZES_E_ARG: a null img, segments or dirs, a null `in` with c != 0, null arrays with cap != 0, flags != 0.
 * zes_tiff_index_dev is the same for a file in device memory: it brings down the 8 header bytes, of every directory on the
 * chain its count and its next-offset, the entries of directory `dir`, the values that do not lie inline in their entries
 * (the two arrays; BitsPerSample and SampleFormat of an image of 3 or 4 samples; in a file that gives another tag the reader
 * uses more than 4 bytes of values, the first of them) - never pixel data - and judges them with the same host function: at
 * most 1 + 2 * dirs + 1 + 16 copies (1 + 2 * dirs + 1 + 4 for a file whose scalar tags have one value), each followed by a
 * synchronisation.
 *
 * zes_tiff_read_dev / zes_tiff_read_alloc decode the rectangle rect = {x, y, w, h} of the image (NULL: the whole image) to
 * h rows of w * spp * bits / 8 bytes, dense, row by row from the top.  Samples of 16 and 32 bits are written little-endian
 * whatever the file's byte order, so that a view of the result as int16 or float32 works.  Decided in this order:
 *   1. ZES_E_ARG: null arrays, a null d_in / in with c != 0, a record the rule could not have produced (across, down and
 *      out_size are computed again from the other fields), an empty rectangle or one that leaves the image, flag bits other
 *      than ZES_F_PIECES (passed on to the inflate tiers), a segment with off + len > c.  Then (device form) cap below the
 *      rectangle's size: ZES_E_NOSPACE with *out_len set; a null d_out: ZES_E_ARG
 *   2. the segments the rectangle touches are chosen on the host.  A segment's decoded size E is seg_w * seg_h * spp * bits / 8
 *      for a tile (a tile is always whole: edge tiles are padded) and rows * width * spp * bits / 8 for a strip of `rows` rows
 *   3. Compression 1: seg_len < E is the segment's ZES_E_TIFF, bytes beyond E are ignored.  The bytes are read where they
 *      lie in the file: no copy is made
 *   4. Compression 8 and 32946: the touched segments are decoded as one batch into pooled scratch (the tiers of
 *      zes_inflate_batch_dev).  A stream keeps its inflate status; a result that is not exactly E bytes, one that would
 *      outgrow its slot included, is ZES_E_TIFF; the Adler-32 is always checked (one segmented launch): a wrong or missing one
 *      is ZES_E_CHECKSUM
 *   5. one k_tiff_place launch for the call, the only thing that writes d_out: Predictor 2 undone (within every segment row,
 *      from the segment's column 0 on, sample k becomes the sum of samples k, k - spp, k - 2 spp, ... modulo 2^bits; the
 *      samples of a big-endian file are swapped first), the samples made little-endian, tile padding and everything outside the
 *      rectangle dropped, every row put at its place at the rectangle's pitch.  The segments that failed are not part of it
 * The call returns ZES_OK when every touched segment is ZES_OK, else the status of the first failing one in segment order; the
 * pixels of the good segments are still written (device form), a failed segment's pixels are unspecified, and no byte outside
 * [d_out, d_out + the rectangle's size) is ever written, at any alignment of d_out.  seg_status (may be null): across * down
 * values, ZES_OK for a segment that was decoded or not touched, else its status.  There is no launch, copy or synchronisation
 * per segment.  *out_len = the rectangle's size (0 with ZES_E_ARG).  The kernels may read the aligned 16-byte groups that
 * hold a segment.
 * zes_tiff_read_alloc is the host form: it indexes directory `dir` on the host (the rule's statuses first, with *img zeros),
 * uploads only the segments the rectangle touches, runs steps 3 to 5 and, when the call is ZES_OK, calls alloc(user, 0, size)
 * once and brings the pixels down (a null answer: ZES_E_ARG).  img may be null.
 * zes_last_tiff_read: the touched segments of this thread's last zes_tiff_read_* call and the bytes that call uploaded (0 for
 * the device form): what a test of "only the touched segments go up" reads.
 * replaces: nothing (the reference has no TIFF container) */
typedef struct zes_tiff_image {  /* 48 bytes */
  uint32_t width, height;
  uint32_t seg_w, seg_h;   /* tile width and length; strips: width, and RowsPerStrip clamped to height */
  uint32_t across, down;   /* segments per row and per column */
  uint16_t bits;           /* 8, 16 or 32 */
  uint16_t spp;            /* 1..4 */
  uint16_t compression, predictor, photometric, sample_format, extra_samples;
  uint8_t big_endian, tiled;
  uint64_t out_size;       /* width * height * spp * bits / 8 */
} zes_tiff_image;
typedef struct zes_tiff_rect {
  uint32_t x, y, w, h;
} zes_tiff_rect;
int zes_tiff_index(const uint8_t* in, uint64_t c, uint32_t dir, zes_tiff_image* img, uint64_t* seg_off, uint64_t* seg_len, uint64_t cap,
                   uint64_t* segments, uint32_t* dirs, uint32_t flags);
int zes_tiff_index_dev(const uint8_t* d_in, uint64_t c, uint32_t dir, zes_tiff_image* img, uint64_t* seg_off, uint64_t* seg_len, uint64_t cap,
                       uint64_t* segments, uint32_t* dirs, uint32_t flags);
int zes_tiff_read_dev(const uint8_t* d_in, uint64_t c, const zes_tiff_image* img, const uint64_t* seg_off, const uint64_t* seg_len,
                      const zes_tiff_rect* rect, uint8_t* d_out, uint64_t cap, uint64_t* out_len, int32_t* seg_status, uint32_t flags);
int zes_tiff_read_alloc(const uint8_t* in, uint64_t c, uint32_t dir, const zes_tiff_rect* rect, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                        zes_tiff_image* img, uint32_t flags);
int zes_last_tiff_read(uint32_t* segments, uint64_t* bytes_up);

/* zes_tiffwrite*: one image written to one classic TIFF file with one directory, its tiles or strips encoded as one batch.
 * The input is what zes_tiff_read_* writes for the whole image: height rows of width * spp * bits / 8 bytes, dense, row by row
 * from the top, samples of 16 and 32 bits little-endian whatever byte order the file gets.  The record is the reader's own
 * zes_tiff_image, so index -> read -> write round-trips: a record that zes_tiff_index produced for a file this writer accepts
 * writes a file whose index is that record again.
 * The file, byte for byte (the same input gives the same bytes):
 *   header      8 bytes: 49 49 2a 00 or 4d 4d 00 2a by big_endian, and the directory's offset
 *   segments    from offset 8 on in row-major segment order, each at an even offset: one zero pad byte follows a segment of
 *               odd length.  A segment's decoded bytes: a tile is always whole, columns right of the image and rows below it
 *               are zeros; a strip holds min(seg_h, height - y0) rows of the image's width.  Under Predictor 2 every sample
 *               from the segment's second pixel on has the sample spp places before it subtracted, modulo 2^bits, from the
 *               segment's column 0 through the pad pixels too, on host-order values; the samples are then put in the file's
 *               byte order.  Compression 1: those bytes as they are.  Compression 8 and 32946: what zes_deflate gives for
 *               them when the encoder accepts the length (not 1, not 1 mod 131072) and the stream is shorter than the stored
 *               form; otherwise the stored form of zes_pngwrite*: 78 01, stored blocks of 65535 bytes, the Adler-32.  The
 *               Compression tag holds the value the record gave
 *   arrays      behind the segments the values that do not fit an entry, each array at an even offset, in this order:
 *               BitsPerSample when spp >= 3; ExtraSamples when its count is 3; SampleFormat when it is written and spp >= 3;
 *               the offsets when there are at least 2 segments; the byte counts likewise
 *   directory   at an even offset behind them, with a next-offset of 0.  Entries sorted by tag: 256, 257 (LONG); 258 (SHORT
 *               x spp); 259; 262; 273 or 324, 278 or 322 / 323, 279 or 325 (all LONG); 277; 284 = 1; 317 only when the
 *               predictor is 2; 338 only when spp exceeds the photometric's base (1 for Photometric 0 and 1, 3 for 2):
 *               spp - base values, each extra_samples; 339 only when sample_format != 1: spp values; nothing else.  Tags
 *               without a type here are SHORT.  Values that fit 4 bytes lie in their entry
 * Statuses, the first that applies:
 *   1. ZES_E_ARG: a null img or out_len; a null d_in / in with n != 0; a null alloc; flag bits other than ZES_F_PIECES; a
 *      record that step 1 of zes_tiff_read_* rejects (one function serves both; across, down and out_size are computed again
 *      from the other fields); n != out_size; big_endian or tiled above 1; bits not 8, 16 or 32; spp outside 1..4; tile
 *      dimensions that are not non-zero multiples of 16; compression not 1, 8 or 32946; predictor not 1 or 2; photometric not
 *      0, 1 or 2; spp below the photometric's base; extra_samples above 2, or non-zero when spp equals the base;
 *      sample_format not 1, 2 or 3, or 3 at a depth other than 32
 *   2. ZES_E_UNSUPPORTED, the reader's own lines, so that the writer never makes a file the reader refuses: Predictor 2 with
 *      Compression 1; a segment of more than 0xFFFFFFFF decoded bytes; more than 2^31 - 1 segments; and a bound above
 *      0xFFFFFFFF (classic TIFF offsets have 32 bits; BigTIFF is not written)
 *   3. ZES_E_NOSPACE, device form only: cap below the file's size, or a null d_out.  *out_len is the size needed (cap == 0
 *      with a null d_out is the sizing call); every group is still encoded; no byte outside [d_out, d_out + cap) is written,
 *      the bytes inside are unspecified
 * On ZES_OK exactly *out_len bytes are written, at any alignment of d_out.  The input is read only inside the aligned 16-byte
 * groups that hold it.  seg_off / seg_len (null, or across * down values each): the positions and byte counts of the segments
 * as written, what zes_tiff_index would give for the file.
 * zes_tiffwrite_bound: *cap = the file's size with every segment in the stored form (Compression 1: as it is) - exact when
 * all segments go stored, and always enough; *segments (may be null) = across * down.  Statuses 1 and 2 as above with n taken
 * as out_size; a null cap is ZES_E_ARG.  It touches no device.
 * The segments go in groups, in order, as zes_pngwrite*'s images do: up to 1024 of them whose encoder slots take up to 256 MiB
 * (4 and 1 MiB under ZES_F_PIECES: same bytes).  Launches per group:
 *   k_tiff_cut    once: every segment of the group cut out of the image into a 16-byte aligned slot of pooled scratch
 *                 (zes_trim, zes_pool_bytes and zes_stage_poison cover it): Predictor 2 applied, pad columns and rows stored
 *                 as zeros, samples in the file's byte order
 *   the encoder   one batch encode over the slots (no CRC-32 launch); its read-back of the sizes is the group's one
 *                 read-back.  Compression 1 skips it
 *   k_adler_seg   once, only in a group with lengths the encoder refuses (only strips have them: a tile is a multiple of 256
 *                 bytes): their Adler-32s, finished on the host (a second read-back).  A segment that goes stored because its
 *                 stream was longer takes the Adler-32 the encoder left behind the stream
 *   k_tiff_pack   once: the group's segments at their file positions with their pad bytes, as stream or stored form; in the
 *                 last group also the arrays, the directory and the header, which go up once as one host-built blob
 * No launch, copy or synchronisation per segment; Compression 1 takes the same path through the scratch.
 * zes_tiffwrite is the host form: it stages the input, runs the same steps with the bound's room, calls alloc(user, 0, size)
 * once and brings the bytes down (a null answer: ZES_E_ARG).
 * replaces: nothing (the reference has no TIFF container) */
int zes_tiffwrite_bound(const zes_tiff_image* img, uint64_t* cap, uint64_t* segments);
int zes_tiffwrite_dev(const uint8_t* d_in, uint64_t n, const zes_tiff_image* img, uint8_t* d_out, uint64_t cap, uint64_t* out_len,
                      uint64_t* seg_off, uint64_t* seg_len, uint32_t flags);
int zes_tiffwrite(const uint8_t* in, uint64_t n, const zes_tiff_image* img, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                  uint32_t flags);

/* Adler-32 of a buffer (standard value as an unsigned 32-bit).
 * replaces: `calcAdler32` src/adler32.ts:1-10 (byte extraction at src/zlib.ts:37-40). */
int zes_adler32(const uint8_t* in, uint64_t n, uint32_t* adler);
int zes_adler32_dev(const uint8_t* d_in, uint64_t n, uint32_t* adler);
/* Adler-32 of many buffers of device memory in one launch: adler[i] = the Adler-32 of d_in[off[i], off[i] + len[i]), i < count.
 * Any alignment, any length (0 gives 1), buffers may overlap; off, len and adler are host arrays.  count == 0 is ZES_OK.
 * ZES_E_ARG: a null array with count != 0, a null d_in with a non-zero length, more than 2^31 work items (a work item is
 * 64 KiB of a buffer).  Made for many short, unaligned buffers (the outputs of an inflate batch), which zes_adler32_dev
 * would take one launch, one copy and one synchronisation each.
 * replaces: `calcAdler32` src/adler32.ts:1-10, once per buffer. */
int zes_adler32_batch_dev(const uint8_t* d_in, const uint64_t* off, const uint64_t* len, uint32_t* adler, uint32_t count);

/* Batch forms over independent buffers (configs 4/5 of BASELINE.json): count buffers, the
 * i-th at d_in + in_off[i] with in_len[i] bytes, written to d_out + out_off[i] (capacity
 * out_cap[i]); out_len[i] and status[i] filled per buffer.  All launches share the stream
 * so small buffers fill the chip together.  replaces: a caller's loop over deflate()/inflate()
 * (README.md:28-42) — the reference has no batch API. */
int zes_deflate_batch_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len,
                          uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                          uint64_t* out_len, int32_t* status, uint32_t count);
int zes_inflate_batch_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len,
                          uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                          uint64_t* out_len, int32_t* status, uint32_t count, uint32_t flags);
/* The same over host pointers (what a binding's deflateBatch(Uint8Array[]) / inflateBatch hands over): in[i] has
 * in_len[i] bytes.  Deflate writes buffer i to out[i] (capacity out_cap[i] >= zes_deflate_bound(in_len[i]));
 * inflate asks alloc(user, i, n) for buffer i's n result bytes once it is decoded (not called for a buffer whose
 * status is an error).  Per-buffer status[] / out_len[] as above; the return value is only non-zero when the call
 * as a whole could not run. */
int zes_deflate_batch(const uint8_t* const* in, const uint64_t* in_len, uint8_t* const* out, const uint64_t* out_cap,
                      uint64_t* out_len, int32_t* status, uint32_t count);
int zes_inflate_batch_alloc(const uint8_t* const* in, const uint64_t* in_len, zes_alloc_fn alloc, void* user,
                            uint64_t* out_len, int32_t* status, uint32_t count, uint32_t flags);

/* One buffer over several GPUs.  Blocks of the reference format are independent: every 131072-byte
 * block gets its own LZ77 index and its own Huffman codes, and blocks are concatenated bit by bit
 * (src/deflate.ts:20-37, src/lz77.ts:11-22).  So each GPU compresses a contiguous range of blocks and one of them
 * joins the bit streams; the result is bit-identical to zes_deflate of the whole buffer.
 * zes_deflate_range_dev: d_in = first byte of the range, n = its length (a multiple of 131072 unless final_range),
 *   n_readable >= n = bytes readable from d_in — the match finder compares up to 258 bytes past a block's end
 *   (src/lz77.ts:78-85), so a range that is not the last needs that much of the next one behind it.  final_range != 0
 *   sets BFINAL on the range's last block (src/deflate.ts:21-27).  d_out receives the raw bit stream from bit 0
 *   ((*out_bits + 7) / 8 bytes, zero padded; cap >= zes_deflate_bound(n)); *adler = Adler-32 of the range's bytes.
 *   Unlike the other deflate device forms it asks for a 16-byte aligned d_in as well as d_out, else ZES_E_ARG (decided
 *   before any launch): a range starts on a block boundary of the caller's buffer, so it is aligned whenever that is.
 * zes_deflate_join_dev: 78 9C | the pieces, bit-concatenated | zero pad | Adler-32 of the whole (combined from the
 *   pieces' values and lengths: src/adler32.ts:1-10 is associative in that sense), into d_out.  The pieces are device
 *   pointers on this GPU (4-byte aligned), in order; they are read, and d_out is written, in whole dwords: piece i
 *   must be readable up to the dword that holds its last bit (zes_deflate_range_dev's own output is; bits behind the
 *   piece's last one may hold anything; the pointer of a piece of no bits is not looked at and may be null), and
 *   cap >= the result's length rounded up to 4 — otherwise ZES_E_NOSPACE with *out_len = the result's length.
 * replaces: the block loop of src/deflate.ts:20-34 and the wrapper of src/zlib.ts:25-49, split at block boundaries. */
int zes_deflate_range_dev(const uint8_t* d_in, uint64_t n, uint64_t n_readable, int final_range, uint8_t* d_out, uint64_t cap,
                          uint64_t* out_bits, uint32_t* adler);
int zes_deflate_join_dev(const uint8_t* const* d_piece, const uint64_t* piece_bits, const uint32_t* piece_adler,
                         const uint64_t* piece_len, uint32_t count, uint8_t* d_out, uint64_t cap, uint64_t* out_len);

/* One stream over several GPUs, the other direction, and streams too long for one pass: a
 * reference-made stream is a chain of independent blocks of exactly 131072 output bytes (the last one shorter), so
 * any GPU can decode the blocks that START inside a range of the compressed bits once it has found them — the same
 * block-start search and block decoder as zes_inflate_dev, restricted to the range.
 *   d_in .. d_in + c     the piece: 16-byte aligned, c < 512 MiB, holding the range, what the range's last block needs
 *                        behind it (<= 144 KiB) and the header of the block after it
 *   lo_bit, own_bit      blocks that start at bit lo_bit <= s < own_bit (relative to d_in; lo_bit >= 16) belong to the call
 *   exact_start          != 0: a block starts exactly at lo_bit (the end bit of the piece before); 0: the first block
 *                        start found at or behind lo_bit begins the chain (a GPU that takes a middle part of the stream)
 *   d_out, cap           block k of the range goes to d_out + k * 131072; nothing is written behind the range's last block
 *   *first_bit, *end_bit bit positions (relative to d_in) of the range's first block and behind its last one: consecutive
 *                        ranges fit when one's end is the next one's first; *nblocks, *final_block (BFINAL seen)
 * A range without exact_start that holds no block start (a piece in the middle of one block) is ZES_OK with *nblocks == 0,
 * *out_len == 0, nothing written, and *first_bit == *end_bit == lo_bit.
 * ZES_E_NOTRANGE: not a clean chain (another encoder's stream, a false block start): decode the stream with zes_inflate_dev.
 * replaces: the block loop of src/inflate.ts:22-37, split at block boundaries. */
int zes_inflate_range_dev(const uint8_t* d_in, uint64_t c, uint64_t lo_bit, uint64_t own_bit, int exact_start, uint8_t* d_out,
                          uint64_t cap, uint64_t* out_len, uint64_t* first_bit, uint64_t* end_bit, uint32_t* nblocks, int* final_block);

/* Stage-level entry points (device pointers) used by the kernel parity tests; each mirrors
 * one internal function of the reference. */
/* replaces: generateLZ77Codes src/lz77.ts:24-119 for the block [start, start+len) of an n-byte input.
 * tokens[i] = literal byte, or 0x80000000 | (len-3) << 16 | (dist-1) for a match. */
int zes_stage_lz77_dev(const uint8_t* d_in, uint64_t n, uint64_t start, uint32_t len,
                       uint32_t* h_tokens, uint32_t* ntokens);
/* The route record of the calling thread's last zes_stage_lz77_dev call: which of the encoder's data-dependent paths that
 * block took.  For tests: the pipeline entry points record nothing.  Nine words (cap >= 9, else ZES_E_ARG):
 *   [0] [1] [2]  the block's flag word (kept positions | 0x80000000 lazy | 0x40000000 left to k_lz_index | 0x20000000 handed
 *                back) behind the first k_lz_sort launch, k_lz_index and the second k_lz_sort launch; [1] and [2] are 0 for
 *                a block k_lz_sort did not leave to k_lz_index
 *   [3]          k_lz_sort, a block it kept: 1 two filter levels | 2 dense (no filter: every position sorted); 0 one level
 *   [4]          k_lz_index: words of its largest class | 0x40000000 a group above 16384 words | 0x80000000 a sixteenth of
 *                the positions in heavy classes
 *   [5]          head of the match list: matches k_lz_match found, or 0xFFFFFFFF for a block of k_lz_match_lazy
 *   [6]          head of the chain mask (lazy blocks: 1 the mask is there; else 0)
 *   [7]          k_lz_match_lazy: 1 guarded loop | 2 probed | 4 found periodic | 8 phase 3 ran out of its budget |
 *                16 words cleared late after a second chain gave up | 32 phase 3 walked the true chain; else 0
 *   [8]          tokens
 * replaces: nothing (the reference has one path). */
int zes_stage_lz77_route(uint32_t* words, uint32_t cap);
/* replaces: the code-length half of generateDeflateHuffmanTable src/huffman.ts:55-115.
 * hist[nsym] symbol counts → lens[nsym] code lengths (0 = unused), limit maxlen (15 or 7). */
int zes_stage_huff_lengths_dev(const uint32_t* h_hist, uint32_t nsym, uint32_t maxlen, uint8_t* h_lens);
/* The block-parallel inflate tier's acceptance rule (csrc/zes_chain.h) on one buffer's candidate records
 * given as host arrays: candidate k's block starts at bit start_bit[k] (>= 16, strictly ascending), ended at end_bit[k],
 * gave out_len[k] bytes, flags[k] bit 0 = decoded, bit 1 = final.  count: candidates found (the arrays' length); cap: the
 * entries the buffer's list holds; first_bit: where the stream's first block starts.
 * on_device = 0: decided by the function a one-buffer call decides with; no device is touched.  != 0: the records go up
 * and k_inf_chain decides, as for a buffer of a batch.
 * *status: 0 accepted, 2 accepted with the slots behind a false candidate shifted, 1 declined (count 0 or above cap
 * included); *total: the chain's bytes; *aux: status 0 the closing candidate + 1, status 2 the chain's length; map[0, *aux)
 * (room for min(count, cap) entries): the candidate of every chain member.
 * ZES_E_ARG: a null array with count != 0, start bits out of order, count or cap above 1048576.
 * replaces: nothing (the reference decodes serially). */
int zes_stage_chain(const uint32_t* start_bit, const uint64_t* end_bit, const uint32_t* out_len, const uint32_t* flags, uint32_t count,
                    uint32_t cap, uint32_t first_bit, int on_device, int32_t* status, uint64_t* total, uint32_t* aux, uint32_t* map);

/* Fills the pooled scratch with a chosen word, for tests/test_gpu_poison.py: every context that is ready, under its own
 * lock, has its streams synchronised, then every pool (its whole capacity, in whole 32-bit words: a tail of up to 3 bytes
 * stays as it is), the page-locked read-back area, the block decoder's host mirror and the large deflate batch's result
 * array (when there is one) set to `word`, and its streams synchronised again.  Notes about what a pool holds do not
 * outlive the fill: the survivor list's note is dropped and the CRC-32 table counts as absent (the next call that needs
 * it builds it again).  The scan's constant table (not a pool), the staging rings, the profiling state and the route
 * record stay.  *bytes (may be null): the bytes filled, over all contexts — the pools' whole words and the three
 * page-locked areas; right after zes_trim that is the page-locked areas alone.  zes_pool_bytes is unchanged.
 * The rule it tests: the library never clears its scratch between calls, so a call may read only words that the same call
 * wrote; with every word nobody wrote set to a value that would do harm, every call must still give its known answer.
 * replaces: nothing. */
int zes_stage_poison(uint32_t word, uint64_t* bytes);

/* Checks, on the device this context drives, the hardware behaviour k_lz_sort's stable ranks rest on: lanes of one
 * wavefront whose returning LDS add (ds_add_rtn_u32) meets in one word receive their old values in ascending lane order.
 * 256 workgroups x 16 wavefronts x iters rounds x 4 adds over six digit patterns; *bad = values that differ from the rank
 * computed with ballots (0 on gfx950), *checked = values compared.  A diagnostic for tests/test_gpu_hw_props.py.
 * replaces: nothing. */
int zes_selftest_lds_order(uint32_t iters, uint32_t seed, uint64_t* bad, uint64_t* checked);

/* Timing of the last *_dev call's kernels, measured with HIP events on the library's own
 * stream: name/ms pairs for bench.py's roofline leg.  Returns the number of entries. */
typedef struct zes_ktime { const char* name; float ms; uint32_t launches; } zes_ktime;
int zes_last_kernel_times(zes_ktime* out, int cap);
/* Which decoder produced the last zes_inflate*() result: 1 block-parallel (reference-made streams),
 * 2 segment-parallel (any valid stream), 3 sequential wavefront, 4 exact single-lane restatement
 * (DESIGN.md §4); 0 if the call failed before decoding. */
int zes_last_inflate_tier(void);
/* Members the member-parallel path decoded in the calling thread's last zes_gunzip* call; 0 when the member-by-member
 * path answered.  After a zes_bgzf_read* call: the members that call decoded (those with output in the range); 0 when it
 * decoded nothing (an empty range) or returned an error. */
int zes_last_gunzip_members(void);
/* (After zes_init_devices: zes_last_inflate_tier / zes_last_gunzip_members / zes_last_kernel_times report on the context that served the calling
 * thread's last call; zes_set_profiling switches every context.) */
int zes_set_profiling(int on);

/* Deterministic integer-only workload generators: host side, used by bench.py,
 * the tests and the JS fixture script alike. kind: 0 xorshift32 bytes, 1 lowent4k, 2 itext. */
int zes_gen(uint8_t* out, uint64_t n, uint32_t kind, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif /* ZES_H */
