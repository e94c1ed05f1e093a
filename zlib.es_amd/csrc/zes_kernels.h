// zes_kernels.h — launch geometry and kernel declarations shared by the .hip files and the host API.
#pragma once
#include "zes_common.h"

#define SORT_THREADS 1024
#define SORT_WAVES (SORT_THREADS / 64)
#ifndef MATCH_THREADS
#define MATCH_THREADS 1024
#endif
#define IDX_THREADS 1024
// k_lz_sort / k_lz_index -> the match finders, per block in idx_a[g][ZES_BLK-1]: kept positions | flags
#define ZES_SORT_LAZY 0x80000000u   // the block's index is sd[] / inv[]: it belongs to k_lz_match_lazy
#define ZES_SORT_INDEX 0x40000000u  // a dense block k_lz_sort left to k_lz_index
#define ZES_SORT_REDO 0x20000000u   // k_lz_index handed the block back (a class too large for its LDS): k_lz_sort, second launch
#define ZES_INV_NONE 0xFFFFFFFFu    // inv entry of a position without a candidate
// The route record (zes_stage_lz77_route, tests only): what the data made a block's kernels do.  k_lz_sort and k_lz_index
// leave one word each in idx_b[g][ZES_BLK-1] (free until the match finders: lists, buckets and k_lz_index's words end below
// it), k_lz_match_lazy one in word 1 of the block's chain mask head; nothing in the pipeline reads them.
#define ZES_ROUTE_WORDS 9u             // words of a record (include/zes.h)
#define ZES_ROUTE_SORT_TWO 1u          // k_lz_sort: two filter levels
#define ZES_ROUTE_SORT_DENSE 2u        // k_lz_sort: a dense block it kept (no filter: every position is sorted)
#define ZES_ROUTE_IDX_MAXC 0x3FFFFu    // k_lz_index: words of its largest class ...
#define ZES_ROUTE_IDX_GROUP 0x40000000u  // ... a group above the LDS's share
#define ZES_ROUTE_IDX_HEAVY 0x80000000u  // ... a sixteenth of the positions in heavy classes
#define ZES_ROUTE_GUARDED 1u           // k_lz_match_lazy: the guarded form of the loop (a block of k_lz_index)
#define ZES_ROUTE_PROBED 2u            // the block was probed (64 windows and more)
#define ZES_ROUTE_PERIODIC 4u          // the probe's verdict: periodic
#define ZES_ROUTE_ABORT3 8u            // phase 3 ran out of its budget: every window got its chain after all
#define ZES_ROUTE_LATE_CLEAR 16u       // an unguarded block whose second chain gave up: words cleared, evaluated once more
#define ZES_ROUTE_WALK3 32u            // phase 3 walked the true chain
#define PARSE_THREADS 1024
#define EMIT_THREADS 1024
#define HUFF_THREADS_HOST 384
#define ADLER_THREADS 256
#define ADLER_CHUNK 65536u
// k_crc32 (zes_crc.hip): a workgroup per 64 KiB chunk, 16 pieces of 16 bytes per thread, 4096 bytes apart; the table
// the host builds (zes_crc_tables): piece tables | fold tables | per-thread shifts | x^(8 * 65536 * m) for m = 0, 1, ...
#define CRC_THREADS 256u
#define CRC_PIECES 16u
#define CRC_CHUNK (CRC_THREADS * CRC_PIECES * 16u)
#define CRC_STRIDE (CRC_THREADS * 16u)
#define CRC_TAB_FOLD 512u
#define CRC_TAB_LANE 640u
#define CRC_TAB_POW (CRC_TAB_LANE + CRC_THREADS)
#define ZES_PAR_DBG_ROW 32  // u64 slots per work item of k_inf_block_par's ZES_DEBUG_PHASES stamps
// k_lz_match_lazy -> k_lz_parse, per block: [0] = 1 when the mask is there, [4..] a bit per position of the greedy chain
#define ZES_TMASK_WORDS (131072 / 32 + 4)
// k_lz_match -> k_lz_parse, per block: [0] = matches found (all ones: a block of k_lz_match_lazy), [1..] the first ZES_MLIST_CAP of them as position | (length - 3) << 17
#define ZES_MLIST_CAP 4095u
#define ZES_MLIST_WORDS 4096u
// k_lz_parse_small -> k_emit, a block parsed from its match list in the pipeline (head word of the list <= ZES_MLIST_CAP):
// the position form.  No token list: the block's row of the token area begins with a pair of words per 32 positions, a
// bit each: [2 i] the position is on the greedy chain, [2 i + 1] a taken match starts there.  A chain position's token is
// the input byte, a taken start's the match word k_lz_match left at the position
#define ZES_POS_WORDS (2u * (131072u / 32u))
#define PAR_THREADS 1024
#define PAR_WAVES (PAR_THREADS / 64)
#define INF_SCAN_THREADS 256
#ifndef INF_SCAN_BYTES
#define INF_SCAN_BYTES 8192u
#endif
#define SEG_BUCKETS 2048u  // T2: at most this many candidate block starts are kept (one per bucket of the compressed stream)

// One entry per buffer of an inflate call (T1); entry [nbuf] is a sentinel carrying the totals.
struct ZesInfBuf {
  uint64_t in_off, c, out_off, cap;
  uint32_t first_chunk;  // k_inf_scan: first workgroup of this buffer
  uint32_t cand_base;    // start of the buffer's region in cand[] / cand_sorted[] / cres[] / map[]
  uint32_t cand_cap;     // entries in that region
  uint32_t work_first;   // k_inf_block_par: first work item of this buffer
  // range form (zes_inflate_range_dev: one piece of a longer stream): the chain of blocks starts at candidate value
  // start_rel (bit position - 16; 0 = right behind the zlib header) or, with ZES_START_ANY, at the first candidate at
  // or behind it; candidates at or behind own_rel only serve as end estimates and are left to the next piece
  uint32_t start_rel;
  uint32_t own_rel;      // 0xFFFFFFFF: the whole buffer
  uint32_t range_flags;  // ZES_START_ANY, ZES_OWN_ONLY
  uint32_t pad;
};
#define ZES_START_ANY 1u
#define ZES_OWN_ONLY 2u  // range form: candidates at or behind own_rel are not decoded (nothing is written for them)

// work_first of the table's sentinel entry in one-buffer calls: the decode kernels take the number of work
// items from the candidate counter on the device (the sentinel's cand_cap holds the launch bound)
#define ZES_WORK_AUTO 0xFFFFFFFFu

struct ZesCandRes {
  uint64_t end_bit;   // absolute bit just past the block's EOB
  uint32_t out_len;
  uint32_t flags;     // bit0 ok, bit1 bfinal
};

// k_inf_block_par*, one-buffer calls: where the results also go, in the host's page-locked memory (the host then checks
// the chain of blocks itself; all null: nothing)
struct ZesParMirror {
  ZesCandRes* cres_host;        // [work] a copy of every work item's result ...
  uint32_t* start_host;         // ... and the bit its block starts at
  const uint32_t* counters;     // the search's counters (final when this kernel starts), copied by work item 0 ...
  uint32_t* counters_host;      // ... to here
  uint32_t counter_words;
};

// T2 (segment-parallel inflate): result of one work item of k_inf_seg_scan
struct ZesSegRes {
  uint64_t end_bit;   // absolute bit where the segment stopped
  uint64_t out_len;   // bytes the segment produces
  uint32_t flags;     // bit0 ok, bit1 the segment ends with the final block, bit2 its symbols did not fit the symbol store
  uint32_t next;      // work item that starts at end_bit (0 = none)
};

// one stored block of a stream that consists of stored blocks only
struct ZesStoredBlk {
  uint64_t src, dst;  // byte offsets inside the stream / inside the output
  uint32_t len, pad;
};

// T2: one entry per buffer of a group; the per-work-item arrays (sres, maps, order, seg, prefix, wins) are laid out
// buffer after buffer, a buffer's part starting at index work_first
struct ZesSegJob {
  uint64_t in_off, c;
  uint64_t sym_base;   // first dword of the buffer's share of the symbol store
  uint32_t cand_base;  // the buffer's candidates in the sorted list
  uint32_t ncand;
  uint32_t work_first;
  uint32_t nseg;       // length of the buffer's chain (0 = not decoded by this tier): k_inf_seg_windows
  // a piece of a longer stream (streams of 512 MiB and more go through this tier piece by piece): work item 0 starts
  // at bit start0 of the piece (16: right behind the zlib header), and a chain that ends in front of a block the piece
  // does not hold whole is accepted as far as it got (ZES_SEG_PARTIAL)
  uint32_t start0;
  uint32_t flags;
};
#define ZES_SEG_PARTIAL 1u

// where a buffer of a segment-parallel group goes (k_inf_seg_translate)
struct ZesSegOut {
  uint64_t out_off, cap;
  uint32_t nseg;  // segments to translate (0: none)
  uint32_t hist;  // bytes of output in front of out_off that exist (a later piece of a long stream: up to 32768)
};

// k_crc32_seg (zes_crc.hip), k_adler_seg (zes_deflate.hip): one buffer of a batch, bytes [off, off + len) of the input
struct ZesCrcSeg {
  uint64_t off, len;
};

// k_gz_walk (zes_gzip.hip): one member of a file whose members all state their size (BGZF); a member's position is the sum
// of the sizes before it
struct ZesGzMember {
  uint32_t size;   // the whole member, header to ISIZE (BSIZE + 1)
  uint32_t hlen;   // its header
  uint32_t crc;    // its trailer: CRC-32 ...
  uint32_t isize;  // ... and length of its output
};
struct ZesGzWalk {
  uint32_t count;  // members written to the table
  uint32_t ok;     // 1: at least two members, all of them qualify, the last one ends with the input
  uint64_t end;    // where the walk stopped
};
#define ZES_GZ_HLEN_MAX 256u  // a member with a longer header does not qualify (the walk reads a header as one window)
// k_bgzf_mark (zes_gzip.hip): a workgroup tests every byte position of a tile of this many bytes for a member's first four
// bytes; a position whose member qualifies becomes one record of the candidate list
#define ZES_BGZF_MARK_TILE 16384u
#define ZES_BGZF_MARK_THREADS 256u
struct ZesBgzfCand {
  uint64_t pos;    // where the member starts
  uint32_t size;   // as ZesGzMember
  uint32_t hlen;
  uint32_t crc;
  uint32_t isize;
};
struct ZesBgzfMark {
  uint32_t count;  // candidates found (those beyond the list's capacity are counted and not stored)
  uint32_t pad[3];
};
// k_gz_gather: one segment of a segmented copy
struct ZesGzSeg {
  uint64_t src_off, dst_off, len;
  uint32_t zhdr;  // 1: the two bytes in front of the destination become 78 9C
  uint32_t pad;
};
#define GZ_GATHER_THREADS 256u
#define GZ_GATHER_PIECE 65536u  // a workgroup's share of a segment
// k_bgzf_pack: one member of a BGZF file being written
struct ZesBgzfRec {
  uint64_t src_off;   // the body's source: ZES_BGZF_STREAM the raw stream's first byte in the slots, ZES_BGZF_STORED the chunk in the input
  uint64_t dst_off;   // the member's first byte in the output
  uint32_t body_len;  // bytes between header and trailer (the member is 18 + body_len + 8 bytes long)
  uint32_t len;       // the chunk's bytes (ISIZE)
  uint32_t crc;       // the chunk's CRC-32
  uint32_t kind;      // ZES_BGZF_*
};
#define ZES_BGZF_STREAM 0u  // the body is the encoder's stream
#define ZES_BGZF_STORED 1u  // the body is one stored block: 01 | LEN | NLEN | the chunk
#define ZES_BGZF_EOF 2u     // the end-of-file marker: no chunk, the body is 03 00
#define ZES_BGZF_HLEN 18u   // a member's header
// k_zip_stage (zes_gzip.hip): one entry of a ZIP archive on its way to the decoders.  Positions are relative to the kernel's
// source pointer: the file itself (device form), or the staged copies of the entry's bytes (host form)
struct ZesZipRec {
  uint64_t hdr_at;    // the local header
  uint64_t name_at;   // the central directory's copy of the name
  uint64_t limit;     // bytes of the file from the local header's first byte to the file's end
  uint64_t dst_off;   // where the body goes: method 8 its scratch slot's byte 2 (behind 78 9C), method 0 its place in the output
  uint32_t csize;     // the body's bytes
  uint16_t name_len, method;
  uint32_t flag0;     // bit 0 of the entry's flags
  uint32_t pad;
};
struct ZesZipVerdict {
  int32_t status;     // ZES_OK, or ZES_E_ZIP: the local header is not what the entry says
  uint32_t pad;
  uint64_t data_off;  // the body's first byte (as hdr_at)
};
// k_zip_pack (zes_gzip.hip): one entry of a ZIP archive being written.  The table has a closing record behind the last
// entry: only its first_wg counts, the launch's workgroups
struct ZesZipPackRec {
  uint64_t src_off;   // the body's source: method 8 the raw stream's first byte in the slots, method 0 the entry's bytes in the input
  uint64_t dst_off;   // the local header's first byte in the output
  uint32_t csize;     // the body's bytes
  uint32_t usize;     // the entry's bytes
  uint32_t crc;       // their CRC-32
  uint32_t name_off;  // the name in the device copy of the names
  uint32_t first_wg;  // the entry's first workgroup: it has the workgroups up to the next record's first one
  uint16_t name_len, method, flags, pad;
  uint32_t pad2;
};
#define ZES_ZIP_PACK_SHARES 1024u  // workgroups that share one entry's body, at most (a share is whole 64 KiB pieces)
// k_png_walk (zes_png.hip): one PNG file of a batch, and its share [tab_base, + tab_cap) of the chunk table
struct ZesPngFile {
  uint64_t in_off, in_len;
  uint32_t tab_base, tab_cap;
};
// what the walk found in one file (the host's png_rule fills the same record): the IHDR fields, the counts, and the verdict
// of the file rule (include/zes.h, "The file rule").  Positions are relative to the file's first byte
struct ZesPngHead {
  int32_t status;       // ZES_OK, ZES_E_PNG or ZES_E_UNSUPPORTED
  uint32_t width, height;
  uint8_t depth, colour, interlace, pad;
  uint32_t nchunks;     // chunks the walk passed; those beyond tab_cap are counted and not stored
  uint32_t idat_count;
  uint32_t plte_len, trns_len;
  uint64_t idat_bytes;
  uint64_t plte_pos, trns_pos;  // the chunks' data (0 when absent)
};
struct ZesPngChunk {
  uint64_t pos;    // the chunk's length field
  uint32_t len;    // its data bytes | ZES_PNG_IDAT
  uint32_t crc;    // the stored CRC field
};
#define ZES_PNG_IDAT 0x80000000u
// k_png_unfilter (zes_png.hip): one image whose filtered scanlines stand in a scratch slot; its bands are the waves
// [first_band, + ceil(height / 64)) of the launch
struct ZesPngJob {
  uint64_t src_off;   // the slot: height rows of 1 + rowbytes bytes
  uint64_t dst_off;   // where the height * rowbytes result bytes go
  uint32_t height, rowbytes, bpp, first_band;
};
#define ZES_PNG_BAND 64u          // rows of a band: a lane each
#define ZES_PNG_UNF_THREADS 256u  // four independent waves to a workgroup
#define ZES_PNG_TO_PASSES 0x80000000u  // in ZesPngJob::bpp: a pass of an interlaced image, dst_off counts in the kernel's `passes`
// k_png_deinterlace (zes_png.hip): one Adam7 image whose seven unfiltered passes stand in a slot of `passes`; pass p begins
// at 16 * pass_off16[p - 1] of the slot, its rows packed (no filter bytes).  Its output rows are cut into tiles of tile_rows,
// a workgroup each: the workgroups [first_tile, + ceil(height / tile_rows)) of the launch.  The image's passes were the
// unfilter jobs [ujob0, + ujobs) of the same call: the kernel leaves an image alone when one of their `bad` words is set
struct ZesPngDeintJob {  // 80 bytes
  uint64_t src_off;   // the slot, 16-byte aligned
  uint64_t dst_off;   // where the height * rowbytes result bytes go, any alignment
  uint32_t width, height, rowbytes;
  uint32_t bits;      // of a pixel: 1, 2, 4, 8, 16, 24, 32, 48, 64
  uint32_t first_tile, tile_rows;
  uint32_t ujob0, ujobs;
  uint32_t pass_off16[7];
  uint32_t pad;
};
#define ZES_PNGD_THREADS 256u
#define ZES_PNGD_TILE_BYTES 32768u  // about what a tile writes
// k_png_expand (zes_png.hip): one image whose scanlines (no filter bytes) become 8-bit RGBA pixels.  Its rows are cut into
// tiles of tile_rows, a workgroup each: the workgroups [first_tile, + ceil(height / tile_rows)) of the launch
struct ZesPngxJob {   // 64 bytes
  uint64_t src_off;   // the scanlines: height rows of rowbytes bytes, any alignment
  uint64_t dst_off;   // where the width * height * 4 result bytes go, any alignment
  uint64_t plte_off, trns_off;  // PLTE and tRNS data in the kernel's `aux` bytes, any alignment
  uint32_t width, height, rowbytes, first_tile;
  uint32_t tile_rows;
  uint16_t plte_len;  // colour 3: bytes of PLTE data, at most 768
  uint16_t trns_len;  // bytes of tRNS data that count: 2 (colour 0), 6 (colour 2), up to plte_len / 3 (colour 3), else 0
  uint8_t depth, colour, pad[2];
  uint32_t pad2;
};
#define ZES_PNGX_THREADS 256u
#define ZES_PNGX_TILE_PIXELS 8192u  // about what a tile holds: 32 KiB of output a workgroup
// k_png_filter (zes_pngw.hip): one image of a PNG writer's group.  Its rows are cut into runs of ZES_PNGW_RUN, a wave each:
// the waves [first_unit, next record's first_unit) of the launch.  The table has a closing record behind the last image:
// only its first_unit counts, the launch's waves
struct ZesPngwJob {
  uint64_t src_off;   // the scanlines in the caller's input: height rows of rowbytes bytes, any alignment
  uint64_t dst_off;   // the 16-byte aligned scratch buffer: height rows of 1 + rowbytes bytes
  uint32_t height, rowbytes;
  uint32_t bpp;       // the filter unit: 1, 2, 3, 4, 6 or 8
  uint32_t mode;      // 0..4: that type on every row; ZES_PNGW_BANDED, ZES_PNGW_ADAPTIVE: the row's cheapest type
  uint32_t first_unit;
  uint32_t pad;
};
#define ZES_PNGW_BANDED 5u      // adaptive, but a row r with r % 64 == 0 chooses between None and Sub (k_png_unfilter's restart rows)
#define ZES_PNGW_ADAPTIVE 6u
#define ZES_PNGW_RUN 16u        // rows of a run: one wave goes through them in order, the row above still in the cache
#define ZES_PNGW_THREADS 256u   // four independent waves to a workgroup
// k_png_pack (zes_pngw.hip): one PNG file being written.  The file has a workgroup per IDAT chunk, [first_wg, next record's
// first_wg); the table has a closing record as ZesZipPackRec's has
struct ZesPngwRec {
  uint64_t src_off;    // stream: the zlib stream's first byte (78 9C) in the slots; stored: the filtered bytes in the scratch
  uint64_t dst_off;    // the signature's first byte in the output
  uint64_t zlen;       // bytes of the zlib stream, the stored form's headers and trailer included
  uint64_t adler_off;  // stored: where the Adler-32's four bytes stand in the slots (behind the encoder's stream), or
                       // ZES_PNGW_NO_SLOT: `adler` holds it
  uint32_t flen;       // stored: the filtered bytes
  uint32_t width, height;
  uint32_t aux_off;    // PLTE data, then tRNS data, in the device copy of the group's aux bytes
  uint32_t first_wg;
  uint32_t adler;
  uint16_t plte_len, trns_len;
  uint8_t depth, colour, stored, pad;
};
#define ZES_PNGW_NO_SLOT 0xFFFFFFFFFFFFFFFFull
#define ZES_PNGW_IDAT 65536u   // data bytes of an IDAT chunk (the last one: what is left)
#define ZES_PNGW_BLOCK 65535u  // bytes of a stored block (the last one: what is left)
// k_tiff_place (zes_tiff.hip): what is the same for every segment of a call, and one touched segment.  A segment's rows
// [row_lo, row_hi) - those the rectangle reaches - are cut into units of unit_rows rows, a wave each: the waves
// [first_unit, next record's first_unit) of the launch.  The table has a closing record behind the last segment: only its
// first_unit counts, the launch's waves
struct ZesTiffCall {
  uint64_t pitch;         // bytes of a row of the rectangle: rw * spp * bps
  uint32_t rx, ry;        // the rectangle's first column and row in the image
  uint32_t seg_rowbytes;  // bytes of a segment's row where it lies: seg_w * spp * bps
  uint32_t lanes_log2;    // a row is taken by 2^lanes_log2 lanes at a time, so a wave takes 64 >> lanes_log2 rows side by side
  uint32_t unit_rows;     // rows of a unit: a multiple of 64 >> lanes_log2
  uint32_t bps, spp;      // bytes a sample (1, 2, 4), samples a pixel (1..4)
  uint32_t predictor;     // 1 or 2
  uint32_t big_endian;
  uint32_t njobs;
};
struct ZesTiffJob {
  uint64_t src_off;       // the segment's decoded bytes: 16-byte aligned in the scratch; anywhere in the file (Compression 1)
  uint32_t x0, y0;        // the image column and row of the segment's first pixel
  uint32_t row_lo, row_hi;  // the segment's rows that lie inside the rectangle
  uint32_t col_lo, col_hi;  // the segment's columns that lie inside the rectangle (the predictor still starts at column 0)
  uint32_t first_unit;
  uint32_t pad;
};
#define ZES_TIFF_THREADS 256u   // four independent waves to a workgroup
// k_tiff_cut (zes_tiff.hip): one segment of a TIFF writer's group, cut out of the caller's image into its scratch slot.  What
// is the same for every segment travels as a ZesTiffCall (pitch: a row of the image; rx, ry: 0).  The segment's rows are cut
// into units of unit_rows rows, a wave each, as k_tiff_place's are; the table has a closing record
struct ZesTiffCutJob {
  uint64_t dst_off;       // the segment's 16-byte aligned slot in the scratch: rows * seg_rowbytes bytes, every one written
  uint32_t x0, y0;        // the image column and row of the segment's first pixel
  uint32_t rows;          // rows of the segment as the file holds it (a tile: seg_h; a strip: its rows of the image)
  uint32_t live_rows;     // ... of which these lie in the image; the rest are zeros
  uint32_t cols;          // the segment's columns that lie in the image; the rest are zeros
  uint32_t first_unit;
};
// k_tiff_pack (zes_tiff.hip): one range of the file being written.  A record has the workgroups [first_wg, next record's
// first_wg): one per ZES_TIFFW_PIECE bytes of a stream, of a segment as it is or of a blob, one per stored block of the
// stored form; the table has a closing record as ZesZipPackRec's has
struct ZesTiffPackRec {
  uint64_t src_off;    // STREAM: the zlib stream's first byte (78 9C) in the slots; STORED, RAW: the segment's bytes in the
                       // scratch; BLOB: the bytes in the device copy of the call's host-built blob
  uint64_t dst_off;    // the range's first byte in the file
  uint64_t adler_off;  // STORED: where the Adler-32's four bytes stand in the slots (behind the encoder's stream), or
                       // ZES_PNGW_NO_SLOT: `adler` holds it
  uint32_t len;        // STREAM: the stream's bytes; STORED, RAW: the segment's decoded bytes; BLOB: its bytes
  uint32_t first_wg;
  uint32_t adler;
  uint32_t kind;
};
#define ZES_TIFFW_STREAM 0u
#define ZES_TIFFW_STORED 1u     // 78 01, stored blocks of ZES_PNGW_BLOCK bytes, the Adler-32: zes_pngwrite*'s stored form
#define ZES_TIFFW_RAW 2u        // Compression 1
#define ZES_TIFFW_BLOB 3u       // the tail (out-of-line arrays and directory) and the header; no pad byte behind it
#define ZES_TIFFW_PIECE 65536u
// k_crc32_put (zes_crc.hip): where buffer q of a k_crc32_seg launch has its CRC-32 stored, most significant byte first, and
// what finishes it from the buffer's two accumulator words: mul * word 0 ^ word 1 ^ add
struct ZesCrcPut {
  uint64_t dst;
  uint32_t mul, add;
};

// CRC-32 host arithmetic (zes_crc.hip): shift(s, k) = s * x^(8k) mod P; the kernel's table with npow powers
uint32_t zes_crc_shift(uint32_t s, uint64_t k);
uint32_t zes_crc_mul(uint32_t a, uint32_t b);  // a * b mod P (zes_crc_shift(0x80000000, k) is x^(8k): a shift kept for many uses)
uint32_t zes_crc_host(const uint8_t* p, uint64_t n);  // CRC-32 of a few bytes on the host (gzip header check)
void zes_crc_tables(uint32_t* tab, uint32_t npow);

#ifdef __HIPCC__
// inflate direction (zes_inflate.hip)
__global__ void k_inf_first_bytes(const uint8_t*, const uint64_t*, uint8_t*, uint32_t);
__global__ void k_inf_scan(const uint8_t*, const ZesInfBuf*, uint32_t, unsigned long long*, uint32_t, uint32_t*, uint8_t*, uint32_t,
                           const uint8_t*);
__global__ void k_inf_set_table1(ZesInfBuf, ZesInfBuf, ZesInfBuf*, uint32_t*, uint32_t);
__global__ void k_inf_verify(const uint8_t*, const ZesInfBuf*, const unsigned long long*, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t, uint32_t*, uint32_t, uint32_t);
__global__ void k_inf_verify_long(const uint8_t*, const ZesInfBuf*, const unsigned long long*, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t, const uint32_t*, uint32_t);
__global__ void k_inf_ranksort(const ZesInfBuf*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t);
__global__ void k_inf_decode(const uint8_t*, uint8_t*, const ZesInfBuf*, ZesRes*, uint64_t*);
__global__ void k_inf_stored_walk(const uint8_t*, uint64_t, uint64_t, uint64_t, ZesStoredBlk*, ZesRes*);
__global__ void k_inf_stored_copy(const uint8_t*, uint64_t, uint8_t*, uint64_t, const ZesStoredBlk*);
__global__ void k_inf_stored_find(const uint8_t*, uint64_t, uint32_t, uint32_t*, uint32_t*);
__global__ void k_inf_stored_rank(const uint8_t*, uint64_t, uint32_t, const uint32_t*, const uint32_t*, uint32_t, uint64_t, ZesStoredBlk*, ZesRes*);
__global__ void k_inf_cand_bucket(const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t*);
__global__ void k_inf_cand_compact(const uint32_t*, uint32_t*, uint32_t*);
__global__ void k_inf_seg_order(const ZesSegJob*, const uint32_t*, uint32_t*);
__global__ void k_inf_seg_scan(const uint8_t*, const ZesSegJob*, uint32_t, const uint32_t*, ZesSegRes*, uint32_t*, uint32_t*, uint32_t,
                               const uint32_t*, uint32_t*, const uint32_t*, uint64_t*);
__global__ void k_inf_seg_scan_short(const uint8_t*, const ZesSegJob*, uint32_t, const uint32_t*, ZesSegRes*, uint32_t*, uint32_t*, uint32_t,
                                     const uint32_t*, uint32_t*, const uint32_t*, uint64_t*);
__global__ void k_inf_seg_block_par(const uint8_t*, const ZesSegJob*, uint32_t, const uint32_t*, ZesSegRes*, uint32_t*, uint32_t*, uint32_t, uint32_t*,
                                    unsigned long long*, uint64_t, uint64_t, uint64_t*, unsigned long long*);
__global__ void k_inf_seg_chain(const ZesSegJob*, const ZesSegRes*, uint32_t*, uint64_t*, ZesRes*, uint32_t*);
__global__ void k_inf_seg_translate(uint8_t*, const ZesSegJob*, const ZesSegOut*, const uint32_t*, const ZesSegRes*, const uint32_t*, const uint64_t*,
                                    const uint8_t*, const uint32_t*, const uint64_t*, uint32_t*);
#define SEGWIN_GROUP 32u
__global__ void k_inf_seg_win_group(const uint32_t*, const uint32_t*, const ZesSegJob*, uint32_t*);
__global__ void k_inf_seg_win_top(const uint32_t*, const ZesSegJob*, uint8_t*, const uint8_t*, const ZesSegOut*);
__global__ void k_inf_seg_win_fin(const uint32_t*, const ZesSegJob*, const uint8_t*, uint8_t*);
__global__ void k_inf_seg_decode(const uint8_t*, uint64_t, uint64_t, uint8_t*, uint64_t, uint64_t, const uint32_t*, const ZesSegRes*,
                                 const uint32_t*, const uint64_t*, const uint8_t*, uint32_t*, uint32_t, uint32_t, uint32_t);
__global__ void k_inf_block_par(const uint8_t*, uint8_t*, const ZesInfBuf*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*,
                                ZesCandRes*, unsigned long long*, const uint32_t*, const uint32_t*, uint32_t*, ZesParMirror);
__global__ void k_inf_block_par2(const uint8_t*, uint8_t*, const ZesInfBuf*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*,
                                ZesCandRes*, unsigned long long*, const uint32_t*, const uint32_t*, uint32_t*, ZesParMirror);
__global__ void k_inf_move_slots(uint8_t*, const uint8_t*, const uint32_t*, const uint32_t*, uint32_t);
__global__ void k_inf_chain(const ZesInfBuf*, const uint32_t*, const uint32_t*, const ZesCandRes*, const uint32_t*, uint32_t*, ZesRes*, const uint32_t*, uint32_t, uint32_t*);
__global__ void k_inf_chain_range(const ZesInfBuf*, const uint32_t*, const uint32_t*, const ZesCandRes*, ZesRes*, unsigned long long*);
__global__ void k_inf_set_table_range(ZesInfBuf, ZesInfBuf, ZesInfBuf*, uint32_t*, uint32_t, const unsigned long long*, unsigned long long);
__global__ void k_inf_exact(const uint8_t*, uint64_t, uint64_t, uint8_t*, uint64_t, uint64_t, const uint64_t*, ZesRes*);
// deflate direction (zes_deflate.hip)
void zes_sort_set_dbg(unsigned long long*);
#ifdef WD_PROFILE
void zes_wd_set_dbg(unsigned long long*);
#endif
void zes_parse_set_dbg(unsigned long long*);
void zes_lazy_set_dbg(unsigned long long*);
void zes_huff_set_dbg(unsigned long long*);
void zes_emit_set_dbg(unsigned long long*);
__global__ void k_make_blks(ZesBuf, uint32_t, ZesBuf*, ZesBlk*, uint32_t, unsigned long long*);
__global__ void k_lz_sort(const uint8_t*, const ZesBuf*, const ZesBlk*, uint32_t*, uint32_t*, uint32_t*, uint16_t*, uint32_t);
__global__ void k_lz_index(const uint8_t*, const ZesBuf*, const ZesBlk*, uint32_t*, uint32_t*, uint32_t*, uint16_t*);
#define ZES_SORT_MODE_FIRST 0u   // k_lz_sort: every block; dense ones are left to k_lz_index when bit 8 is set
#define ZES_SORT_MODE_REDO 1u    // k_lz_sort: only the blocks k_lz_index handed back
#define ZES_SORT_USE_INDEX 256u
__global__ void k_lz_match_lazy(const uint8_t*, const ZesBuf*, const ZesBlk*, const uint32_t*, const uint32_t*, const uint16_t*, uint32_t*, uint32_t*, uint32_t*,
                                const uint32_t*);
__global__ void k_lz_order(const uint32_t*, uint32_t, uint32_t*);
__global__ void k_lz_match(const uint8_t*, const ZesBuf*, const ZesBlk*, const uint32_t*, uint32_t*, uint32_t*);
__global__ void k_lz_parse(const uint8_t*, const ZesBuf*, ZesBlk*, const uint32_t*, uint32_t*, uint32_t*, const uint32_t*, const uint32_t*);
__global__ void k_lz_parse_small(const uint8_t*, const ZesBuf*, ZesBlk*, const uint32_t*, uint32_t*, uint32_t*, const uint32_t*, const uint32_t*, uint32_t);
__global__ void k_huff(ZesBlk*, const uint32_t*, uint32_t*, uint32_t*);
__global__ void k_huff_lengths_only(const uint32_t*, uint32_t, uint32_t, uint8_t*);
__global__ void k_selftest_lds_order(unsigned long long*, uint32_t, uint32_t);
__global__ void k_adler(const uint8_t*, uint64_t, uint64_t, unsigned long long*);
__global__ void k_crc32(const uint8_t*, uint64_t, const uint32_t*, unsigned int*);
__global__ void k_crc32_seg(const uint8_t*, const ZesCrcSeg*, const uint2*, const uint32_t*, unsigned int*);
// gzip reader and BGZF writer (zes_gzip.hip)
__global__ void k_gz_walk(const uint8_t*, uint64_t, ZesGzWalk*, ZesGzMember*, uint32_t);
__global__ void k_bgzf_mark(const uint8_t*, uint64_t, ZesBgzfMark*, ZesBgzfCand*, uint32_t);
__global__ void k_gz_gather(const uint8_t*, uint8_t*, const ZesGzSeg*);
__global__ void k_bgzf_pack(const uint8_t*, const uint8_t*, uint8_t*, const ZesBgzfRec*);
__global__ void k_zip_stage(const uint8_t*, uint8_t*, uint8_t*, const ZesZipRec*, ZesZipVerdict*);
__global__ void k_zip_pack(const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, const ZesZipPackRec*, uint32_t);
// PNG reader (zes_png.hip)
__global__ void k_png_walk(const uint8_t*, const ZesPngFile*, uint32_t, ZesPngHead*, ZesPngChunk*);
__global__ void k_png_unfilter(const uint8_t*, uint8_t*, uint8_t*, const ZesPngJob*, uint32_t, uint32_t, uint32_t*);
__global__ void k_png_deinterlace(const uint8_t*, uint8_t*, const ZesPngDeintJob*, uint32_t, const uint32_t*);
__global__ void k_png_expand(const uint8_t*, const uint8_t*, uint8_t*, const ZesPngxJob*, uint32_t);
// TIFF reader (zes_tiff.hip)
__global__ void k_tiff_place(const uint8_t*, uint8_t*, const ZesTiffJob*, ZesTiffCall);
// TIFF writer (zes_tiff.hip)
__global__ void k_tiff_cut(const uint8_t*, uint8_t*, const ZesTiffCutJob*, ZesTiffCall);
__global__ void k_tiff_pack(const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, const ZesTiffPackRec*, uint32_t);
// PNG writer (zes_pngw.hip, zes_crc.hip)
__global__ void k_png_filter(const uint8_t*, uint8_t*, const ZesPngwJob*, uint32_t);
__global__ void k_png_pack(const uint8_t*, const uint8_t*, const uint8_t*, uint8_t*, const ZesPngwRec*, uint32_t);
__global__ void k_crc32_put(const unsigned int*, const ZesCrcPut*, uint32_t, uint8_t*);
__global__ void k_adler_blocks(const uint8_t*, const ZesBuf*, const ZesBlk*, unsigned long long*);
__global__ void k_adler_seg(const uint8_t*, const ZesCrcSeg*, const uint2*, unsigned long long*);
__global__ void k_layout(uint8_t*, const ZesBuf*, ZesBlk*, const unsigned long long*, ZesRes*);
__global__ void k_emit(uint8_t*, const ZesBuf*, const ZesBlk*, const uint32_t*, const uint32_t*, const uint32_t*, const uint8_t*, const uint32_t*,
                       const uint32_t*);
__global__ void k_zero_u64(unsigned long long*, uint32_t);
__global__ void k_bits_place(uint32_t*, uint64_t, const uint32_t*, uint64_t);
#endif
