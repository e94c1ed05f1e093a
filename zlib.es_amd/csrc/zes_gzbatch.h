// zes_gzbatch.h — what the batch forms over independent gzip files (include/zes.h: "zes_gzip_batch*", "zes_gunzip_batch*")
// share between the host (zes_api.hip) and the device (zes_gzip.hip): the records of k_gz_heads and k_gz_pack, and the rule
// by which a file of a gunzip batch is a candidate for the batched route.
#pragma once
#include "zes_common.h"
#include "zes_kernels.h"

// k_gz_heads: one file of a gunzip batch, bytes [off, off + len) of the kernel's source; cap: the room its output has (the
// device form's out_cap; ZES_GZB_NO_CAP in the host form, whose outputs are placed behind the verdicts)
struct ZesGzFile {
  uint64_t off, len, cap;
};
#define ZES_GZB_NO_CAP 0xFFFFFFFFFFFFFFFFull
// what k_gz_heads (or the host, by the same rule) found: candidate 1 and the header's length, or candidate 0; the trailer's
// two words as they stand in the file's last 8 bytes (0 for a file shorter than 8 bytes)
struct ZesGzHead {
  uint32_t candidate, hlen, crc, isize;
};
#define ZES_GZ_HEADS_THREADS 256u  // four files a workgroup, a wavefront each
#define ZES_GZB_RATIO 1032ull      // DEFLATE's best: a candidate's ISIZE is at most this many times its body's bytes

// k_gz_pack: one gzip file being written.  The table has a closing record behind the last file: only its first_wg counts,
// the launch's workgroups
struct ZesGzPackRec {
  uint64_t src_off;   // the body's source: the raw stream's first byte in the slots, or (stored) the file's bytes in the input
  uint64_t dst_off;   // the header's first byte in the output
  uint64_t body_len;  // bytes between header and trailer (the file is 10 + body_len + 8 bytes long)
  uint32_t len;       // the input's bytes (ISIZE)
  uint32_t crc;       // their CRC-32
  uint32_t first_wg;  // the file's first workgroup: it has the workgroups up to the next record's first one
  uint32_t stored;    // 1: the body is the stored form, 0: the encoder's stream
};
#define ZES_GZ_STORED_BLOCK 65535u  // the stored form: blocks of this many bytes (LEN has 16 bits), five header bytes each
#define ZES_GZ_PACK_SHARES 1024u    // workgroups that share one file's body, at most

// the stored form of n bytes: one block at least (n == 0: 01 00 00 ff ff)
static inline __host__ __device__ uint64_t zes_gz_stored_blocks(uint64_t n) {
  return n ? (n + ZES_GZ_STORED_BLOCK - 1) / ZES_GZ_STORED_BLOCK : 1;
}
static inline __host__ __device__ uint64_t zes_gz_stored_len(uint64_t n) { return n + 5 * zes_gz_stored_blocks(n); }

__global__ void k_gz_heads(const uint8_t*, const ZesGzFile*, ZesGzHead*, uint32_t);
__global__ void k_gz_pack(const uint8_t*, const uint8_t*, uint8_t*, const ZesGzPackRec*, uint32_t);

// The candidate rule (include/zes.h, "zes_gunzip_batch*": step 1), once for k_gz_heads and the host forms.  `a` gives the
// file's first a.avail = min(len, ZES_GZ_HLEN_MAX) bytes: a.byte(i) for i < a.avail, and a.nul_from(p): the first position in
// [p, a.avail) that holds a zero byte, a.avail when there is none.  isize: the file's last four bytes (len >= 8).  It never
// gives a status: a file that is no candidate is the per-file path's to judge.
template <class A>
__host__ __device__ inline bool zes_gz_candidate(const A& a, uint64_t len, uint64_t cap, uint32_t isize, uint32_t* hlen) {
  if (len < 18) return false;
  if (a.byte(0) != 0x1f || a.byte(1) != 0x8b || a.byte(2) != 8) return false;
  const uint32_t flg = a.byte(3);
  if (flg & 0xE2u) return false;  // reserved bits 5-7, FHCRC
  const uint32_t avail = a.avail;
  uint32_t p = 10;
  if (flg & 4u) {  // FEXTRA: a subfield 'B','C' that states a member shorter than the file makes it a BGZF file
    if (p + 2 > avail) return false;
    const uint32_t end = p + 2 + (a.byte(p) | a.byte(p + 1) << 8);
    if (end > avail) return false;
    for (uint32_t q = p + 2; q + 4 <= end;) {
      const uint32_t sl = a.byte(q + 2) | a.byte(q + 3) << 8;
      if (q + 4 + sl > end) break;
      if (a.byte(q) == 'B' && a.byte(q + 1) == 'C' && sl == 2 && (uint64_t)(a.byte(q + 4) | a.byte(q + 5) << 8) + 1 < len) return false;
      q += 4 + sl;
    }
    p = end;
  }
  for (uint32_t f = 8; f <= 16; f <<= 1)  // FNAME, FCOMMENT: zero-terminated
    if (flg & f) {
      const uint32_t z = a.nul_from(p);
      if (z >= avail) return false;
      p = z + 1;
    }
  if (p > ZES_GZ_HLEN_MAX || (uint64_t)p + 8 > len) return false;
  const uint64_t body = len - 8 - p;
  if (isize > cap || isize > ZES_GZB_RATIO * body) return false;
  *hlen = p;
  return true;
}
