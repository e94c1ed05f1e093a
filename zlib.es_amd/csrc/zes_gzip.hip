// zes_gzip.hip — device pieces of the member-parallel gzip reader (zes_api.hip: gunzip_parallel) and of the BGZF writer
// (zes_api.hip: bgzip_core), and of the ZIP reader and writer (zes_api.hip: zip_read_core, zipwrite_core).  The two readers
// share their plan (body_plan, body_run) and differ in the staging kernel, the two writers share the group step (EncGroup)
// and differ in the pack kernel.
//
// A file whose members all state their own size — BGZF, the format of bgzip / htslib: every member's extra field holds a
// subfield 'B','C' with BSIZE = member size - 1 — can be cut into its members without decoding anything.
//
//   k_gz_walk    one wavefront follows the chain of members from byte 0.  The chain is serial (a member's position is the
//                sum of the sizes before it), so a hop costs one memory round trip: the 64 lanes fetch the 256 bytes at the
//                member's start as one coalesced access, a dword per lane, and the header is then parsed from the lanes'
//                registers with uniform lane reads.  The member's trailer (CRC-32, ISIZE) is fetched by eight lanes once
//                its size is known and stored while the next header is on its way, so it adds no round trip of its own.
//   k_bgzf_mark  the same members found in parallel (zes_api.hip: bgzf_index_dev): every byte position is tested for a
//                member's first four bytes, and each hit is judged by the walk's rule by the thread that holds it; the host
//                follows the chain through the list of those that qualify.
//   k_gz_gather  a segmented copy, {src_off, dst_off, len} per segment at any alignment on both sides: workgroup (s, y)
//                takes the 64 KiB pieces y, y + gridDim.y, ... of segment s.  The destination's whole 16-byte groups are
//                written as 16-byte stores; a group's bytes come from the two aligned 16-byte groups of the source that hold
//                them (one, when both sides are aligned alike), shifted into place.  Only groups that hold bytes of the
//                segment are read, and only the segment's bytes are written; the under-16-byte head and tail go bytewise.
//                (The copy itself is gz_copy of zes_copy.h, which the pack kernels call too.)
//   k_bgzf_pack  a workgroup per member of a BGZF file being written (a member is at most 64 KiB): the 18 header bytes, the
//                body at whatever alignment its place has — the encoder's stream out of its scratch slot, or a stored block:
//                five bytes and the chunk out of the caller's input — and the 8 trailer bytes.  Only the member's own bytes
//                are written, and the input is read only inside the aligned 16-byte groups that hold the chunk's bytes.
//   k_zip_stage  workgroups (e, y) for entry e of a ZIP batch: each judges the entry's local header against its directory
//                record (include/zes.h, zes_zip_read*: step 2) — the 30 header bytes at any alignment, the name against the
//                directory's copy strided over the workgroup and joined by a block-wide OR — and workgroup (e, 0) writes
//                the verdict {status, data_off}, whatever the outcome.  When the entry checks out, the workgroups copy its
//                csize body bytes as shares y of gz_copy: a DEFLATE body into its scratch slot behind a 78 9C (k_gz_gather's
//                zhdr layout), a stored one straight to its place in the output.  Only the entry's own bytes are written, and
//                the file is read only inside the aligned 16-byte groups that hold bytes of it.
//   k_zip_pack   the local part of a ZIP archive being written, over a flat list of workgroups: an entry has as many as its
//                body has 64 KiB pieces (one at least, ZES_ZIP_PACK_SHARES at most), so a body of gigabytes is shared and a
//                thousand tiny entries launch a thousand workgroups.  A workgroup finds its entry by bisection over the
//                records' first workgroups.  The entry's first one writes the 30 header bytes and the name (out of the device
//                copy of the names); all of them copy the body as shares of gz_copy — the encoder's stream out of its scratch
//                slot, or the caller's bytes.  Entries meet at any byte: only the entry's own bytes are written, each by one
//                workgroup, and the input is read only inside the aligned 16-byte groups that hold the entry's bytes.
//
// Independent gzip files as one batch (zes_api.hip: gzip_batch_core for the writer; zes_gunzip_batch_dev and
// zes_gunzip_batch_alloc over gzb_heads_dev, gzb_batch and gzb_one_scratch for the reader):
//   k_gz_heads   a wavefront per file of a gunzip batch, as k_gz_walk reads a member: the 64 lanes fetch the file's first 256
//                bytes side by side, lane l bytes 4l .. 4l + 3 into one register by four byte loads (a file starts at any
//                byte), each tested against the file's end; the header is
//                parsed from the lanes' registers with uniform lane reads, the NULs that end FNAME and FCOMMENT are found by
//                ballot; eight lanes fetch the trailer.  One record {candidate, hlen, crc, isize} per file by the rule of
//                zes_gzbatch.h (zes_gz_candidate), which the host forms apply to the caller's memory.  No byte outside the
//                file is read.
//   k_gz_pack    the files of a gzip batch being written, over a flat list of workgroups as in k_zip_pack: a file has as many
//                as its body has 64 KiB pieces (one at least, ZES_GZ_PACK_SHARES at most), found by bisection.  The file's
//                first workgroup writes the 10 header bytes and the 8 trailer bytes; all of them copy the body as shares of
//                gz_copy: the encoder's stream out of its slot, or the stored form, whose blocks (five header bytes, then up
//                to 65535 bytes out of the caller's input) are dealt out to the workgroups in turn.  Files meet at any byte:
//                only the file's own bytes are written, each by one workgroup, and the input is read only inside the
//                aligned 16-byte groups that hold the file's bytes.
#include "../../include/zes.h"
#include "zes_common.h"
#include "zes_kernels.h"
#include "zes_copy.h"
#include "zes_gzbatch.h"

__global__ __launch_bounds__(64) void k_gz_walk(const uint8_t* __restrict__ d_in, uint64_t c, ZesGzWalk* __restrict__ head,
                                               ZesGzMember* __restrict__ tab, uint32_t cap) {
  const uint32_t lane = threadIdx.x;
  uint64_t pos = 0;
  uint32_t k = 0, tb = 0;
  bool ok = true;
  while (pos < c) {
    if (k >= cap) {
      ok = false;
      break;
    }
    uint32_t w = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
      const uint64_t o = pos + lane * 4 + b;
      if (o < c) w |= (uint32_t)d_in[o] << (8 * b);
    }
    if (k && lane < 8) reinterpret_cast<uint8_t*>(&tab[k - 1])[8 + lane] = (uint8_t)tb;  // the member before: its trailer has arrived
    // byte i of the window, the same value in every lane
    auto B = [&](uint32_t i) -> uint32_t { return ((uint32_t)__builtin_amdgcn_readlane((int)w, (int)(i >> 2)) >> (8 * (i & 3u))) & 255u; };
    const uint64_t left = c - pos;
    const uint32_t hlen = 12 + (B(10) | B(11) << 8);
    bool q = B(0) == 0x1f && B(1) == 0x8b && B(2) == 8 && B(3) == 4 && hlen <= ZES_GZ_HLEN_MAX && hlen <= left;
    uint32_t p = 12, size = 0;
    while (q && p + 4 <= hlen) {  // the extra field, subfield by subfield
      const uint32_t sl = B(p + 2) | B(p + 3) << 8;
      if (p + 4 + sl > hlen) break;
      if (!size && B(p) == 'B' && B(p + 1) == 'C' && sl == 2) size = (B(p + 4) | B(p + 5) << 8) + 1;
      p += 4 + sl;
    }
    q = q && p == hlen && size && hlen + 8 <= size && size <= left;
    if (!q) {
      ok = false;
      break;
    }
    if (lane == 0) {
      tab[k].size = size;
      tab[k].hlen = hlen;
    }
    pos += size;
    tb = lane < 8 ? d_in[pos - 8 + lane] : 0u;
    k++;
  }
  if (k && lane < 8) reinterpret_cast<uint8_t*>(&tab[k - 1])[8 + lane] = (uint8_t)tb;
  if (lane == 0) {
    head->count = k;
    head->ok = ok && k >= 2 && pos == c;
    head->end = pos;
  }
}

// The member that may start at pos, judged by k_gz_walk's rule from global memory (no byte at or behind c is read); one that
// qualifies is appended to the list with its trailer.
__device__ __forceinline__ void bgzf_candidate(const uint8_t* __restrict__ d_in, uint64_t c, uint64_t pos, ZesBgzfMark* __restrict__ head,
                                               ZesBgzfCand* __restrict__ list, uint32_t cap) {
  const uint64_t left = c - pos;
  if (left < 12) return;
  const uint8_t* h = d_in + pos;
  auto le16 = [&](uint32_t i) -> uint32_t { return (uint32_t)h[i] | (uint32_t)h[i + 1] << 8; };
  const uint32_t hlen = 12 + le16(10);
  if (hlen > ZES_GZ_HLEN_MAX || hlen > left) return;
  uint32_t p = 12, size = 0;
  while (p + 4 <= hlen) {  // the extra field, subfield by subfield
    const uint32_t sl = le16(p + 2);
    if (p + 4 + sl > hlen) break;
    if (!size && h[p] == 'B' && h[p + 1] == 'C' && sl == 2) size = le16(p + 4) + 1;
    p += 4 + sl;
  }
  if (p != hlen || !size || hlen + 8 > size || size > left) return;
  const uint8_t* t = h + size - 8;
  ZesBgzfCand r;
  r.pos = pos;
  r.size = size;
  r.hlen = hlen;
  r.crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
  r.isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
  const uint32_t at = atomicAdd(&head->count, 1u);
  if (at < cap) list[at] = r;
}

// The parallel member finder: every byte position of d_in[0, c) is tested for 1f 8b 08 04, and the thread that holds a hit
// judges the member there.  Tiles start at the 16-byte boundary at or below d_in and are read as aligned 16-byte groups, a
// thread taking every ZES_BGZF_MARK_THREADS-th group of its tile together with the first dword of the group behind it (the
// three bytes a signature may reach into it, across a tile's end as well); only groups that hold bytes of [0, c) are read,
// and a position counts only when its four bytes lie inside [0, c).
__global__ __launch_bounds__(ZES_BGZF_MARK_THREADS) void k_bgzf_mark(const uint8_t* __restrict__ d_in, uint64_t c, ZesBgzfMark* __restrict__ head,
                                                                    ZesBgzfCand* __restrict__ list, uint32_t cap) {
  const uint32_t sh = (uint32_t)((uintptr_t)d_in & 15u);
  const uint4* p16 = reinterpret_cast<const uint4*>(d_in - sh);
  const uint64_t ngroups = (sh + c + 15) / 16;  // the groups that hold bytes of the input
  constexpr uint32_t TILE_GROUPS = ZES_BGZF_MARK_TILE / 16;
  const uint64_t g0 = (uint64_t)blockIdx.x * TILE_GROUPS + threadIdx.x;
#pragma unroll
  for (uint32_t i = 0; i < TILE_GROUPS / ZES_BGZF_MARK_THREADS; i++) {
    const uint64_t gi = g0 + (uint64_t)i * ZES_BGZF_MARK_THREADS;
    if (gi >= ngroups) break;
    const uint4 v = p16[gi];
    const uint32_t nx = gi + 1 < ngroups ? reinterpret_cast<const uint32_t*>(p16 + gi + 1)[0] : 0u;
    const uint32_t w[5] = {v.x, v.y, v.z, v.w, nx};
    uint32_t hits = 0;
#pragma unroll
    for (uint32_t b = 0; b < 16; b++) {
      const uint32_t sig = (uint32_t)((((uint64_t)w[b / 4 + 1] << 32) | w[b / 4]) >> (8 * (b & 3u)));
      hits |= (sig == 0x04088b1fu ? 1u : 0u) << b;
    }
    while (hits) {
      const uint64_t x = gi * 16 + (uint32_t)(__ffs((int)hits) - 1);  // the hit's distance from the first group's start
      hits &= hits - 1;
      if (x >= sh && x - sh + 4 <= c) bgzf_candidate(d_in, c, x - sh, head, list, cap);
    }
  }
}

__global__ __launch_bounds__(GZ_GATHER_THREADS) void k_gz_gather(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                const ZesGzSeg* __restrict__ segs) {
  const ZesGzSeg sg = segs[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  uint8_t* d = dst + sg.dst_off;
  if (sg.zhdr && blockIdx.y == 0 && tid < 2) d[(int)tid - 2] = tid ? 0x9C : 0x78;
  gz_copy(src + sg.src_off, d, sg.len, tid, blockIdx.y, gridDim.y);
}

// a member's header in front of BSIZE: FLG 4 (FEXTRA), MTIME 0, XFL 0, OS 255, XLEN 6, subfield 'B','C' of SLEN 2
__device__ __constant__ static const uint8_t kBgzfHead[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};

__global__ __launch_bounds__(GZ_GATHER_THREADS) void k_bgzf_pack(const uint8_t* __restrict__ in, const uint8_t* __restrict__ slots,
                                                                uint8_t* __restrict__ out, const ZesBgzfRec* __restrict__ recs) {
  const ZesBgzfRec r = recs[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  uint8_t* m = out + r.dst_off;
  const uint32_t bsize = ZES_BGZF_HLEN + r.body_len + 8 - 1;
  if (tid < ZES_BGZF_HLEN) m[tid] = tid < 16 ? kBgzfHead[tid] : (uint8_t)(bsize >> (8 * (tid - 16)));
  if (tid >= 32 && tid < 40) {
    const uint32_t k = tid - 32;
    m[ZES_BGZF_HLEN + r.body_len + k] = (uint8_t)((k < 4 ? r.crc : r.len) >> (8 * (k & 3u)));
  }
  uint8_t* body = m + ZES_BGZF_HLEN;
  if (r.kind == ZES_BGZF_STREAM) {
    gz_copy(slots + r.src_off, body, r.body_len, tid, 0, 1);
  } else if (r.kind == ZES_BGZF_STORED) {  // 01 | LEN | NLEN | the chunk
    if (tid >= 64 && tid < 69) {
      const uint32_t k = tid - 64, v = r.len | (~r.len << 16);
      body[k] = k ? (uint8_t)(v >> (8 * (k - 1))) : 1;
    }
    gz_copy(in + r.src_off, body + 5, r.len, tid, 0, 1);
  } else if (tid < 2) {  // the end-of-file marker's body: an empty fixed-Huffman block
    body[tid] = tid ? 0 : 3;
  }
}

__global__ __launch_bounds__(GZ_GATHER_THREADS) void k_zip_stage(const uint8_t* __restrict__ src, uint8_t* __restrict__ slots, uint8_t* __restrict__ out,
                                                                const ZesZipRec* __restrict__ recs, ZesZipVerdict* __restrict__ verdicts) {
  const ZesZipRec r = recs[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const uint8_t* h = src + r.hdr_at;  // (the host has seen to it that the header's 30 bytes and the directory's name lie inside the file)
  auto le16 = [&](uint32_t i) -> uint32_t { return (uint32_t)h[i] | (uint32_t)h[i + 1] << 8; };
  const uint32_t nlen = le16(26);
  const uint64_t data = 30ull + nlen + le16(28);  // the body's distance from the header
  const bool fits = h[0] == 0x50 && h[1] == 0x4b && h[2] == 3 && h[3] == 4 && le16(8) == r.method && (h[6] & 1u) == r.flag0 && nlen == r.name_len &&
                    data + r.csize <= r.limit;
  uint32_t diff = fits ? 0u : 1u;
  if (fits) {
    const uint8_t* a = h + 30;
    const uint8_t* b = src + r.name_at;
    for (uint32_t i = tid; i < nlen; i += GZ_GATHER_THREADS) diff |= (uint32_t)(a[i] ^ b[i]);
  }
  const bool ok = __syncthreads_or((int)diff) == 0;
  if (blockIdx.y == 0 && tid == 0) {
    ZesZipVerdict v;
    v.status = ok ? ZES_OK : ZES_E_ZIP;
    v.pad = 0;
    v.data_off = r.hdr_at + data;
    verdicts[blockIdx.x] = v;
  }
  if (!ok) return;
  const uint8_t* body = h + data;
  if (r.method == 8) {
    uint8_t* d = slots + r.dst_off;
    if (blockIdx.y == 0 && tid < 2) d[(int)tid - 2] = tid ? 0x9C : 0x78;
    gz_copy(body, d, r.csize, tid, blockIdx.y, gridDim.y);
  } else {
    gz_copy(body, out + r.dst_off, r.csize, tid, blockIdx.y, gridDim.y);
  }
}

__global__ __launch_bounds__(GZ_GATHER_THREADS) void k_zip_pack(const uint8_t* __restrict__ in, const uint8_t* __restrict__ slots,
                                                               const uint8_t* __restrict__ names, uint8_t* __restrict__ out,
                                                               const ZesZipPackRec* __restrict__ recs, uint32_t count) {
  // the last record whose first workgroup is not behind this one (recs[count] closes the table: no workgroup is its own)
  uint32_t lo = 0, hi = count;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (recs[mid].first_wg <= blockIdx.x) lo = mid; else hi = mid;
  }
  const ZesZipPackRec r = recs[lo];
  const uint32_t y = blockIdx.x - r.first_wg, ny = recs[lo + 1].first_wg - r.first_wg;
  const uint32_t tid = threadIdx.x;
  uint8_t* h = out + r.dst_off;
  if (y == 0) {
    if (tid < 30) {  // the local header, as eight little-endian words (the last one's upper half is not part of it)
      const uint32_t k = tid >> 2;
      const uint32_t w = k == 0 ? 0x04034b50u
                       : k == 1 ? 20u | (uint32_t)r.flags << 16
                       : k == 2 ? (uint32_t)r.method  // time 0
                       : k == 3 ? 33u | r.crc << 16   // date 1980-01-01
                       : k == 4 ? r.crc >> 16 | r.csize << 16
                       : k == 5 ? r.csize >> 16 | r.usize << 16
                       : k == 6 ? r.usize >> 16 | (uint32_t)r.name_len << 16
                                : 0u;                 // no extra field
      h[tid] = (uint8_t)(w >> (8 * (tid & 3u)));
    }
    gz_copy(names + r.name_off, h + 30, r.name_len, tid, 0, 1);
  }
  gz_copy((r.method == 8 ? slots : in) + r.src_off, h + 30 + r.name_len, r.csize, tid, y, ny);
}

namespace {
// the first a.avail bytes of a file as a wavefront holds them: lane l has bytes 4l .. 4l + 3 in w (0 behind the file's end)
struct GzWaveBytes {
  uint32_t w, lane, avail;
  __device__ __forceinline__ uint32_t byte(uint32_t i) const {
    return ((uint32_t)__builtin_amdgcn_readlane((int)w, (int)(i >> 2)) >> (8 * (i & 3u))) & 255u;
  }
  __device__ __forceinline__ uint32_t nul_from(uint32_t p) const {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
      const uint32_t q = lane * 4 + b;
      if (q >= p && q < avail && ((w >> (8 * b)) & 255u) == 0) m |= 1u << b;
    }
    const unsigned long long hit = __ballot(m != 0);
    if (!hit) return avail;
    const uint32_t l = (uint32_t)__ffsll((long long)hit) - 1;
    const uint32_t lm = (uint32_t)__builtin_amdgcn_readlane((int)m, (int)l);
    return l * 4 + (uint32_t)__ffs((int)lm) - 1;
  }
};
}  // namespace

__global__ __launch_bounds__(ZES_GZ_HEADS_THREADS) void k_gz_heads(const uint8_t* __restrict__ d_in, const ZesGzFile* __restrict__ files,
                                                                  ZesGzHead* __restrict__ heads, uint32_t count) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (ZES_GZ_HEADS_THREADS / 64u) + threadIdx.x / 64u));
  if (f >= count) return;
  const ZesGzFile F = files[f];
  const uint8_t* p = d_in + F.off;
  uint32_t w = 0;
#pragma unroll
  for (uint32_t b = 0; b < 4; b++) {
    const uint64_t o = (uint64_t)lane * 4 + b;
    if (o < F.len) w |= (uint32_t)p[o] << (8 * b);
  }
  const uint32_t tb = (lane < 8 && F.len >= 8) ? p[F.len - 8 + lane] : 0u;
  uint32_t t[2] = {0, 0};
#pragma unroll
  for (uint32_t k = 0; k < 8; k++) t[k >> 2] |= (uint32_t)__builtin_amdgcn_readlane((int)tb, (int)k) << (8 * (k & 3u));
  const GzWaveBytes a{w, lane, (uint32_t)min(F.len, (uint64_t)ZES_GZ_HLEN_MAX)};
  uint32_t hlen = 0;
  const bool cand = zes_gz_candidate(a, F.len, F.cap, t[1], &hlen);
  if (lane == 0) heads[f] = ZesGzHead{cand ? 1u : 0u, hlen, t[0], t[1]};
}

__global__ __launch_bounds__(GZ_GATHER_THREADS) void k_gz_pack(const uint8_t* __restrict__ in, const uint8_t* __restrict__ slots,
                                                              uint8_t* __restrict__ out, const ZesGzPackRec* __restrict__ recs, uint32_t count) {
  // the last record whose first workgroup is not behind this one (recs[count] closes the table: no workgroup is its own)
  uint32_t lo = 0, hi = count;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (recs[mid].first_wg <= blockIdx.x) lo = mid; else hi = mid;
  }
  const ZesGzPackRec r = recs[lo];
  const uint32_t y = blockIdx.x - r.first_wg, ny = recs[lo + 1].first_wg - r.first_wg;
  const uint32_t tid = threadIdx.x;
  uint8_t* m = out + r.dst_off;
  if (y == 0) {
    if (tid < 10) m[tid] = tid == 0 ? 0x1f : tid == 1 ? 0x8b : tid == 2 ? 8 : tid == 9 ? 0xff : 0;  // FLG 0, MTIME 0, XFL 0, OS 255
    if (tid >= 32 && tid < 40) {
      const uint32_t k = tid - 32;
      m[10 + r.body_len + k] = (uint8_t)((k < 4 ? r.crc : r.len) >> (8 * (k & 3u)));
    }
  }
  uint8_t* body = m + 10;
  if (!r.stored) {
    gz_copy(slots + r.src_off, body, r.body_len, tid, y, ny);
    return;
  }
  // the stored form: per block of ZES_GZ_STORED_BLOCK bytes final, LEN, NLEN, the bytes; block b is workgroup b mod ny's
  const uint32_t nb = (uint32_t)zes_gz_stored_blocks(r.len);
  for (uint32_t b = y; b < nb; b += ny) {
    const uint32_t at = b * ZES_GZ_STORED_BLOCK;  // (below 2^32 with len)
    const uint32_t len = min(ZES_GZ_STORED_BLOCK, r.len - at);
    uint8_t* blk = body + (uint64_t)b * (5ull + ZES_GZ_STORED_BLOCK);
    if (tid >= 64 && tid < 69) {
      const uint32_t k = tid - 64, v = len | (~len << 16);
      blk[k] = k ? (uint8_t)(v >> (8 * (k - 1))) : (uint8_t)(b + 1 == nb ? 1 : 0);
    }
    gz_copy(in + r.src_off + at, blk + 5, len, tid, 0, 1);
  }
}
