// zes_tiff.hip — the device pieces of the TIFF reader (zes_api.hip: tiff_read_core; include/zes.h: "zes_tiff_*") and, at the
// end of the file, of the TIFF writer (k_tiff_cut, k_tiff_pack), which share tiff_load, tiff_store and the funnel shift.
//
//   k_tiff_place  everything between the decoded segments (tiles or strips) of a call and the caller's pixels, in one launch
//                 over a job table uploaded once: Predictor 2 undone, the samples made little-endian, tile padding and what
//                 lies outside the rectangle dropped, every row put at its place at the rectangle's pitch.  It is the only
//                 thing that writes the output.
//                 Work split: a segment's rows inside the rectangle are cut into units of unit_rows rows and a wave is
//                 launched per (segment, unit), found by bisection over the records' first units — no list, no queue, no
//                 atomic, no wait.  A row is taken by L = 2^lanes_log2 lanes at a time (the smallest power of two whose
//                 runs cover a segment row, at most 64), so a wave takes 64 / L rows side by side: a 16-pixel-wide tile of
//                 8-bit grey has a lane a row, not a wave.
//                 What a lane owns: a run of 16 bytes of the segment row, or of 48 bytes when a pixel is 3, 6 or 12 bytes
//                 long, so that a run always holds whole pixels and starts at a 16-byte boundary of the row.  Tile rows in
//                 the scratch are multiples of 16 bytes at 16-byte aligned slots: the run is fetched by 16-byte loads.  A
//                 strip's rows, and segments read where they lie in the file (Compression 1), have any alignment: the run
//                 is then fetched as the aligned dwords that hold bytes of the row, shifted into place.
//                 Predictor 2: the lane sums its run's pixels channel by channel (a chain as long as the run's pixels, 1 to
//                 16), the runs' totals are scanned across the L lanes of the row by __shfl_up in log2 L steps per channel,
//                 and every lane adds what the lanes below it and the row's earlier chunks (a row longer than L runs is
//                 taken L runs at a time, the running sums kept in registers) hand it.  Sums are modulo 2^bits; the samples
//                 of a big-endian file are swapped before they are added.  The sum starts at the segment's column 0 whatever
//                 the rectangle; runs wholly to the right of the rectangle are not fetched.
//                 Stores: the destination has any alignment.  A run that is kept whole goes out as 16-byte stores when its
//                 place is 16-byte aligned, else as up to 3 head bytes, the aligned dwords of the middle (two neighbouring
//                 dwords of the run funnel-shifted into one) and up to 3 tail bytes; a run the rectangle or the image's edge
//                 cuts goes out bytewise, kept bytes only.  No byte outside the rectangle's rows is written.
//                 Traffic: every decoded byte the rectangle's columns need is read once, every byte of the rectangle is
//                 written once.
#include "../../include/zes.h"
#include "zes_common.h"
#include "zes_kernels.h"
#include "zes_copy.h"

namespace {
__device__ __forceinline__ uint32_t tiff_funnel(uint32_t hi, uint32_t lo, uint32_t bytes) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * bytes)); }

// The run of 4 NW bytes at S.  `whole`: all of it lies inside the row, which ends at E; otherwise, and at any S that is not
// 16-byte aligned, only aligned dwords that hold a byte of [S, E) are read, the others count as zeros.
template <int NW>
__device__ __forceinline__ void tiff_load(const uint8_t* S, const uint8_t* E, bool whole, uint32_t (&w)[NW]) {
  if (whole && ((uintptr_t)S & 15u) == 0) {
#pragma unroll
    for (int k = 0; k < NW / 4; k++) {
      const uint4 v = reinterpret_cast<const uint4*>(S)[k];
      w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
    }
    return;
  }
  const uintptr_t base = (uintptr_t)S & ~(uintptr_t)3, lim = ((uintptr_t)E + 3) & ~(uintptr_t)3;
  const uint32_t sh = (uint32_t)((uintptr_t)S & 3u);
  uint32_t q[NW + 1];
#pragma unroll
  for (int k = 0; k <= NW; k++) q[k] = base + 4u * k < lim ? *reinterpret_cast<const uint32_t*>(base + 4u * k) : 0u;
#pragma unroll
  for (int k = 0; k < NW; k++) w[k] = tiff_funnel(q[k + 1], q[k], sh);
}

// Bytes [b0, b1) of the run to D, the place of byte b0
template <int NW>
__device__ __forceinline__ void tiff_store(uint8_t* D, const uint32_t (&w)[NW], uint32_t b0, uint32_t b1) {
  if (b0 == 0 && b1 == 4u * NW) {
    if (((uintptr_t)D & 15u) == 0) {
#pragma unroll
      for (int k = 0; k < NW / 4; k++) reinterpret_cast<uint4*>(D)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
      return;
    }
    const uint32_t h = (uint32_t)(0 - (uintptr_t)D) & 3u;  // bytes in front of the first aligned dword
    if (h == 0) {
#pragma unroll
      for (int k = 0; k < NW; k++) reinterpret_cast<uint32_t*>(D)[k] = w[k];
      return;
    }
#pragma unroll
    for (uint32_t i = 0; i < 3; i++)
      if (i < h) D[i] = (uint8_t)(w[0] >> (8u * i));
#pragma unroll
    for (int m = 0; m + 1 < NW; m++) reinterpret_cast<uint32_t*>(D + h)[m] = tiff_funnel(w[m + 1], w[m], h);
#pragma unroll
    for (uint32_t i = 0; i < 3; i++)
      if (i < 4u - h) D[h + 4u * (NW - 1) + i] = (uint8_t)(w[NW - 1] >> (8u * (h + i)));
    return;
  }
#pragma unroll
  for (uint32_t i = 0; i < 4u * NW; i++)
    if (i >= b0 && i < b1) D[i - b0] = (uint8_t)(w[i >> 2] >> (8u * (i & 3u)));
}

// Predictor 2 over one chunk of a row: w holds the lane's run (samples in host order), carry[c] the sum of channel c over the
// row's earlier chunks.  li: the lane's place among the L lanes of its row.
template <int BPS, int SPP, int NW>
__device__ __forceinline__ void tiff_sum(uint32_t (&w)[NW], uint32_t (&carry)[4], uint32_t lane, uint32_t li, uint32_t L) {
  constexpr int NS = 4 * NW / BPS;
  static_assert(NS % SPP == 0, "a run holds whole pixels");
  constexpr uint32_t M = BPS == 4 ? 0xFFFFFFFFu : (1u << (8 * (BPS & 3))) - 1u;
  uint32_t s[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) s[i] = BPS == 4 ? w[i] : BPS == 2 ? (w[i >> 1] >> (16 * (i & 1))) & M : (w[i >> 2] >> (8 * (i & 3))) & M;
#pragma unroll
  for (int i = SPP; i < NS; i++) s[i] += s[i - SPP];
  uint32_t add[SPP];
#pragma unroll
  for (int c = 0; c < SPP; c++) {
    uint32_t t = s[NS - SPP + c];
    for (uint32_t d = 1; d < L; d <<= 1) {
      const uint32_t v = __shfl_up(t, d);
      if (li >= d) t += v;
    }
    const uint32_t below = __shfl_up(t, 1);
    add[c] = (li ? below : 0u) + carry[c];
    carry[c] += __shfl(t, (int)(lane | (L - 1)));
  }
#pragma unroll
  for (int i = 0; i < NS; i++) s[i] += add[i % SPP];
#pragma unroll
  for (int k = 0; k < NW; k++) {
    if (BPS == 4) w[k] = s[k];
    else if (BPS == 2) w[k] = (s[2 * k] & M) | (s[2 * k + 1] & M) << 16;
    else w[k] = (s[4 * k] & M) | (s[4 * k + 1] & M) << 8 | (s[4 * k + 2] & M) << 16 | (s[4 * k + 3] & M) << 24;
  }
}

// The rows [row0, row0 + unit_rows) of segment j, as far as they lie below row_hi: runs of 4 NW bytes
template <int NW>
__device__ __forceinline__ void tiff_rows(const uint8_t* src, uint8_t* dst, const ZesTiffCall& c, const ZesTiffJob& j, uint32_t row0, uint32_t lane) {
  constexpr uint64_t RUNB = 4 * NW;
  const uint32_t ps = c.bps * c.spp;
  const uint32_t L = 1u << c.lanes_log2, li = lane & (L - 1), sub = lane >> c.lanes_log2, side = 64u >> c.lanes_log2;
  const uint64_t nbytes = (uint64_t)j.col_hi * ps, skip = (uint64_t)j.col_lo * ps;
  const uint32_t chunks = (uint32_t)((nbytes + L * RUNB - 1) / (L * RUNB));
  const uint32_t key = c.predictor == 2 ? 8 * c.bps + c.spp : 0;
  for (uint32_t p = 0; p < c.unit_rows && row0 + p < j.row_hi; p += side) {
    const uint32_t r = row0 + p + sub;
    const bool live = r < j.row_hi;
    const uint8_t* rowS = src + j.src_off + (uint64_t)r * c.seg_rowbytes;
    uint32_t carry[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < chunks; k++) {
      const uint64_t boff = ((uint64_t)k * L + li) * RUNB;
      const bool has = live && boff < nbytes && (key || boff + RUNB > skip);
      uint32_t w[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) w[i] = 0;
      if (has) tiff_load<NW>(rowS + boff, rowS + c.seg_rowbytes, boff + RUNB <= c.seg_rowbytes, w);
      if (c.big_endian && c.bps > 1) {
#pragma unroll
        for (int i = 0; i < NW; i++) w[i] = c.bps == 2 ? ((w[i] & 0xFF00FF00u) >> 8) | ((w[i] & 0x00FF00FFu) << 8) : __builtin_bswap32(w[i]);
      }
      if constexpr (NW == 4) {
        switch (key) {
          case 8 + 1: tiff_sum<1, 1, NW>(w, carry, lane, li, L); break;
          case 8 + 2: tiff_sum<1, 2, NW>(w, carry, lane, li, L); break;
          case 8 + 4: tiff_sum<1, 4, NW>(w, carry, lane, li, L); break;
          case 16 + 1: tiff_sum<2, 1, NW>(w, carry, lane, li, L); break;
          case 16 + 2: tiff_sum<2, 2, NW>(w, carry, lane, li, L); break;
          case 16 + 4: tiff_sum<2, 4, NW>(w, carry, lane, li, L); break;
          case 32 + 1: tiff_sum<4, 1, NW>(w, carry, lane, li, L); break;
          case 32 + 2: tiff_sum<4, 2, NW>(w, carry, lane, li, L); break;
          case 32 + 4: tiff_sum<4, 4, NW>(w, carry, lane, li, L); break;
          default: break;
        }
      } else {
        switch (key) {
          case 8 + 3: tiff_sum<1, 3, NW>(w, carry, lane, li, L); break;
          case 16 + 3: tiff_sum<2, 3, NW>(w, carry, lane, li, L); break;
          case 32 + 3: tiff_sum<4, 3, NW>(w, carry, lane, li, L); break;
          default: break;
        }
      }
      if (has) {
        const uint64_t lo = skip > boff ? skip : boff, hi = nbytes < boff + RUNB ? nbytes : boff + RUNB;
        if (hi > lo) {
          // (lo >= skip: the byte's image column is not left of the rectangle)
          uint8_t* D = dst + (uint64_t)(j.y0 + r - c.ry) * c.pitch + ((uint64_t)j.x0 * ps + lo - (uint64_t)c.rx * ps);
          tiff_store<NW>(D, w, (uint32_t)(lo - boff), (uint32_t)(hi - boff));
        }
      }
    }
  }
}

// Predictor 2 applied to one chunk of a row: w holds the lane's run (samples in host order), carry[c] channel c of the last
// pixel of the row's earlier chunk (zeros in front of the row).  li: the lane's place among the L lanes of its row.
template <int BPS, int SPP, int NW>
__device__ __forceinline__ void tiff_diff(uint32_t (&w)[NW], uint32_t (&carry)[4], uint32_t lane, uint32_t li, uint32_t L) {
  constexpr int NS = 4 * NW / BPS;
  static_assert(NS % SPP == 0, "a run holds whole pixels");
  constexpr uint32_t M = BPS == 4 ? 0xFFFFFFFFu : (1u << (8 * (BPS & 3))) - 1u;
  uint32_t s[NS], prev[SPP];
#pragma unroll
  for (int i = 0; i < NS; i++) s[i] = BPS == 4 ? w[i] : BPS == 2 ? (w[i >> 1] >> (16 * (i & 1))) & M : (w[i >> 2] >> (8 * (i & 3))) & M;
#pragma unroll
  for (int c = 0; c < SPP; c++) {
    const uint32_t t = s[NS - SPP + c];
    const uint32_t below = __shfl_up(t, 1);
    prev[c] = li ? below : carry[c];
    carry[c] = __shfl(t, (int)(lane | (L - 1)));
  }
  // (the row's first pixel stays as it is: the carry in front of the row is zeros)
  uint32_t d[NS];
#pragma unroll
  for (int i = 0; i < NS; i++) d[i] = (s[i] - (i >= SPP ? s[i - SPP] : prev[i])) & M;
#pragma unroll
  for (int k = 0; k < NW; k++) {
    if (BPS == 4) w[k] = d[k];
    else if (BPS == 2) w[k] = d[2 * k] | d[2 * k + 1] << 16;
    else w[k] = d[4 * k] | d[4 * k + 1] << 8 | d[4 * k + 2] << 16 | d[4 * k + 3] << 24;
  }
}

// The rows [row0, row0 + unit_rows) of segment j, as far as the segment has them, out of the image at img: runs of 4 NW bytes
template <int NW>
__device__ __forceinline__ void tiff_cut_rows(const uint8_t* img, uint8_t* dst, const ZesTiffCall& c, const ZesTiffCutJob& j, uint32_t row0, uint32_t lane) {
  constexpr uint64_t RUNB = 4 * NW;
  const uint32_t ps = c.bps * c.spp;
  const uint32_t L = 1u << c.lanes_log2, li = lane & (L - 1), sub = lane >> c.lanes_log2, side = 64u >> c.lanes_log2;
  const uint64_t nbytes = (uint64_t)j.cols * ps;  // bytes of a segment row that the image has
  const uint32_t chunks = (uint32_t)(((uint64_t)c.seg_rowbytes + L * RUNB - 1) / (L * RUNB));
  const uint32_t key = c.predictor == 2 ? 8 * c.bps + c.spp : 0;
  for (uint32_t p = 0; p < c.unit_rows && row0 + p < j.rows; p += side) {
    const uint32_t r = row0 + p + sub;
    const bool live = r < j.rows, inside = r < j.live_rows;
    const uint8_t* rowS = img + (uint64_t)(j.y0 + r) * c.pitch + (uint64_t)j.x0 * ps;
    uint8_t* rowD = dst + j.dst_off + (uint64_t)r * c.seg_rowbytes;
    uint32_t carry[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < chunks; k++) {
      const uint64_t boff = ((uint64_t)k * L + li) * RUNB;
      uint32_t w[NW];
#pragma unroll
      for (int i = 0; i < NW; i++) w[i] = 0;
      if (inside && boff < nbytes) {
        const uint64_t have = nbytes - boff;  // the run's bytes that the image has: the others, which a dword may share, are zeros
        tiff_load<NW>(rowS + boff, rowS + nbytes, have >= RUNB, w);
        if (have < RUNB) {
#pragma unroll
          for (int i = 0; i < NW; i++) {
            const uint32_t keep = have > 4u * i ? (uint32_t)min<uint64_t>(4, have - 4u * i) : 0u;
            w[i] &= keep >= 4 ? 0xFFFFFFFFu : (1u << (8 * keep)) - 1u;
          }
        }
      }
      if constexpr (NW == 4) {
        switch (key) {
          case 8 + 1: tiff_diff<1, 1, NW>(w, carry, lane, li, L); break;
          case 8 + 2: tiff_diff<1, 2, NW>(w, carry, lane, li, L); break;
          case 8 + 4: tiff_diff<1, 4, NW>(w, carry, lane, li, L); break;
          case 16 + 1: tiff_diff<2, 1, NW>(w, carry, lane, li, L); break;
          case 16 + 2: tiff_diff<2, 2, NW>(w, carry, lane, li, L); break;
          case 16 + 4: tiff_diff<2, 4, NW>(w, carry, lane, li, L); break;
          case 32 + 1: tiff_diff<4, 1, NW>(w, carry, lane, li, L); break;
          case 32 + 2: tiff_diff<4, 2, NW>(w, carry, lane, li, L); break;
          case 32 + 4: tiff_diff<4, 4, NW>(w, carry, lane, li, L); break;
          default: break;
        }
      } else {
        switch (key) {
          case 8 + 3: tiff_diff<1, 3, NW>(w, carry, lane, li, L); break;
          case 16 + 3: tiff_diff<2, 3, NW>(w, carry, lane, li, L); break;
          case 32 + 3: tiff_diff<4, 3, NW>(w, carry, lane, li, L); break;
          default: break;
        }
      }
      if (c.big_endian && c.bps > 1) {  // (behind the differences, which are taken on host-order values)
#pragma unroll
        for (int i = 0; i < NW; i++) w[i] = c.bps == 2 ? ((w[i] & 0xFF00FF00u) >> 8) | ((w[i] & 0x00FF00FFu) << 8) : __builtin_bswap32(w[i]);
      }
      // every byte of the slot is written: pad columns and pad rows as the zeros they are
      if (live && boff < c.seg_rowbytes) tiff_store<NW>(rowD + boff, w, 0, (uint32_t)min<uint64_t>(RUNB, c.seg_rowbytes - boff));
    }
  }
}
}  // namespace

// src: the decoded segments (the scratch, or the file itself for Compression 1); dst: the rectangle's first byte; jobs: c.njobs
// records and the closing one.  Launched with ZES_TIFF_THREADS threads and a wave per unit.
__global__ __launch_bounds__(ZES_TIFF_THREADS) void k_tiff_place(const uint8_t* src, uint8_t* dst, const ZesTiffJob* jobs, ZesTiffCall c) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t unit = blockIdx.x * (ZES_TIFF_THREADS / 64u) + (threadIdx.x >> 6);
  if (unit >= jobs[c.njobs].first_unit) return;
  uint32_t a = 0, b = c.njobs;  // the last record whose first_unit is <= unit
  while (b - a > 1) {
    const uint32_t m = a + (b - a) / 2;
    if (jobs[m].first_unit <= unit) a = m;
    else b = m;
  }
  const ZesTiffJob j = jobs[a];
  const uint32_t row0 = j.row_lo + (unit - j.first_unit) * c.unit_rows;
  if ((c.bps * c.spp) % 3u == 0) tiff_rows<12>(src, dst, c, j, row0, lane);
  else tiff_rows<4>(src, dst, c, j, row0, lane);
}

// ---- the TIFF writer's kernels (zes_api.hip: tiffwrite_core; include/zes.h: "zes_tiffwrite*") ----
//   k_tiff_cut    k_tiff_place run backwards: every segment of a writer's group out of the caller's image into its 16-byte
//                 aligned scratch slot, in one launch over a job table uploaded once.  The work split is k_tiff_place's: a wave
//                 per (segment, unit of rows) found by bisection, L = 2^lanes_log2 lanes to a row, runs of 16 bytes, or 48
//                 when a pixel is 3, 6 or 12 bytes long.
//                 Fetch: the image lies at any alignment and any pitch remainder, so a run is fetched by tiff_load: 16-byte
//                 loads where the run is whole and aligned, else the aligned dwords that hold bytes of the image's part of
//                 the row, funnel-shifted into place; bytes of a shared dword beyond that part are masked to zeros.  Runs
//                 right of the image and rows below it are not fetched: they are zeros.
//                 Predictor 2 needs no scan: a lane needs only the pixel in front of its run.  It comes from the lane below
//                 by __shfl_up, a sample a channel, and across the chunks of a row longer than L runs from the chunk's top
//                 lane, kept in registers: at most 8 cross-lane moves a chunk, where a direct fetch of a pixel of up to 16
//                 bytes at any alignment costs up to 5 loads, as many funnel shifts and their latency.  Differences are
//                 modulo 2^bits on host-order samples, from the segment's column 0 through the pad pixels; the samples of a
//                 big-endian file are swapped behind them.
//                 Stores: every byte of the slot is written, the zeros too (pooled scratch holds an earlier call's bytes).
//                 A tile's rows are multiples of 16 bytes in a 16-byte aligned slot: 16-byte stores.  A strip's rows have any
//                 length: tiff_store, bytewise only in the run that the row's end cuts.
//                 Traffic: every byte of the image is read once, every byte of the slots is written once.
//   k_tiff_pack   the file's ranges of a group over a flat list of workgroups, a record found by bisection as k_zip_pack
//                 finds its entry: a segment as the encoder's stream out of its slot, as the stored form (78 01, a workgroup
//                 per stored block: its five header bytes and its bytes out of the scratch; the Adler-32 the encoder left
//                 behind its stream, or the record's) or as it is (Compression 1), with the zero pad byte behind an odd
//                 length by the segment's last workgroup; and the host-built blobs: the arrays and the directory, and the
//                 header.  Every byte by one workgroup through gz_copy.
__global__ __launch_bounds__(ZES_TIFF_THREADS) void k_tiff_cut(const uint8_t* img, uint8_t* dst, const ZesTiffCutJob* jobs, ZesTiffCall c) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t unit = blockIdx.x * (ZES_TIFF_THREADS / 64u) + (threadIdx.x >> 6);
  if (unit >= jobs[c.njobs].first_unit) return;
  uint32_t a = 0, b = c.njobs;  // the last record whose first_unit is <= unit
  while (b - a > 1) {
    const uint32_t m = a + (b - a) / 2;
    if (jobs[m].first_unit <= unit) a = m;
    else b = m;
  }
  const ZesTiffCutJob j = jobs[a];
  const uint32_t row0 = (unit - j.first_unit) * c.unit_rows;
  if ((c.bps * c.spp) % 3u == 0) tiff_cut_rows<12>(img, dst, c, j, row0, lane);
  else tiff_cut_rows<4>(img, dst, c, j, row0, lane);
}

__global__ __launch_bounds__(GZ_GATHER_THREADS) void k_tiff_pack(const uint8_t* __restrict__ cut, const uint8_t* __restrict__ slots,
                                                                const uint8_t* __restrict__ blob, uint8_t* __restrict__ out,
                                                                const ZesTiffPackRec* __restrict__ recs, uint32_t count) {
  // the last record whose first workgroup is not behind this one (recs[count] closes the table: no workgroup is its own)
  uint32_t lo = 0, hi = count;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (recs[mid].first_wg <= blockIdx.x) lo = mid;
    else hi = mid;
  }
  const ZesTiffPackRec r = recs[lo];
  const uint32_t c = blockIdx.x - r.first_wg, nwg = recs[lo + 1].first_wg - r.first_wg;
  const uint32_t tid = threadIdx.x;
  uint8_t* f = out + r.dst_off;
  if (r.kind != ZES_TIFFW_STORED) {
    const uint8_t* s = (r.kind == ZES_TIFFW_STREAM ? slots : r.kind == ZES_TIFFW_RAW ? cut : blob) + r.src_off;
    const uint64_t b0 = (uint64_t)c * ZES_TIFFW_PIECE, b1 = min<uint64_t>(r.len, b0 + ZES_TIFFW_PIECE);
    if (b1 > b0) gz_copy(s + b0, f + b0, b1 - b0, tid, 0, 1);
    if (c + 1 == nwg && tid == 0 && r.kind != ZES_TIFFW_BLOB && (r.len & 1u)) f[r.len] = 0;
    return;
  }
  // the stored form: 78 01 | per block of ZES_PNGW_BLOCK bytes: final, LEN, NLEN, the bytes | the Adler-32; block c is this
  // workgroup's
  const uint32_t nb = (r.len + ZES_PNGW_BLOCK - 1) / ZES_PNGW_BLOCK;
  const uint64_t zlen = 2ull + 5ull * nb + r.len + 4;
  auto be = [](uint32_t v, uint32_t k) { return (uint8_t)(v >> (8 * (3 - k))); };  // byte k of v, most significant first
  if (c == 0 && tid < 2) f[tid] = tid ? 0x01 : 0x78;
  if (c + 1 == nwg) {
    if (tid >= 32 && tid < 36) {
      const uint32_t k = tid - 32;
      f[zlen - 4 + k] = r.adler_off != ZES_PNGW_NO_SLOT ? slots[r.adler_off + k] : be(r.adler, k);
    }
    if (tid == 36 && (zlen & 1u)) f[zlen] = 0;
  }
  if (c < nb) {
    const uint64_t hb = 2 + (uint64_t)c * (5ull + ZES_PNGW_BLOCK);  // the block's header in the stream
    const uint32_t len = min(ZES_PNGW_BLOCK, r.len - c * ZES_PNGW_BLOCK);
    if (tid >= 64 && tid < 69) {
      const uint32_t k = tid - 64, v = len | (~len << 16);
      f[hb + k] = k ? (uint8_t)(v >> (8 * (k - 1))) : (uint8_t)(c + 1 == nb ? 1 : 0);
    }
    gz_copy(cut + r.src_off + (uint64_t)c * ZES_PNGW_BLOCK, f + hb + 5, len, tid, 0, 1);
  }
}
