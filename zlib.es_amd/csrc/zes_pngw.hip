// zes_pngw.hip — device pieces of the PNG writer (zes_api.hip: pngwrite_core; include/zes.h: "zes_pngwrite*").
//
//   k_png_filter  the scanline filters applied (PNG specification, 9.2) and, for the adaptive modes, chosen: every row of
//                 every image of a group in one launch.  A filtered row depends on raw rows only, so rows are independent:
//                 an image's rows are cut into runs of ZES_PNGW_RUN and a wave is launched per (image, run), found by
//                 bisection over the records' first waves — no list, no queue, no atomic, no wait.  The wave goes through
//                 its rows in order.
//                 What a lane owns: the scratch row (a filter byte and rowbytes bytes) is cut at the 16-byte boundaries of
//                 the scratch, and lane l of tile t owns the aligned group (64 t + l) of the row — 16 filtered bytes, stored
//                 by one 16-byte store.  The groups the row shares with its neighbours (its first and its last one, the
//                 row stride 1 + rowbytes being any number) are stored bytewise, own bytes only.  The lane fetches the raw
//                 bytes under its group and the bytes above them as aligned 16-byte loads (two each, shifted into place:
//                 the input lies at any alignment), and only groups that hold bytes of the image are read.  Left and
//                 upper-left are up to 8 bytes back: they come from the lane below by __shfl_up, and across a tile's
//                 end from lane 63 of the tile before, kept in a register.  So the four neighbours of all 16 bytes stand in
//                 registers, as dwords X (raw), A (left), B (up), C (upper-left), masked to the row's bytes.
//                 Adaptive modes: pass 1 sums min(v, 256 - v) over the filtered bytes v of all five types (64-bit sums a
//                 lane, reduced across the wave by __shfl_xor; a tie goes to the lowest type), pass 2 filters with the
//                 winner.  A row of one tile (up to about 1000 bytes) keeps its registers between the passes; a longer one
//                 is fetched again in pass 2, out of the cache its own pass 1 has just filled.  A fixed type skips pass 1.
//                 Traffic of the launch: every raw byte is read from HBM once as the row itself; it is read again as the
//                 row above (and again in pass 2 of a long row) by the same wave a row later, out of the vector cache or
//                 L2 — only a run's first row fetches a row above that another wave read (1 / ZES_PNGW_RUN of the
//                 input).  Every filtered byte is written once.  In HBM terms: input + input / 16 read, input + height
//                 written.
//   k_png_pack    the files of a group, over a flat list of workgroups: a file has a workgroup per IDAT chunk, found by
//                 bisection as k_zip_pack finds its entry.  A chunk's workgroup writes the chunk's length and type and its
//                 data — a piece of the encoder's stream out of its slot, or of the stored form: 78 01, stored blocks of
//                 ZES_PNGW_BLOCK bytes out of the filtered scratch behind five header bytes each, the Adler-32 (the one the
//                 encoder left behind its stream, or the record's).  The file's first workgroup also writes the signature
//                 and IHDR, PLTE and tRNS (length, type, data), its last one IEND.  Every byte by one workgroup through
//                 gz_copy; the four CRC bytes behind every chunk are left to k_crc32_put (zes_crc.hip).
#include "../../include/zes.h"
#include "zes_common.h"
#include "zes_kernels.h"
#include "zes_copy.h"

namespace {
// The 16 bytes at address `at` (any alignment) as four dwords; of the two aligned groups that hold them, one outside
// [A, E) — the groups that hold bytes of the image — is not read and counts as zeros.
__device__ __forceinline__ void pngw_load16(int64_t at, int64_t A, int64_t E, uint32_t (&o)[4]) {
  const int64_t al = at & ~15ll;
  const uint32_t sh = (uint32_t)(at & 15);
  uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
  if (al >= A && al < E) lo = *reinterpret_cast<const uint4*>((uintptr_t)al);
  if (sh && al + 16 >= A && al + 16 < E) hi = *reinterpret_cast<const uint4*>((uintptr_t)(al + 16));
  const uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  const uint32_t qd = sh >> 2, rb = 8 * (sh & 3u);
  uint32_t e[5];
#pragma unroll
  for (uint32_t k = 0; k < 5; k++) e[k] = qd == 0 ? v[k] : qd == 1 ? v[k + 1] : qd == 2 ? v[k + 2] : v[k + 3];
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) o[k] = (uint32_t)((((uint64_t)e[k + 1] << 32) | e[k]) >> rb);
}

// the mask that keeps the bytes [lo, hi) of the 16 that four dwords hold, dword k
__device__ __forceinline__ uint32_t pngw_mask(int lo, int hi, int k) {
  const int a = min(max(lo - 4 * k, 0), 4), b = min(max(hi - 4 * k, 0), 4);
  const uint32_t below_b = b >= 4 ? 0xFFFFFFFFu : ((1u << (8 * b)) - 1u), below_a = a >= 4 ? 0xFFFFFFFFu : ((1u << (8 * a)) - 1u);
  return below_b & ~below_a;
}

// Dword K of the neighbours BACK bytes behind the 16 that w2..w5 hold (w0, w1: the 8 bytes in front of them).  (Scalars and
// compile-time places: a window kept as an array ends up in memory.)
template <int Q>
__device__ __forceinline__ uint32_t pngw_pick(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5) {
  return Q == 0 ? w0 : Q == 1 ? w1 : Q == 2 ? w2 : Q == 3 ? w3 : Q == 4 ? w4 : w5;
}
template <int BACK, int K>
__device__ __forceinline__ uint32_t pngw_back(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5) {
  constexpr int o = 8 - BACK, q = (o >> 2) + K;
  const uint32_t lo = pngw_pick<q>(w0, w1, w2, w3, w4, w5);
  if ((o & 3) == 0) return lo;
  const uint32_t hi = pngw_pick<(q < 5 ? q + 1 : 5)>(w0, w1, w2, w3, w4, w5);
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (o & 3)));
}

__device__ __forceinline__ uint32_t pngw_paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);  // ties: a, then b, then c
}

__device__ __forceinline__ uint32_t pngw_cost(uint32_t v) { return min(v, 256u - v); }

// One row.  Called by a whole wave with wave-uniform arguments: cur the row's first raw byte, up the first byte of the row
// above (0: the row above is zeros), [A, E) the aligned groups that hold the image, out the row's filter byte in the scratch.
template <int BPP>
__device__ __forceinline__ void pngw_row(int64_t cur, int64_t up, int64_t A, int64_t E, uint8_t* out, uint32_t rowbytes, uint32_t lane, uint32_t mode,
                                         bool restart) {
  const uint32_t m = (uint32_t)((uintptr_t)out & 15u);  // the filter byte's place in its group
  const uint64_t span = (uint64_t)m + 1 + rowbytes;     // bytes from the first group's start to the row's end
  const uint32_t ntiles = (uint32_t)((span + 1023) / 1024);
  uint4* const grp = reinterpret_cast<uint4*>(out - m);
  uint32_t X[4], Aw[4], B[4], Cw[4];
  uint32_t carry0 = 0, carry1 = 0, carry2 = 0, carry3 = 0;  // the last 8 raw bytes and the 8 above them of the tile before: lane 63's
  int p_lo = 0, p_hi = 0;            // the bytes of the lane's group that are the row's: [p_lo, p_hi)
  uint64_t g = 0;                    // the group's number in the row

  // the lane's group of tile t: its four neighbours into X, Aw, B, Cw
  auto fetch = [&](uint32_t t) __attribute__((always_inline)) {
    g = (uint64_t)t * 64 + lane;
    const int64_t x0 = (int64_t)(g * 16) - m - 1;  // the row byte at place 0 of the group (the filter byte is byte -1)
    p_lo = g == 0 ? (int)m : 0;
    p_hi = (int)min<int64_t>(16, max<int64_t>(0, (int64_t)rowbytes - x0));
    uint32_t vc[4] = {0, 0, 0, 0}, vu[4] = {0, 0, 0, 0};
    if (p_hi > 0) {
      const int first = g == 0 ? (int)m + 1 : 0;  // places in front of row byte 0 count as zeros
      pngw_load16(cur + x0, A, E, vc);
      if (up) pngw_load16(up + x0, A, E, vu);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t keep = pngw_mask(first, 16, k);
        vc[k] &= keep, vu[k] &= keep;
      }
    }
    const uint32_t c0 = vc[0], c1 = vc[1], c2 = vc[2], c3 = vc[3], u0 = vu[0], u1 = vu[1], u2 = vu[2], u3 = vu[3];
    const uint32_t sc0 = __shfl_up(c2, 1), sc1 = __shfl_up(c3, 1), su0 = __shfl_up(u2, 1), su1 = __shfl_up(u3, 1);
    const uint32_t lc0 = lane ? sc0 : carry0, lc1 = lane ? sc1 : carry1, lu0 = lane ? su0 : carry2, lu1 = lane ? su1 : carry3;
    carry0 = __shfl(c2, 63), carry1 = __shfl(c3, 63), carry2 = __shfl(u2, 63), carry3 = __shfl(u3, 63);
    const uint32_t k0 = pngw_mask(0, p_hi, 0), k1 = pngw_mask(0, p_hi, 1), k2 = pngw_mask(0, p_hi, 2), k3 = pngw_mask(0, p_hi, 3);
    X[0] = c0 & k0, X[1] = c1 & k1, X[2] = c2 & k2, X[3] = c3 & k3;
    B[0] = u0 & k0, B[1] = u1 & k1, B[2] = u2 & k2, B[3] = u3 & k3;
    Aw[0] = pngw_back<BPP, 0>(lc0, lc1, c0, c1, c2, c3) & k0, Aw[1] = pngw_back<BPP, 1>(lc0, lc1, c0, c1, c2, c3) & k1;
    Aw[2] = pngw_back<BPP, 2>(lc0, lc1, c0, c1, c2, c3) & k2, Aw[3] = pngw_back<BPP, 3>(lc0, lc1, c0, c1, c2, c3) & k3;
    Cw[0] = pngw_back<BPP, 0>(lu0, lu1, u0, u1, u2, u3) & k0, Cw[1] = pngw_back<BPP, 1>(lu0, lu1, u0, u1, u2, u3) & k1;
    Cw[2] = pngw_back<BPP, 2>(lu0, lu1, u0, u1, u2, u3) & k2, Cw[3] = pngw_back<BPP, 3>(lu0, lu1, u0, u1, u2, u3) & k3;
  };

  uint32_t ft = mode;
  if (mode >= ZES_PNGW_BANDED) {
    uint64_t sum[5] = {0, 0, 0, 0, 0};
    for (uint32_t t = 0; t < ntiles; t++) {
      fetch(t);
      uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
      for (int k = 0; k < 4; k++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint32_t x = (X[k] >> (8 * q)) & 255u, a = (Aw[k] >> (8 * q)) & 255u, b = (B[k] >> (8 * q)) & 255u, c = (Cw[k] >> (8 * q)) & 255u;
          s0 += pngw_cost(x);
          s1 += pngw_cost((x - a) & 255u);
          s2 += pngw_cost((x - b) & 255u);
          s3 += pngw_cost((x - ((a + b) >> 1)) & 255u);
          s4 += pngw_cost((x - pngw_paeth(a, b, c)) & 255u);
        }
      sum[0] += s0, sum[1] += s1, sum[2] += s2, sum[3] += s3, sum[4] += s4;
    }
#pragma unroll
    for (int f = 0; f < 5; f++) {
      uint32_t lo = (uint32_t)sum[f], hi = (uint32_t)(sum[f] >> 32);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t other = ((uint64_t)(uint32_t)__shfl_xor((int)hi, d, 64) << 32) | (uint32_t)__shfl_xor((int)lo, d, 64);
        const uint64_t mine = (((uint64_t)hi << 32) | lo) + other;
        lo = (uint32_t)mine, hi = (uint32_t)(mine >> 32);
      }
      sum[f] = ((uint64_t)hi << 32) | lo;
    }
    const int types = (mode == ZES_PNGW_BANDED && restart) ? 2 : 5;
    ft = 0;
    uint64_t best = sum[0];
#pragma unroll
    for (int f = 1; f < 5; f++)
      if (f < types && sum[f] < best) ft = (uint32_t)f, best = sum[f];
    ft = (uint32_t)__builtin_amdgcn_readfirstlane((int)ft);  // (the same in every lane: the sums are)
    carry0 = carry1 = carry2 = carry3 = 0;
  }

  const bool held = mode >= ZES_PNGW_BANDED && ntiles == 1;  // pass 1 left the row's only tile in the registers
  for (uint32_t t = 0; t < ntiles; t++) {
    if (!held) fetch(t);
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t w = 0;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t x = (X[k] >> (8 * q)) & 255u, a = (Aw[k] >> (8 * q)) & 255u, b = (B[k] >> (8 * q)) & 255u;
        uint32_t pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : 0u;
        if (ft == 4) pred = pngw_paeth(a, b, (Cw[k] >> (8 * q)) & 255u);
        w |= ((x - pred) & 255u) << (8 * q);
      }
      o[k] = w;
    }
    if (g == 0) {  // the filter byte, at place m of the row's first group
#pragma unroll
      for (int k = 0; k < 4; k++)
        if ((int)(m >> 2) == k) o[k] = (o[k] & ~(255u << (8 * (m & 3u)))) | ft << (8 * (m & 3u));
    }
    if (p_lo == 0 && p_hi == 16) {
      grp[g] = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
      uint8_t* d = reinterpret_cast<uint8_t*>(grp + g);
#pragma unroll
      for (int p = 0; p < 16; p++)
        if (p >= p_lo && p < p_hi) d[p] = (uint8_t)(o[p >> 2] >> (8 * (p & 3)));
    }
  }
}
}  // namespace

__global__ __launch_bounds__(ZES_PNGW_THREADS) void k_png_filter(const uint8_t* __restrict__ in, uint8_t* __restrict__ filt,
                                                                const ZesPngwJob* __restrict__ jobs, uint32_t njobs) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (ZES_PNGW_THREADS / 64u) + threadIdx.x / 64u));
  if (wave >= jobs[njobs].first_unit) return;
  uint32_t lo = 0, hi = njobs;  // the last image whose first wave is not behind this one
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (jobs[mid].first_unit <= wave) lo = mid;
    else hi = mid;
  }
  const ZesPngwJob j = jobs[lo];
  const int64_t base = (int64_t)(uintptr_t)in + (int64_t)j.src_off;
  const int64_t A = base & ~15ll, E = (base + (int64_t)j.height * (int64_t)j.rowbytes + 15) & ~15ll;
  const uint32_t r0 = (wave - j.first_unit) * ZES_PNGW_RUN, r1 = min(j.height, r0 + ZES_PNGW_RUN);
  for (uint32_t r = r0; r < r1; r++) {
    const int64_t cur = base + (int64_t)r * (int64_t)j.rowbytes, up = r ? cur - (int64_t)j.rowbytes : 0;
    uint8_t* out = filt + j.dst_off + (uint64_t)r * (1ull + j.rowbytes);
    const bool restart = r % 64u == 0;
    switch (j.bpp) {
      case 1: pngw_row<1>(cur, up, A, E, out, j.rowbytes, lane, j.mode, restart); break;
      case 2: pngw_row<2>(cur, up, A, E, out, j.rowbytes, lane, j.mode, restart); break;
      case 3: pngw_row<3>(cur, up, A, E, out, j.rowbytes, lane, j.mode, restart); break;
      case 4: pngw_row<4>(cur, up, A, E, out, j.rowbytes, lane, j.mode, restart); break;
      case 6: pngw_row<6>(cur, up, A, E, out, j.rowbytes, lane, j.mode, restart); break;
      default: pngw_row<8>(cur, up, A, E, out, j.rowbytes, lane, j.mode, restart); break;
    }
  }
}

__global__ __launch_bounds__(GZ_GATHER_THREADS) void k_png_pack(const uint8_t* __restrict__ filt, const uint8_t* __restrict__ slots,
                                                               const uint8_t* __restrict__ aux, uint8_t* __restrict__ out,
                                                               const ZesPngwRec* __restrict__ recs, uint32_t count) {
  // the last record whose first workgroup is not behind this one (recs[count] closes the table: no workgroup is its own)
  uint32_t lo = 0, hi = count;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (recs[mid].first_wg <= blockIdx.x) lo = mid;
    else hi = mid;
  }
  const ZesPngwRec r = recs[lo];
  const uint32_t c = blockIdx.x - r.first_wg, nch = recs[lo + 1].first_wg - r.first_wg;
  const uint32_t tid = threadIdx.x;
  uint8_t* f = out + r.dst_off;
  const uint32_t plte = r.plte_len ? 12u + r.plte_len : 0u, trns = r.trns_len ? 12u + r.trns_len : 0u;
  auto be = [](uint32_t v, uint32_t k) { return (uint8_t)(v >> (8 * (3 - k))); };  // byte k of v, most significant first
  if (c == 0) {
    if (tid < 29) {  // the signature, and IHDR without its CRC
      const uint32_t k = tid >> 2;
      const uint32_t w = k == 0 ? 0x89504e47u
                       : k == 1 ? 0x0d0a1a0au
                       : k == 2 ? 13u
                       : k == 3 ? 0x49484452u
                       : k == 4 ? r.width
                       : k == 5 ? r.height
                       : k == 6 ? (uint32_t)r.depth << 24 | (uint32_t)r.colour << 16  // compression 0, filter method 0
                                : 0u;                                                   // no interlace
      f[tid] = be(w, tid & 3u);
    }
    if (plte) {
      if (tid >= 32 && tid < 40) f[33 + tid - 32] = be(tid < 36 ? (uint32_t)r.plte_len : 0x504c5445u, tid & 3u);
      gz_copy(aux + r.aux_off, f + 33 + 8, r.plte_len, tid, 0, 1);
    }
    if (trns) {
      if (tid >= 64 && tid < 72) f[33 + plte + tid - 64] = be(tid < 68 ? (uint32_t)r.trns_len : 0x74524e53u, tid & 3u);
      gz_copy(aux + r.aux_off + r.plte_len, f + 33 + plte + 8, r.trns_len, tid, 0, 1);
    }
  }
  const uint64_t z0 = (uint64_t)c * ZES_PNGW_IDAT, z1 = min(r.zlen, z0 + ZES_PNGW_IDAT);
  const uint32_t dl = (uint32_t)(z1 - z0);
  uint8_t* ch = f + 33 + plte + trns + (uint64_t)c * (ZES_PNGW_IDAT + 12ull);
  if (tid >= 96 && tid < 104) ch[tid - 96] = be(tid < 100 ? dl : 0x49444154u, tid & 3u);
  if (c + 1 == nch && tid >= 128 && tid < 136) ch[12 + dl + tid - 128] = be(tid < 132 ? 0u : 0x49454e44u, tid & 3u);
  uint8_t* data = ch + 8;  // bytes [z0, z1) of the zlib stream
  if (!r.stored) {
    gz_copy(slots + r.src_off + z0, data, dl, tid, 0, 1);
    return;
  }
  // the stored form: 78 01 | per block of ZES_PNGW_BLOCK bytes: final, LEN, NLEN, the bytes | the Adler-32
  if (tid < 2 && z0 == 0) data[tid] = tid ? 0x01 : 0x78;
  if (tid >= 160 && tid < 164) {
    const uint32_t k = tid - 160;
    const uint64_t zp = r.zlen - 4 + k;
    if (zp >= z0 && zp < z1) data[zp - z0] = r.adler_off != ZES_PNGW_NO_SLOT ? slots[r.adler_off + k] : be(r.adler, k);
  }
  constexpr uint64_t STEP = 5ull + ZES_PNGW_BLOCK;
  const uint32_t nb = (r.flen + ZES_PNGW_BLOCK - 1) / ZES_PNGW_BLOCK;
  for (uint64_t b = z0 > 2 ? (z0 - 2) / STEP : 0; b < nb; b++) {
    const uint64_t hb = 2 + b * STEP;  // the block's header in the stream
    if (hb >= z1) break;
    const uint32_t len = min(ZES_PNGW_BLOCK, r.flen - (uint32_t)b * ZES_PNGW_BLOCK);
    if (tid >= 192 && tid < 197) {
      const uint32_t k = tid - 192, v = len | (~len << 16);
      const uint64_t zp = hb + k;
      if (zp >= z0 && zp < z1) data[zp - z0] = k ? (uint8_t)(v >> (8 * (k - 1))) : (uint8_t)(b + 1 == nb ? 1 : 0);
    }
    const uint64_t d0 = max(hb + 5, z0), d1 = min(hb + 5 + len, z1);
    if (d1 > d0) gz_copy(filt + r.src_off + b * ZES_PNGW_BLOCK + (d0 - hb - 5), data + (d0 - z0), d1 - d0, tid, 0, 1);
  }
}
