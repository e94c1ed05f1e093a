// zes_copy.h — gz_copy, the byte placement that the container kernels share (zes_gzip.hip: k_gz_gather, k_bgzf_pack,
// k_zip_stage, k_zip_pack; zes_pngw.hip: k_png_pack).
#pragma once
#include "zes_common.h"
#include "zes_kernels.h"

#ifdef __HIPCC__
// Bytes [0, len) of s to d, any alignment on both sides, by the GZ_GATHER_THREADS threads of a workgroup that is share y of
// the ny that copy this range: share 0 writes the bytes in front of d's first 16-byte boundary and behind its last one,
// the whole 16-byte groups between go in pieces of GZ_GATHER_PIECE bytes, piece y, y + ny, ... to share y.
__device__ __forceinline__ void gz_copy(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, uint64_t len, uint32_t tid, uint32_t y, uint32_t ny) {
  // [0, head): in front of the destination's first 16-byte boundary; [head, head + 16 * groups): whole groups; the rest: tail
  const uint64_t head = min(len, (uint64_t)((0 - (uintptr_t)d) & 15u));
  const uint64_t groups = (len - head) / 16;
  if (y == 0) {
    if (tid < head) d[tid] = s[tid];
    const uint64_t t0 = head + groups * 16;
    if (t0 + tid < len) d[t0 + tid] = s[t0 + tid];
  }
  const uint8_t* sa = s + head;                     // the source of group 0
  const uint32_t sh = (uint32_t)((uintptr_t)sa & 15u);  // (the same for every group of the range)
  const uint4* s16 = reinterpret_cast<const uint4*>(sa - sh);
  uint4* d16 = reinterpret_cast<uint4*>(d + head);
  const uint32_t qd = sh >> 2, rb = 8 * (sh & 3u);
  constexpr uint64_t PIECE_GROUPS = GZ_GATHER_PIECE / 16;
  for (uint64_t g0 = (uint64_t)y * PIECE_GROUPS; g0 < groups; g0 += (uint64_t)ny * PIECE_GROUPS) {
    const uint64_t g1 = min(groups, g0 + PIECE_GROUPS);
#pragma unroll 4
    for (uint64_t gi = g0 + tid; gi < g1; gi += GZ_GATHER_THREADS) {
      const uint4 lo = s16[gi];
      if (sh == 0) {
        d16[gi] = lo;
        continue;
      }
      const uint4 hi = s16[gi + 1];  // (sh != 0: the group's last bytes lie in it)
      const uint32_t v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      uint32_t e[5];
#pragma unroll
      for (uint32_t k = 0; k < 5; k++) e[k] = qd == 0 ? v[k] : qd == 1 ? v[k + 1] : qd == 2 ? v[k + 2] : v[k + 3];
      uint4 o;
      o.x = (uint32_t)((((uint64_t)e[1] << 32) | e[0]) >> rb);
      o.y = (uint32_t)((((uint64_t)e[2] << 32) | e[1]) >> rb);
      o.z = (uint32_t)((((uint64_t)e[3] << 32) | e[2]) >> rb);
      o.w = (uint32_t)((((uint64_t)e[4] << 32) | e[3]) >> rb);
      d16[gi] = o;
    }
  }
}
#endif
