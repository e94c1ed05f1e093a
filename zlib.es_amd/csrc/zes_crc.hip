// zes_crc.hip — CRC-32 (the checksum of gzip, zlib's crc32() and PNG: reflected polynomial 0xEDB88320, initial value
// and final XOR 0xFFFFFFFF) on gfx950, and the GF(2) arithmetic its host side needs.
//
// CRC is linear over GF(2).  With raw(M) = the CRC of M from initial value 0 without the final XOR:
//   raw(A || B) = shift(raw(A), |B|) ^ raw(B),  shift(s, k) = s * x^(8k) mod P
//   crc(M)      = raw(M) ^ shift(0xFFFFFFFF, |M|) ^ 0xFFFFFFFF
// so a message can be cut anywhere, every piece reduced on its own and the pieces shifted into place.
//
//   k_crc32   one workgroup per 64 KiB chunk.  Thread t of the chunk owns the 16-byte pieces at offsets
//             (i * 256 + t) * 16, i = 0..15 (16 loads in flight per thread, coalesced across the wave).  A piece's raw
//             CRC is the XOR of 32 lookups, one per nibble, in 16-entry tables in LDS: a 16-entry table puts every
//             entry in a bank of its own, so the 32 lanes of a lane group never conflict (lanes that ask for the same
//             entry are served by a broadcast) — a 256-entry slicing table would meet ~3-way conflicts on random
//             bytes.  The thread folds its pieces together by shifting its state over the 4080 bytes between them
//             (8 more nibble lookups) and XORs the result into the next piece's first dword.  Each thread's state is
//             then shifted to the chunk's end (one GF(2) multiply by a constant of its own), XOR-reduced over the
//             workgroup, shifted to its place in the message (one multiply by x^(8 * 65536 * m)) and XORed into the
//             accumulator with one atomic.
//   tail      the last chunk (shorter than 64 KiB) and the chunks of an input that is not 16-byte aligned are read
//             bytewise, laid out against the chunk's END: the missing bytes count as leading zeros, which leave a raw
//             CRC unchanged, so the same per-thread constants apply.  The last chunk XORs into a second word, which
//             the host shifts by the last chunk's length (it is the only shift that is not a multiple of 64 KiB).
//   k_crc32_seg  many buffers at any alignment in one launch; a work item is (buffer, 64 KiB chunk).  The chunks of a buffer
//             are cut at 64 KiB steps of MEMORY counted from the 16-byte boundary at or below its first byte, so every piece
//             of every chunk is an aligned 16-byte load whatever the buffer's start.  A short chunk (the first one of an
//             unaligned buffer, the last one) lays its bytes against the chunk's end as the tail above does, so the same
//             per-thread constants apply; rows of pieces that lie wholly in front of the data are skipped.  What goes
//             bytewise: the piece the buffer starts inside (under 16 bytes) and the bytes behind the buffer's last 16-byte
//             boundary (under 16), which the last chunk's first thread runs through the CRC register behind the chunk's
//             state.  Two accumulator words per buffer, as above; the host shifts word 0 by the last work item's bytes.
#include "zes_common.h"
#include "zes_kernels.h"

#define CRC_POLY 0xEDB88320u

// ---- host and device: GF(2) multiply of two reflected polynomials mod P (bit 31 = x^0) ----
__host__ __device__ static inline uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
#pragma unroll
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
  }
  return p;
}

// x^(8k) mod P
static uint32_t crc_x8n(uint64_t k) {
  static uint32_t pw[64];  // x^(8 * 2^j)
  static bool ready = false;
  if (!ready) {
    uint32_t v = 0x00800000u;  // x^8
    for (int j = 0; j < 64; j++) {
      pw[j] = v;
      v = crc_mulmod(v, v);
    }
    ready = true;
  }
  uint32_t r = 0x80000000u;  // x^0
  for (int j = 0; k; j++, k >>= 1)
    if (k & 1u) r = crc_mulmod(r, pw[j]);
  return r;
}

uint32_t zes_crc_shift(uint32_t s, uint64_t k) { return crc_mulmod(crc_x8n(k), s); }
uint32_t zes_crc_mul(uint32_t a, uint32_t b) { return crc_mulmod(a, b); }

// raw CRC of n bytes, bit by bit (host: table construction only)
static uint32_t crc_raw_bits(const uint8_t* p, uint32_t n) {
  uint32_t c = 0;
  for (uint32_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int b = 0; b < 8; b++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
  }
  return c;
}

uint32_t zes_crc_host(const uint8_t* p, uint64_t n) {  // (a few header bytes: gzip's FHCRC)
  uint32_t c = 0xFFFFFFFFu;
  for (uint64_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int b = 0; b < 8; b++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
  }
  return c ^ 0xFFFFFFFFu;
}

void zes_crc_tables(uint32_t* tab, uint32_t npow) {
  // [0, 512): piece tables, [k][v] = raw CRC of 16 bytes whose nibble k (low nibble of byte 0 first) is v, all else 0
  for (uint32_t k = 0; k < 32; k++)
    for (uint32_t v = 0; v < 16; v++) {
      uint8_t piece[16] = {0};
      piece[k >> 1] = (uint8_t)(v << (4 * (k & 1)));
      tab[k * 16 + v] = crc_raw_bits(piece, 16);
    }
  // [512, 640): fold tables, [m][v] = shift(v << 4m, 4080)
  const uint32_t gap = crc_x8n((uint64_t)CRC_STRIDE - 16);
  for (uint32_t m = 0; m < 8; m++)
    for (uint32_t v = 0; v < 16; v++) tab[CRC_TAB_FOLD + m * 16 + v] = crc_mulmod(gap, v << (4 * m));
  // [640, 896): thread t's shift to the chunk's end, x^(8 * 16 * (255 - t))
  for (uint32_t t = 0; t < CRC_THREADS; t++) tab[CRC_TAB_LANE + t] = crc_x8n((uint64_t)16 * (CRC_THREADS - 1 - t));
  // [896, ...): x^(8 * 65536 * m)
  const uint32_t step = crc_x8n(CRC_CHUNK);
  uint32_t v = 0x80000000u;
  for (uint32_t m = 0; m < npow; m++) {
    tab[CRC_TAB_POW + m] = v;
    v = crc_mulmod(v, step);
  }
}

// ---- device ----
// raw CRC of one 16-byte piece (its first dword already XORed with the state carried in)
__device__ __forceinline__ static uint32_t crc_piece(const uint32_t* __restrict__ s_t, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
  uint32_t r = 0;
  const uint32_t d[4] = {d0, d1, d2, d3};
#pragma unroll
  for (uint32_t w = 0; w < 4; w++)
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) r ^= s_t[(w * 8 + q) * 16 + ((d[w] >> (4 * q)) & 15u)];
  return r;
}

__device__ __forceinline__ static uint32_t crc_fold(const uint32_t* __restrict__ s_t, uint32_t s) {
  uint32_t r = 0;
#pragma unroll
  for (uint32_t q = 0; q < 8; q++) r ^= s_t[CRC_TAB_FOLD + q * 16 + ((s >> (4 * q)) & 15u)];
  return r;
}

// acc[0] ^= shift(raw(chunk j), 65536 * (nch - 2 - j)) for every chunk but the last; acc[1] ^= raw(last chunk)
__global__ __launch_bounds__(CRC_THREADS) void k_crc32(const uint8_t* __restrict__ d_in, uint64_t n, const uint32_t* __restrict__ tab,
                                                      unsigned int* __restrict__ acc) {
  __shared__ uint32_t s_t[CRC_TAB_LANE];
  __shared__ uint32_t s_w[CRC_THREADS / 64];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < CRC_TAB_LANE; i += CRC_THREADS) s_t[i] = tab[i];
  const uint64_t nch = (n + CRC_CHUNK - 1) / CRC_CHUNK, j = blockIdx.x;
  const uint64_t base = j * CRC_CHUNK;
  const uint32_t len = (uint32_t)min((uint64_t)CRC_CHUNK, n - base);
  const uint8_t* p = d_in + base;
  uint32_t st = 0;
  if (len == CRC_CHUNK && (((uintptr_t)p) & 15u) == 0) {
    uint4 v[CRC_PIECES];
#pragma unroll
    for (uint32_t i = 0; i < CRC_PIECES; i++) v[i] = reinterpret_cast<const uint4*>(p)[i * CRC_THREADS + tid];
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < CRC_PIECES; i++) st = crc_piece(s_t, v[i].x ^ (i ? crc_fold(s_t, st) : 0u), v[i].y, v[i].z, v[i].w);
  } else {
    // bytewise, laid out against the chunk's end: virtual offset o holds byte o - lead (leading zeros: no effect)
    __syncthreads();
    const int64_t lead = (int64_t)CRC_CHUNK - len;
    for (uint32_t i = 0; i < CRC_PIECES; i++) {
      const int64_t o = (int64_t)(i * CRC_THREADS + tid) * 16 - lead;
      uint32_t d[4] = {0, 0, 0, 0};
      if (o + 16 > 0)
        for (int b = 0; b < 16; b++)
          if (o + b >= 0) d[b >> 2] |= (uint32_t)p[o + b] << (8 * (b & 3));
      st = crc_piece(s_t, d[0] ^ (i ? crc_fold(s_t, st) : 0u), d[1], d[2], d[3]);
    }
  }
  st = crc_mulmod(st, tab[CRC_TAB_LANE + tid]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) st ^= (uint32_t)__shfl_xor((int)st, m, 64);
  if ((tid & 63u) == 0) s_w[tid >> 6] = st;
  __syncthreads();
  if (tid == 0) {
    uint32_t r = 0;
    for (uint32_t w = 0; w < CRC_THREADS / 64; w++) r ^= s_w[w];
    if (j + 1 == nch) atomicXor(&acc[1], r);
    else atomicXor(&acc[0], crc_mulmod(r, tab[CRC_TAB_POW + (nch - 2 - j)]));
  }
}

// Work item w = (buffer, chunk) of segs[]; acc[2b] / acc[2b + 1] as k_crc32's two words, for buffer b.  With a = the address
// of the buffer's first byte, A = a rounded down to 16, E = its end rounded down to 16 (a, when that lies in front of a):
// chunk j holds [max(a, A + 64Ki * j), min(E, A + 64Ki * (j + 1))), the last one also the bytes [E, end).
__global__ __launch_bounds__(CRC_THREADS) void k_crc32_seg(const uint8_t* __restrict__ d_in, const ZesCrcSeg* __restrict__ segs,
                                                          const uint2* __restrict__ work, const uint32_t* __restrict__ tab,
                                                          unsigned int* __restrict__ acc) {
  __shared__ uint32_t s_t[CRC_TAB_LANE];
  __shared__ uint32_t s_w[CRC_THREADS / 64];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < CRC_TAB_LANE; i += CRC_THREADS) s_t[i] = tab[i];
  const uint2 w = work[blockIdx.x];
  const ZesCrcSeg sg = segs[w.x];
  // (signed: virtual offset 0 of a short chunk may stand for an address below zero)
  const int64_t a = (int64_t)(uintptr_t)d_in + (int64_t)sg.off, end = a + (int64_t)sg.len;
  const int64_t A = a & ~15ll, E = max(end & ~15ll, a), CH = CRC_CHUNK;
  const int64_t nch = E > a ? (E - A + CH - 1) / CH : 1, j = w.y;
  const int64_t lo = max(a, A + j * CH);
  const int64_t hi = max(lo, min(E, A + (j + 1) * CH));
  const uint32_t len = (uint32_t)(hi - lo);
  const int64_t v0 = hi - CH;  // the address virtual offset 0 stands for (16-byte aligned whenever len != 0)
  uint32_t st = 0;
  __syncthreads();
  if (len == CRC_CHUNK) {
    uint4 v[CRC_PIECES];
#pragma unroll
    for (uint32_t i = 0; i < CRC_PIECES; i++) v[i] = reinterpret_cast<const uint4*>((uintptr_t)lo)[i * CRC_THREADS + tid];
#pragma unroll
    for (uint32_t i = 0; i < CRC_PIECES; i++) st = crc_piece(s_t, v[i].x ^ (i ? crc_fold(s_t, st) : 0u), v[i].y, v[i].z, v[i].w);
  } else if (len) {
    const uint32_t row0 = (CRC_CHUNK - len) / CRC_STRIDE;  // the first row of pieces that holds data
    uint4 v[CRC_PIECES];
#pragma unroll
    for (uint32_t i = 0; i < CRC_PIECES; i++) {
      v[i] = make_uint4(0, 0, 0, 0);
      if (i < row0) continue;
      const int64_t m = v0 + (int64_t)(i * CRC_THREADS + tid) * 16;
      if (m >= lo) {
        v[i] = *reinterpret_cast<const uint4*>((uintptr_t)m);
      } else if (m + 16 > lo) {  // the piece the buffer starts inside
        uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t b = 0; b < 16; b++)
          if (m + b >= lo) d[b >> 2] |= (uint32_t)(*reinterpret_cast<const uint8_t*>((uintptr_t)(m + b))) << (8 * (b & 3));
        v[i] = make_uint4(d[0], d[1], d[2], d[3]);
      }
    }
#pragma unroll
    for (uint32_t i = 0; i < CRC_PIECES; i++)
      if (i >= row0) st = crc_piece(s_t, v[i].x ^ crc_fold(s_t, st), v[i].y, v[i].z, v[i].w);
  }
  st = crc_mulmod(st, tab[CRC_TAB_LANE + tid]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) st ^= (uint32_t)__shfl_xor((int)st, m, 64);
  if ((tid & 63u) == 0) s_w[tid >> 6] = st;
  __syncthreads();
  if (tid == 0) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < CRC_THREADS / 64; k++) r ^= s_w[k];
    if (j + 1 == nch) {
      for (int64_t q = E; q < end; q++) {  // behind the last 16-byte boundary: through the register, bit by bit
        r ^= *reinterpret_cast<const uint8_t*>((uintptr_t)q);
        for (int b = 0; b < 8; b++) r = (r >> 1) ^ (CRC_POLY & (0u - (r & 1u)));
      }
      atomicXor(&acc[2 * (size_t)w.x + 1], r);
    } else {
      atomicXor(&acc[2 * (size_t)w.x], crc_mulmod(r, tab[CRC_TAB_POW + (nch - 2 - j)]));
    }
  }
}

// Buffer q of a k_crc32_seg launch finished on the device and stored, most significant byte first (a PNG chunk's CRC
// field): what the host does with the two words in seg_checksum_locked, with the two constants that depend on the buffer's
// length alone made there.  A thread per buffer.
__global__ __launch_bounds__(256) void k_crc32_put(const unsigned int* __restrict__ acc, const ZesCrcPut* __restrict__ puts, uint32_t count,
                                                  uint8_t* __restrict__ out) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= count) return;
  const ZesCrcPut p = puts[q];
  const uint32_t crc = crc_mulmod(p.mul, acc[2 * (size_t)q]) ^ acc[2 * (size_t)q + 1] ^ p.add;
  uint8_t* d = out + p.dst;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) d[k] = (uint8_t)(crc >> (8 * (3 - k)));
}
