// zes_png.hip — device pieces of the PNG reader (zes_api.hip: png_decode_core; include/zes.h: "PNG images").
//
//   k_png_walk      one lane per file follows the chunk chain from byte 8 and judges the file by the file rule of
//                   include/zes.h — the restatement of zes_api.hip's png_rule, which the host forms call.  It leaves a
//                   ZesPngHead per file (the IHDR fields, the counts, where PLTE and tRNS lie, the verdict) and one
//                   ZesPngChunk per chunk in the file's share of a table; chunks beyond the share are counted and not
//                   stored, and the host then launches once more with the shares the first launch counted.  Bytes are read
//                   one by one: a file and its chunks lie at any alignment, and the chain is serial anyway.
//   k_png_unfilter  the scanline filters undone (PNG specification, 9.2), the batch in one launch.  Rows are cut into bands
//                   of 64 and a wave is launched per (image, band).  A band is a restart when it is the image's first or
//                   its first row's filter is None or Sub: such a row does not read the row above.  The wave of a restart
//                   band decodes it and goes on through the bands behind it up to the next restart band or the image's
//                   end; the wave of any other band reads that one filter byte and exits.  So every band has one owner,
//                   found without a list, a queue, an atomic or a wait.
//                   Inside a band lane j owns row r0 + j, one filter unit (bpp bytes) behind the lane above: at step t it
//                   reconstructs unit t - j.  Left is its own last result; up is what lane j - 1 made one step ago, and
//                   upper-left what it made two steps ago: one __shfl_up a step, the value of the step before kept in a
//                   register.  Lane 0's row above is zeros for image row 0, and otherwise the last row of the band before,
//                   which this same wave has stored: it reads it back from the output.
//                   A lane reads its row (at any alignment in the slot: the stride is rowbytes + 1) as aligned dwords into
//                   a shift register, the first one shifted past the bytes in front of the row — the slot is the call's own
//                   scratch, padded on both sides, so a dword may reach over the row's ends.  It writes through a second
//                   shift register: single bytes up to the output's first dword boundary, whole dwords from there, single
//                   bytes for what is left at the row's end, so that no byte outside the row is written.
//   k_png_expand    the scanlines of the batch turned into 8-bit RGBA pixels by the conversion rule of include/zes.h, in one
//                   launch: a streaming kernel, a workgroup per (image, tile of rows), a lane four pixels a step — source
//                   bytes fetched as aligned 16-byte groups and shifted into place, results stored as 16-byte groups from
//                   the first 16-byte boundary of a row's output.  It stands behind the unfilter kernel.
//   k_png_deinterlace  ZES_F_PNG_INTERLACED: the seven Adam7 passes of an image, which k_png_unfilter has unfiltered as images
//                   of their own into a scratch slot, gathered into the image's scanlines in one launch for the batch: a
//                   gather driven by the output, a workgroup per (image, tile of output rows), every output byte stored
//                   once as part of a 16-byte group, a dword or (at a row's ends) a byte.  It stands at the end of this file.
#include "../../include/zes.h"
#include "zes_common.h"
#include "zes_kernels.h"

#include <type_traits>

namespace {
__device__ __forceinline__ uint32_t png_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }

constexpr uint32_t PNG_IHDR = 0x49484452u, PNG_IDAT = 0x49444154u, PNG_PLTE = 0x504c5445u, PNG_IEND = 0x49454e44u, PNG_TRNS = 0x74524e53u;

// The file rule on p[0, c): the verdict, h filled as far as the walk got.  (zes_api.hip: png_rule is the same, step by step.)
__device__ int png_walk_file(const uint8_t* __restrict__ p, uint64_t c, ZesPngHead& h, ZesPngChunk* __restrict__ tab, uint32_t cap) {
  if (c < 8 || png_be32(p) != 0x89504e47u || png_be32(p + 4) != 0x0d0a1a0au) return ZES_E_PNG;
  uint64_t pos = 8;
  uint32_t k = 0;
  bool idat = false, closed = false, plte = false, trns = false;
  const uint64_t steps = c / 12;  // a chunk takes 12 bytes at least
  for (uint64_t s = 0; s < steps; s++) {
    if (c - pos < 12) return ZES_E_PNG;  // (pos == c: the chain ends without IEND)
    const uint32_t L = png_be32(p + pos), type = png_be32(p + pos + 4);
    if (L > 0x7fffffffu) return ZES_E_PNG;
    for (uint32_t b = 0; b < 4; b++)
      if ((((type >> (8 * b)) & 0xDFu) - 'A') >= 26u || ((type >> (8 * b)) & 0x80u)) return ZES_E_PNG;
    if (L > c - pos - 12) return ZES_E_PNG;
    const uint8_t* d = p + pos + 8;
    if (k < cap) {
      ZesPngChunk r;
      r.pos = pos;
      r.len = L | (type == PNG_IDAT ? ZES_PNG_IDAT : 0u);
      r.crc = png_be32(d + L);
      tab[k] = r;
    }
    h.nchunks = ++k;
    if (k == 1) {
      if (type != PNG_IHDR || L != 13) return ZES_E_PNG;
      h.width = png_be32(d);
      h.height = png_be32(d + 4);
      h.depth = d[8];
      h.colour = d[9];
      h.interlace = d[12];
      if (h.width - 1 > 0x7ffffffeu || h.height - 1 > 0x7ffffffeu) return ZES_E_PNG;
      const uint32_t dp = h.depth;
      bool ok;
      switch (h.colour) {
        case 0: ok = dp == 1 || dp == 2 || dp == 4 || dp == 8 || dp == 16; break;
        case 3: ok = dp == 1 || dp == 2 || dp == 4 || dp == 8; break;
        case 2: case 4: case 6: ok = dp == 8 || dp == 16; break;
        default: ok = false;
      }
      if (!ok || d[10] != 0 || d[11] != 0 || h.interlace > 1) return ZES_E_PNG;
    } else if (type == PNG_IHDR) {
      return ZES_E_PNG;
    } else if (type == PNG_IDAT) {
      if (closed || (h.colour == 3 && !plte)) return ZES_E_PNG;
      idat = true;
      h.idat_count++;
      h.idat_bytes += L;
    } else {
      closed = idat;
      if (type == PNG_PLTE) {
        if (plte || idat || L % 3 || L < 3 || L > 768) return ZES_E_PNG;
        plte = true;
        h.plte_pos = pos + 8;
        h.plte_len = L;
      } else if (type == PNG_IEND) {
        if (L != 0 || pos + 12 != c || !idat) return ZES_E_PNG;
        const uint32_t ch = h.colour == 2 ? 3u : h.colour == 4 ? 2u : h.colour == 6 ? 4u : 1u;
        const uint64_t rowbytes = ((uint64_t)h.width * (ch * h.depth) + 7) / 8;
        return 1 + rowbytes > 0xFFFFFFFFull / h.height ? ZES_E_UNSUPPORTED : ZES_OK;
      } else if (!(type & 0x20000000u)) {
        return ZES_E_UNSUPPORTED;  // a critical chunk this reader does not know
      } else if (type == PNG_TRNS && !idat && !trns) {
        trns = true;
        h.trns_pos = pos + 8;
        h.trns_len = L;
      }
    }
    pos += 12ull + L;
  }
  return ZES_E_PNG;
}
}  // namespace

__global__ __launch_bounds__(64) void k_png_walk(const uint8_t* __restrict__ d_in, const ZesPngFile* __restrict__ files, uint32_t count,
                                                ZesPngHead* __restrict__ heads, ZesPngChunk* __restrict__ tab) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= count) return;
  const ZesPngFile f = files[i];
  ZesPngHead h;
  h.status = 0, h.width = h.height = 0, h.depth = h.colour = h.interlace = h.pad = 0;
  h.nchunks = h.idat_count = h.plte_len = h.trns_len = 0;
  h.idat_bytes = h.plte_pos = h.trns_pos = 0;
  h.status = png_walk_file(d_in + f.in_off, f.in_len, h, tab + f.tab_base, f.tab_cap);
  heads[i] = h;
}

namespace {
// a filter unit in a register, and the shift registers that hold a row's bytes on their way in and out
template <int BPP>
struct PngUnit {
  using T = typename std::conditional<(BPP <= 4), uint32_t, uint64_t>::type;
  using W = typename std::conditional<(BPP <= 4), uint64_t, unsigned __int128>::type;
  static constexpr T MASK = BPP == (int)sizeof(T) ? ~(T)0 : (((T)1 << (8 * (BPP % (int)sizeof(T)))) - 1);
};

// A row's bytes as aligned dwords: at most 3 + 4 bytes wait in front of a take of up to 4 (uint64_t), 7 + 4 in front of one
// of 6 or 8 (128 bits).  The last dword read is the one that holds the row's last byte.
template <int BPP>
struct PngIn {
  using U = PngUnit<BPP>;
  const uint32_t* next;
  typename U::W buf;
  uint32_t avail;
  __device__ __forceinline__ void open(const uint8_t* p) {
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    next = reinterpret_cast<const uint32_t*>(p - sh);
    buf = (typename U::W)(*next++ >> (8 * sh));
    avail = 4 - sh;
  }
  __device__ __forceinline__ typename U::T take() {
    while (avail < (uint32_t)BPP) {
      buf |= (typename U::W)(*next++) << (8 * avail);
      avail += 4;
    }
    const typename U::T v = (typename U::T)buf & U::MASK;
    buf >>= 8 * BPP;
    avail -= BPP;
    return v;
  }
};

// A row's results: bytes until the place is a dword boundary, dwords from there (at most 3 bytes wait behind a put), and
// the bytes that are left at the row's end.  Only bytes of the row are ever stored.
template <int BPP>
struct PngOut {
  using U = PngUnit<BPP>;
  uint8_t* p;
  typename U::W buf;
  uint32_t n;
  __device__ __forceinline__ void open(uint8_t* to) { p = to, buf = 0, n = 0; }
  __device__ __forceinline__ void put(typename U::T v) {
    buf |= (typename U::W)v << (8 * n);
    n += BPP;
    while (n) {
      if (((uintptr_t)p & 3u) == 0) {
        if (n < 4) break;
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)buf;
        p += 4, buf >>= 32, n -= 4;
      } else {
        *p = (uint8_t)buf;
        p += 1, buf >>= 8, n -= 1;
      }
    }
  }
  __device__ __forceinline__ void flush() {
    for (; n; n--, buf >>= 8) *p++ = (uint8_t)buf;
  }
};

// Recon(x) = Filt(x) + predictor, byte by byte (PNG specification, 9.2 and 9.4): a left, b up, c upper-left.  Every lane
// computes every predictor it may need and selects by its own row's filter type, so rows of different types share the
// steps; the Paeth arithmetic runs only when a row of the band asks for it.
template <int BPP>
__device__ __forceinline__ typename PngUnit<BPP>::T png_recon(typename PngUnit<BPP>::T raw, typename PngUnit<BPP>::T a, typename PngUnit<BPP>::T b,
                                                               typename PngUnit<BPP>::T c, uint32_t ft, bool paeth) {
  using T = typename PngUnit<BPP>::T;
  T out = 0;
#pragma unroll
  for (int k = 0; k < BPP; k++) {
    const int x = (int)((raw >> (8 * k)) & 255u), A = (int)((a >> (8 * k)) & 255u), B = (int)((b >> (8 * k)) & 255u), C = (int)((c >> (8 * k)) & 255u);
    int pred = ft == 1 ? A : ft == 2 ? B : ft == 3 ? (A + B) >> 1 : 0;
    if (paeth) {
      const int pa = abs(B - C), pb = abs(A - C), pc = abs(A + B - 2 * C);
      const int pp = (pa <= pb && pa <= pc) ? A : (pb <= pc ? B : C);  // ties: a, then b, then c
      pred = ft == 4 ? pp : pred;
    }
    out |= (T)((uint32_t)(x + pred) & 255u) << (8 * k);
  }
  return out;
}

// One band: rows [r0, min(r0 + 64, height)), lane j the row r0 + j.  Called by a whole wave.
template <int BPP>
__device__ __forceinline__ void png_band(const uint8_t* __restrict__ src, uint8_t* dst, uint32_t r0, uint32_t height, uint32_t rowbytes, uint32_t lane,
                                         uint32_t* __restrict__ bad) {
  using T = typename PngUnit<BPP>::T;
  const uint32_t npix = rowbytes / BPP;  // (rowbytes is a multiple of bpp: bpp is 1 below 8 bits a sample)
  const uint32_t row = r0 + lane;
  const bool live = row < height;
  uint32_t ft = 0;
  PngIn<BPP> in, up;
  PngOut<BPP> out;
  if (live) {
    const uint8_t* s = src + (uint64_t)row * (rowbytes + 1ull);
    ft = s[0];
    in.open(s + 1);
    out.open(dst + (uint64_t)row * rowbytes);
  }
  if (ft > 4) {  // not a filter type: the image is ZES_E_PNG, its range unspecified
    *bad = 1u;
    ft = 0;
  }
  // lane 0 of a restart band has filter None or Sub, or the image's row 0 above it: it reads no row (the last row of the
  // band before is then another wave's, and may not be there yet)
  const bool has_up = lane == 0 && r0 > 0 && ft >= 2;
  if (has_up) up.open(dst + (uint64_t)(r0 - 1) * rowbytes);
  const bool paeth = __ballot(ft == 4) != 0;
  const uint32_t steps = npix + min(height - r0, ZES_PNG_BAND) - 1;
  T res = 0, bl = 0;
  for (uint32_t t = 0; t < steps; t++) {
    T b = __shfl_up(res, 1);  // the lane above, one step ago: the unit above mine
    if (lane == 0) b = 0;
    const uint32_t pix = t - lane;
    if (live && t >= lane && pix < npix) {
      if (has_up) b = up.take();
      res = png_recon<BPP>(in.take(), res, b, bl, ft, paeth);
      out.put(res);
    }
    bl = b;  // the lane above, two steps ago by the next step: the unit above and to the left
  }
  if (live) out.flush();
}
}  // namespace

__global__ __launch_bounds__(ZES_PNG_UNF_THREADS) void k_png_unfilter(const uint8_t* __restrict__ slots, uint8_t* dst, uint8_t* passes,
                                                                    const ZesPngJob* __restrict__ jobs, uint32_t njobs, uint32_t nbands,
                                                                    uint32_t* __restrict__ bad) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (ZES_PNG_UNF_THREADS / 64u) + threadIdx.x / 64u));
  if (wave >= nbands) return;
  uint32_t lo = 0, hi = njobs;  // the last image whose first band is not behind this one
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (jobs[mid].first_band <= wave) lo = mid;
    else hi = mid;
  }
  ZesPngJob j = jobs[lo];
  const uint8_t* src = slots + j.src_off;
  uint8_t* out = ((j.bpp & ZES_PNG_TO_PASSES) ? passes : dst) + j.dst_off;  // (a pass of an Adam7 image is an image of its own)
  j.bpp &= ~ZES_PNG_TO_PASSES;
  const uint32_t nb = (j.height + ZES_PNG_BAND - 1) / ZES_PNG_BAND;
  uint32_t band = wave - j.first_band;
  auto restart = [&](uint32_t bnd) { return bnd == 0 || src[(uint64_t)bnd * ZES_PNG_BAND * (j.rowbytes + 1ull)] <= 1; };
  if (!restart(band)) return;  // the wave of a restart band in front decodes this one
  for (;;) {
    const uint32_t r0 = band * ZES_PNG_BAND;
    switch (j.bpp) {
      case 1: png_band<1>(src, out, r0, j.height, j.rowbytes, lane, bad + lo); break;
      case 2: png_band<2>(src, out, r0, j.height, j.rowbytes, lane, bad + lo); break;
      case 3: png_band<3>(src, out, r0, j.height, j.rowbytes, lane, bad + lo); break;
      case 4: png_band<4>(src, out, r0, j.height, j.rowbytes, lane, bad + lo); break;
      case 6: png_band<6>(src, out, r0, j.height, j.rowbytes, lane, bad + lo); break;
      default: png_band<8>(src, out, r0, j.height, j.rowbytes, lane, bad + lo); break;
    }
    if (++band >= nb || restart(band)) break;
    // Lane 0 of the next band reads the row that lane 63 has just stored.  Writer and reader are lanes of one wave, so
    // they sit on one compute unit and go through the same vector cache: a workgroup-scope fence makes the wave wait until
    // its stores have left for that cache before a later load is issued, and keeps the compiler from moving either across
    // it.  No other wave reads or writes these rows, so no wider scope is needed.
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
}

// ---- k_png_expand: scanlines to 8-bit RGBA (include/zes.h: "The conversion rule") ----
namespace {
constexpr int pngx_channels(int colour) { return colour == 2 ? 3 : colour == 4 ? 2 : colour == 6 ? 4 : 1; }

// The nb <= NB bytes at `a` (any alignment) as little-endian dwords w[0 .. ceil(NB / 4)): read as the aligned 16-byte groups
// that hold them and nothing else, then moved down by a's place in its group — whole dwords by selection, the bytes left
// by a funnel shift.  Bytes behind the nb are zeros or whatever stands in the last group read.
template <int NB>
__device__ __forceinline__ void pngx_load(const uint8_t* a, uint32_t nb, uint32_t (&w)[(NB + 3) / 4]) {
  constexpr int NQ = (NB + 30) / 16, NW = (NB + 3) / 4;
  const uint32_t off = (uint32_t)((uintptr_t)a & 15u);
  const uint4* q = reinterpret_cast<const uint4*>(a - off);
  uint32_t d[4 * NQ + 1];
#pragma unroll
  for (int k = 0; k < NQ; k++) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (16u * k < off + nb) v = q[k];
    d[4 * k] = v.x, d[4 * k + 1] = v.y, d[4 * k + 2] = v.z, d[4 * k + 3] = v.w;
  }
  d[4 * NQ] = 0u;
  const uint32_t dsh = off >> 2, bsh = 8u * (off & 3u);
  uint32_t t[NW + 1];
#pragma unroll
  for (int k = 0; k <= NW; k++) t[k] = dsh == 0 ? d[k] : dsh == 1 ? d[k + 1] : dsh == 2 ? d[k + 2] : d[k + 3];
#pragma unroll
  for (int k = 0; k < NW; k++) w[k] = (uint32_t)((((uint64_t)t[k + 1] << 32) | t[k]) >> bsh);
}

template <int NW>
__device__ __forceinline__ uint32_t pngx_byte(const uint32_t (&w)[NW], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// sample i (counted in samples from the window's first byte) of depth 8 or 16 at its full depth, and any sample as 8 bits
template <int DEPTH, int NW>
__device__ __forceinline__ uint32_t pngx_sample(const uint32_t (&w)[NW], int i) {
  if (DEPTH == 16) return pngx_byte(w, 2 * i) << 8 | pngx_byte(w, 2 * i + 1);
  return pngx_byte(w, i);
}
template <int DEPTH>
__device__ __forceinline__ uint32_t pngx_to8(uint32_t s) {
  return DEPTH == 1 ? s * 255u : DEPTH == 2 ? s * 85u : DEPTH == 4 ? s * 17u : DEPTH == 8 ? s : s >> 8;
}

// A tile: rows [r0, r1) of one image.  A row's pixels go in groups: the 1 to 4 pixels in front of the first 16-byte boundary
// of the row's output are group 0, then four pixels a group.  So a whole group behind group 0 is one aligned 16-byte store;
// group 0 and the row's last group store whole pixels (dwords).  An output that is not 4-byte aligned takes the slow path:
// the same groups, every pixel stored as four single bytes.
// A row has at most G groups (one fewer where its boundary falls late: the slot is then empty).  The tile's rows * G slots
// are taken by the threads in order, ZES_PNGX_THREADS a step: consecutive lanes have consecutive groups of a row, a narrow
// image keeps every lane busy, and a thread finds its next slot by two additions — the one division by G a tile is by a
// value the workgroup shares.
template <int COLOUR, int DEPTH>
__device__ __forceinline__ void pngx_tile(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const ZesPngxJob& j, uint32_t r0, uint32_t r1,
                                          const uint32_t* pal, bool keyed, uint32_t k0, uint32_t k1, uint32_t k2) {
  constexpr int CH = pngx_channels(COLOUR), BITS = CH * DEPTH;
  constexpr int NB = BITS >= 8 ? BITS / 2 : BITS == 4 ? 3 : 2;  // bytes that four pixels touch at most
  constexpr int NW = (NB + 3) / 4;
  const uint32_t G = 1u + (j.width + 2u) / 4u, dr = ZES_PNGX_THREADS / G, dg = ZES_PNGX_THREADS % G;
  const bool words = ((uintptr_t)dst & 3u) == 0;
  uint32_t row = r0 + threadIdx.x / G, g = threadIdx.x % G;
  for (; row < r1; g += dg, row += dr + (g >= G ? 1u : 0u), g -= (g >= G ? G : 0u)) {
    const uint8_t* s = src + (uint64_t)row * j.rowbytes;
    uint8_t* o = dst + (uint64_t)row * j.width * 4ull;
    uint32_t first = 4u;
    if (words) {
      first = ((16u - (uint32_t)((uintptr_t)o & 15u)) & 15u) >> 2;
      if (first == 0) first = 4u;
    }
    const uint32_t p0 = g ? first + 4u * (g - 1u) : 0u;
    if (p0 < j.width) {
      const uint32_t p1 = min(j.width, first + 4u * g), n = p1 - p0;
      const uint64_t bit0 = (uint64_t)p0 * BITS, byte0 = bit0 >> 3;
      uint32_t w[NW];
      pngx_load<NB>(s + byte0, (uint32_t)((((uint64_t)p1 * BITS + 7u) >> 3) - byte0), w);
      uint32_t px[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        uint32_t c[4];
        if (BITS < 8) {  // one sample a pixel, the first one of a byte in its high bits
          const uint32_t bit = (uint32_t)(bit0 & 7u) + k * DEPTH;
          c[0] = (w[0] >> (8u * (bit >> 3) + 8u - DEPTH - (bit & 7u))) & ((1u << DEPTH) - 1u);
        } else {
#pragma unroll
          for (int q = 0; q < CH; q++) c[q] = pngx_sample<DEPTH>(w, k * CH + q);
        }
        if (COLOUR == 3) {
          px[k] = pal[c[0]];
        } else if (COLOUR == 0) {
          px[k] = pngx_to8<DEPTH>(c[0]) * 0x010101u | ((keyed && c[0] == k0) ? 0u : 0xFF000000u);
        } else if (COLOUR == 2) {
          px[k] = pngx_to8<DEPTH>(c[0]) | pngx_to8<DEPTH>(c[1]) << 8 | pngx_to8<DEPTH>(c[2]) << 16 |
                  ((keyed && c[0] == k0 && c[1] == k1 && c[2] == k2) ? 0u : 0xFF000000u);
        } else if (COLOUR == 4) {
          px[k] = pngx_to8<DEPTH>(c[0]) * 0x010101u | pngx_to8<DEPTH>(c[1]) << 24;
        } else {
          px[k] = pngx_to8<DEPTH>(c[0]) | pngx_to8<DEPTH>(c[1]) << 8 | pngx_to8<DEPTH>(c[2]) << 16 | pngx_to8<DEPTH>(c[3]) << 24;
        }
      }
      uint8_t* to = o + 4ull * p0;
      if (n == 4u && words && ((uintptr_t)to & 15u) == 0) {
        *reinterpret_cast<uint4*>(to) = make_uint4(px[0], px[1], px[2], px[3]);
      } else if (words) {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if ((uint32_t)k < n) reinterpret_cast<uint32_t*>(to)[k] = px[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if ((uint32_t)k < n) {
            to[4 * k] = (uint8_t)px[k], to[4 * k + 1] = (uint8_t)(px[k] >> 8);
            to[4 * k + 2] = (uint8_t)(px[k] >> 16), to[4 * k + 3] = (uint8_t)(px[k] >> 24);
          }
      }
    }
  }
}
}  // namespace

// A workgroup per (image, tile of rows); the tile's image by a binary search of the job table, as k_png_unfilter finds its
// band.  Colour type 3: the workgroup first builds the 256-entry RGBA table in LDS from the PLTE and tRNS bytes (read one
// by one: they lie at any byte of a file), entries behind the palette (0, 0, 0, 255); a pixel is then one LDS dword.
// Colour types 0 and 2: the tRNS key, compared with the stored samples at their full depth.  `aux` holds PLTE and tRNS.
__global__ __launch_bounds__(ZES_PNGX_THREADS) void k_png_expand(const uint8_t* __restrict__ lines, const uint8_t* __restrict__ aux, uint8_t* __restrict__ dst,
                                                                const ZesPngxJob* __restrict__ jobs, uint32_t njobs) {
  __shared__ uint32_t pal[256];
  const uint32_t tile = blockIdx.x;
  uint32_t lo = 0, hi = njobs;  // the last image whose first tile is not behind this one
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (jobs[mid].first_tile <= tile) lo = mid;
    else hi = mid;
  }
  const ZesPngxJob j = jobs[lo];
  const uint32_t r0 = (tile - j.first_tile) * j.tile_rows, r1 = min(j.height, r0 + j.tile_rows);  // (tile_rows * tiles < 2^32: the host's rule)
  if (r0 >= j.height) return;
  const uint8_t* src = lines + j.src_off;
  uint8_t* out = dst + j.dst_off;
  uint32_t k0 = 0, k1 = 0, k2 = 0;
  bool keyed = false;
  if (j.colour == 3) {
    const uint8_t *P = aux + j.plte_off, *T = aux + j.trns_off;
    const uint32_t i = threadIdx.x, entries = min((uint32_t)j.plte_len / 3u, 256u);
    uint32_t e = 0xFF000000u;
    if (i < entries) e = (uint32_t)P[3 * i] | (uint32_t)P[3 * i + 1] << 8 | (uint32_t)P[3 * i + 2] << 16 | (i < j.trns_len ? (uint32_t)T[i] : 255u) << 24;
    pal[i] = e;
    __syncthreads();
  } else if (j.colour == 0 && j.trns_len == 2) {
    const uint8_t* T = aux + j.trns_off;
    keyed = true, k0 = (uint32_t)T[0] << 8 | T[1];
  } else if (j.colour == 2 && j.trns_len == 6) {
    const uint8_t* T = aux + j.trns_off;
    keyed = true, k0 = (uint32_t)T[0] << 8 | T[1], k1 = (uint32_t)T[2] << 8 | T[3], k2 = (uint32_t)T[4] << 8 | T[5];
  }
#define PNGX_CASE(C, D) \
  case (C) * 32 + (D): pngx_tile<C, D>(src, out, j, r0, r1, pal, keyed, k0, k1, k2); break;
  switch (j.colour * 32u + j.depth) {
    PNGX_CASE(0, 1) PNGX_CASE(0, 2) PNGX_CASE(0, 4) PNGX_CASE(0, 8) PNGX_CASE(0, 16)
    PNGX_CASE(2, 8) PNGX_CASE(2, 16)
    PNGX_CASE(3, 1) PNGX_CASE(3, 2) PNGX_CASE(3, 4) PNGX_CASE(3, 8)
    PNGX_CASE(4, 8) PNGX_CASE(4, 16)
    PNGX_CASE(6, 8) PNGX_CASE(6, 16)
    default: break;  // (the host passes no other pair)
  }
#undef PNGX_CASE
}

// ---- k_png_deinterlace: the seven Adam7 passes gathered back into scanlines (include/zes.h: "Interlaced images") ----
namespace {
// Pass p = 1..7 holds the pixels (x0 + k * dx, y0 + m * dy); dx = 1 << sx, dy = 1 << sy, and x0 < dx, y0 < dy, so the
// pixel (x, y) of pass p is its pixel x >> sx of its row y >> sy.  A nibble a pass, pass 1 lowest.
constexpr uint32_t PNGD_SX = 0x0112233u, PNGD_SY = 0x1122333u, PNGD_X0 = 0x0102040u;
struct PngdPass {
  const uint8_t* base;  // its unfiltered rows, 16-byte aligned
  uint32_t prb;         // bytes of one of them
  uint32_t pad;
};
// the pass of a pixel of an even row (an odd row is pass 7 from end to end)
__device__ __forceinline__ uint32_t pngd_pass(uint32_t x, uint32_t y) {
  return (x & 1u) ? 6u : (y & 2u) ? 5u : (x & 2u) ? 4u : (y & 4u) ? 3u : (x & 4u) ? 2u : 1u;
}
// where pixel (x, y), y even, begins in its pass, for pixels of B whole bytes
template <int B>
__device__ __forceinline__ const uint8_t* pngd_at(const PngdPass* ps, uint32_t x, uint32_t y) {
  const uint32_t p = pngd_pass(x, y), q = 4u * (p - 1u);
  return ps[p].base + (uint64_t)(y >> ((PNGD_SY >> q) & 7u)) * ps[p].prb + (uint64_t)(x >> ((PNGD_SX >> q) & 7u)) * B;
}
// output byte o of the even row y, at depths below 8: 8 / D pixels from up to four passes, the first one in the high
// bits; the places behind the row's last pixel stay zeros
template <int D>
__device__ __forceinline__ uint32_t pngd_sub(const PngdPass* ps, uint32_t width, uint32_t y, uint32_t o) {
  constexpr uint32_t PPB = 8 / D;
  uint32_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < PPB; k++) {
    const uint32_t x = o * PPB + k;
    if (x < width) {
      const uint32_t p = pngd_pass(x, y), q = 4u * (p - 1u);
      const uint64_t bit = (uint64_t)(x >> ((PNGD_SX >> q) & 7u)) * D;
      const uint32_t byte = ps[p].base[(uint64_t)(y >> ((PNGD_SY >> q) & 7u)) * ps[p].prb + (bit >> 3)];
      v |= ((byte >> (8u - D - (uint32_t)(bit & 7u))) & ((1u << D) - 1u)) << (8u - D - k * D);
    }
  }
  return v;
}
// The output bytes [wo, wo + 4) of the even row y as a little-endian dword; those outside [0, rb) are zeros.  Pixels of 2,
// 4 and 8 bytes are fetched whole where the dword begins on one (a pass begins on a 16-byte boundary and its rows are
// whole pixels, so such a pixel is aligned to its own size, 4 at most); everything else goes byte by byte.
template <int BITS>
__device__ __forceinline__ uint32_t pngd_word(const PngdPass* ps, uint32_t width, uint32_t rb, uint32_t y, int64_t wo) {
  if ((BITS == 32 || BITS == 64) && wo >= 0 && (wo & 3) == 0) {  // (rb is a multiple of 4: the dword ends inside the row)
    const uint32_t x = (uint32_t)((uint64_t)wo / (BITS / 8));
    return *reinterpret_cast<const uint32_t*>(pngd_at<BITS / 8>(ps, x, y) + ((uint64_t)wo % (BITS / 8)));
  }
  if (BITS == 16 && wo >= 0 && (wo & 1) == 0) {
    const uint32_t x = (uint32_t)((uint64_t)wo / 2);
    uint32_t v = *reinterpret_cast<const uint16_t*>(pngd_at<2>(ps, x, y));
    if (wo + 2 < (int64_t)rb) v |= (uint32_t)*reinterpret_cast<const uint16_t*>(pngd_at<2>(ps, x + 1u, y)) << 16;
    return v;
  }
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    const int64_t o = wo + b;
    if (o >= 0 && o < (int64_t)rb) {
      uint32_t byte;
      if (BITS < 8) {
        byte = pngd_sub<(BITS < 8 ? BITS : 1)>(ps, width, y, (uint32_t)o);
      } else {
        constexpr uint32_t B = BITS < 8 ? 1 : BITS / 8;
        byte = pngd_at<(int)B>(ps, (uint32_t)o / B, y)[(uint32_t)o % B];
      }
      v |= byte << (8 * b);
    }
  }
  return v;
}
// the aligned dword at `a`, of which only bytes inside [lo, hi) are read: the others count as zeros
__device__ __forceinline__ uint32_t pngd_ldw(const uint8_t* a, const uint8_t* lo, const uint8_t* hi) {
  if (a >= lo && a + 4 <= hi) return *reinterpret_cast<const uint32_t*>(a);
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; b++)
    if (a + b >= lo && a + b < hi) v |= (uint32_t)a[b] << (8 * b);
  return v;
}

// A tile: output rows [r0, r1) of one image.  A row's output is cut at the 16-byte boundaries of its addresses into units:
// a thread makes a unit's four dwords in registers and stores them as one 16-byte group; the unit in front of the row's
// first boundary and the one that holds its end store their whole dwords and, around those, single bytes.  So every byte of
// the row is stored once, and none outside it.  The tile's rows * G unit slots are taken by the threads in order, as
// k_png_expand takes its groups: consecutive lanes have consecutive units of a row.
// An odd row is row y / 2 of pass 7 as it stands: a dword of it is two aligned dwords of the pass and a funnel shift, no
// arithmetic per pixel.  Its last byte loses the pad bits of the file (depths below 8).
template <int BITS>
__device__ __forceinline__ void pngd_tile(const PngdPass* ps, uint8_t* dst, const ZesPngDeintJob& j, uint32_t r0, uint32_t r1) {
  const uint32_t rb = j.rowbytes;
  const uint32_t G = rb / 16u + 2u, dr = ZES_PNGD_THREADS / G, dg = ZES_PNGD_THREADS % G;
  const uint8_t *p7lo = ps[7].base, *p7hi = p7lo + (uint64_t)(j.height >> 1) * rb;
  const uint32_t used = (uint32_t)((((uint64_t)j.width * BITS - 1u) & 7u) + 1u);  // bits of a row's last byte that are pixels
  const uint32_t padmask = ~(((0xFFu >> used) & 0xFFu) << 24);                    // (for a dword whose top byte is that one)
  uint32_t row = r0 + threadIdx.x / G, g = threadIdx.x % G;
  for (; row < r1; g += dg, row += dr + (g >= G ? 1u : 0u), g -= (g >= G ? G : 0u)) {
    uint8_t* o = dst + (uint64_t)row * rb;
    const int64_t u0 = 16ll * g - (int64_t)((uintptr_t)o & 15u);  // the unit's first byte, counted from the row's
    if (u0 >= (int64_t)rb) continue;
    const bool odd = (row & 1u) != 0;
    const uint8_t* s7 = p7lo + (uint64_t)(row >> 1) * rb;
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int64_t wo = u0 + 4 * k;
      w[k] = 0;
      if (wo > -4 && wo < (int64_t)rb) {
        if (odd) {
          const uint8_t* s = s7 + wo;
          const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
          const uint32_t a = pngd_ldw(s - sh, p7lo, p7hi);
          const uint32_t b = sh ? pngd_ldw(s - sh + 4, p7lo, p7hi) : 0u;
          w[k] = (uint32_t)((((uint64_t)b << 32) | a) >> (8u * sh));
          const int64_t last = (int64_t)rb - 1 - wo;  // the row's last byte, counted from this dword's first
          if (BITS < 8 && last >= 0 && last < 4) w[k] &= padmask >> (8 * (3 - (int)last));
        } else {
          w[k] = pngd_word<BITS>(ps, j.width, rb, row, wo);
        }
      }
    }
    uint8_t* to = o + u0;
    if (u0 >= 0 && u0 + 16 <= (int64_t)rb) {
      *reinterpret_cast<uint4*>(to) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int64_t wo = u0 + 4 * k;
        if (wo >= 0 && wo + 4 <= (int64_t)rb) {
          *reinterpret_cast<uint32_t*>(to + 4 * k) = w[k];
        } else {
#pragma unroll
          for (int b = 0; b < 4; b++)
            if (wo + b >= 0 && wo + b < (int64_t)rb) to[4 * k + b] = (uint8_t)(w[k] >> (8 * b));
        }
      }
    }
  }
}
}  // namespace

// A workgroup per (image, tile of output rows); the tile's image by a binary search of the job table, as k_png_expand finds
// its tile.  The seven passes' places and row sizes go to LDS once a workgroup: a pixel's pass is then an index.
__global__ __launch_bounds__(ZES_PNGD_THREADS) void k_png_deinterlace(const uint8_t* __restrict__ passes, uint8_t* __restrict__ dst,
                                                                     const ZesPngDeintJob* __restrict__ jobs, uint32_t njobs,
                                                                     const uint32_t* __restrict__ bad) {
  __shared__ PngdPass ps[8];
  const uint32_t tile = blockIdx.x;
  uint32_t lo = 0, hi = njobs;  // the last image whose first tile is not behind this one
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (jobs[mid].first_tile <= tile) lo = mid;
    else hi = mid;
  }
  const ZesPngDeintJob j = jobs[lo];
  const uint32_t r0 = (tile - j.first_tile) * j.tile_rows, r1 = min(j.height, r0 + j.tile_rows);  // (tile_rows * tiles < 2^32: the host's rule)
  if (r0 >= j.height) return;
  for (uint32_t q = 0; q < j.ujobs; q++)
    if (bad[j.ujob0 + q]) return;  // a filter byte above 4 in one of its passes: ZES_E_PNG, nothing of it is written
  if (threadIdx.x < 7u) {
    const uint32_t q = 4u * threadIdx.x, sx = (PNGD_SX >> q) & 7u, x0 = (PNGD_X0 >> q) & 7u;
    const uint64_t pw = j.width > x0 ? ((uint64_t)(j.width - x0) + (1u << sx) - 1u) >> sx : 0u;
    PngdPass p;
    p.base = passes + j.src_off + 16ull * j.pass_off16[threadIdx.x];
    p.prb = (uint32_t)((pw * j.bits + 7u) >> 3);
    p.pad = 0;
    ps[threadIdx.x + 1u] = p;
  }
  __syncthreads();
  uint8_t* out = dst + j.dst_off;
  switch (j.bits) {
    case 1: pngd_tile<1>(ps, out, j, r0, r1); break;
    case 2: pngd_tile<2>(ps, out, j, r0, r1); break;
    case 4: pngd_tile<4>(ps, out, j, r0, r1); break;
    case 8: pngd_tile<8>(ps, out, j, r0, r1); break;
    case 16: pngd_tile<16>(ps, out, j, r0, r1); break;
    case 24: pngd_tile<24>(ps, out, j, r0, r1); break;
    case 32: pngd_tile<32>(ps, out, j, r0, r1); break;
    case 48: pngd_tile<48>(ps, out, j, r0, r1); break;
    default: pngd_tile<64>(ps, out, j, r0, r1); break;
  }
}
