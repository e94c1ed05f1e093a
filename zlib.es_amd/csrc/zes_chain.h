// zes_chain.h — the acceptance rule of the block-parallel inflate tier (T1), written once for the device
// (k_inf_chain, k_inf_chain_range) and the host (the walk on the page-locked mirror, zes_stage_chain).
//
// The rule.  The block decoder has decoded one block per candidate start (rank order = ascending start bit) and left
// a ZesCandRes for each.  The output is accepted when candidate 0 is the stream's first block, every block of the chain
// decoded, every non-final block gave exactly ZES_BLK bytes and ends on the bit the next one starts at, and the first
// final block closes the chain.  Chain member k sitting at candidate k is the fast form; with false candidates between
// the blocks the chain is followed end bit -> next start, and the slots behind a false candidate have to move.
// Plain C++ as well as HIP: nothing here touches a device.
#pragma once
#include "zes_kernels.h"

#ifdef __HIPCC__
#define ZES_HD __host__ __device__
#else
#define ZES_HD
#endif

// ZesCandRes::flags
#define ZES_CAND_OK 1u     // the block decoded to its end-of-block symbol
#define ZES_CAND_FINAL 2u  // its header has BFINAL set

// One buffer's candidates.  The device lists hold start bit - 16 (bias 16), the host's mirror the start bit (bias 0).
struct ZesChainView {
  const uint32_t* start;
  const ZesCandRes* res;
  uint32_t n;  // candidates in the list: min(count, cap)
  uint32_t bias;
};
// the bit candidate k's block starts at
ZES_HD static inline uint64_t zes_chain_start(const ZesChainView& v, uint32_t k) { return (uint64_t)v.start[k] + v.bias; }

// Is there a chain to look at?  Not with no candidates, no work items (the buffer was left out: its results would be
// stale), a count above the cap (another encoder's stream), more candidates than work items were launched, or a list
// that does not begin at the stream's first block.
ZES_HD static inline bool zes_chain_enter(const ZesChainView& v, uint32_t count, uint32_t cap, uint32_t nwork, uint64_t first_bit) {
  return v.n != 0 && nwork != 0 && count <= cap && v.n <= nwork && zes_chain_start(v, 0) == first_bit;
}
// a non-final block of the chain, by itself: decoded, exactly one slot
ZES_HD static inline bool zes_chain_whole(const ZesCandRes& r) { return (r.flags & ZES_CAND_OK) && r.out_len == ZES_BLK; }
// a non-final block r of the chain, followed by candidate nxt: whole, nxt exists and starts on r's end bit
ZES_HD static inline bool zes_chain_link(const ZesChainView& v, const ZesCandRes& r, uint32_t nxt) {
  return zes_chain_whole(r) && nxt < v.n && zes_chain_start(v, nxt) == r.end_bit;
}
// the block that closes a chain: decoded and final
ZES_HD static inline bool zes_chain_closes(const ZesCandRes& r) {
  return (r.flags & (ZES_CAND_OK | ZES_CAND_FINAL)) == (ZES_CAND_OK | ZES_CAND_FINAL);
}

// a block of an accepted chain decoded again into its own slot (the slot repair): still whole, the chain's last one
// still decoded and no longer than a slot
ZES_HD static inline bool zes_chain_redone(const ZesCandRes& r, bool last) {
  return last ? (r.flags & ZES_CAND_OK) && r.out_len <= ZES_BLK : zes_chain_whole(r);
}

// The chain followed serially from candidate 0, end bit -> next start (binary search: the list ascends).  true: it
// closes; *total = its bytes, *len = its blocks, map[k] = the candidate of chain member k (map may be null).
ZES_HD static inline bool zes_chain_walk(const ZesChainView& v, uint32_t* map, uint64_t* total, uint32_t* len) {
  uint32_t j = 0, k = 0;
  uint64_t t = 0;
  for (;;) {
    const ZesCandRes r = v.res[j];
    if (map) map[k] = j;
    k++;
    t += r.out_len;
    if (zes_chain_closes(r)) break;
    uint32_t lo = j + 1, hi = v.n;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (zes_chain_start(v, mid) < r.end_bit) lo = mid + 1; else hi = mid;
    }
    if (!zes_chain_link(v, r, lo)) return false;
    j = lo;
  }
  *total = t;
  *len = k;
  return true;
}

// The whole rule on one thread (the host's form; k_inf_chain runs the fast check over 256 threads and is otherwise the
// same).  status 0: accepted, aux = the closing candidate + 1; 2: accepted, the slots are shifted, aux = the chain's
// length; 1: declined.  map (may be null): the chain, for status 0 and 2.
ZES_HD static inline ZesRes zes_chain_decide(const ZesChainView& v, uint32_t count, uint32_t cap, uint32_t nwork, uint64_t first_bit,
                                             uint32_t* map) {
  ZesRes res;
  res.status = 1;
  res.out_len = 0;
  res.aux = 0;
  if (!zes_chain_enter(v, count, cap, nwork, first_bit)) return res;
  // fast check: chain member k is candidate k, the first closing candidate closes the chain
  uint32_t K = 0;
  while (K < v.n && !zes_chain_closes(v.res[K])) K++;
  bool fast = K < v.n;
  uint64_t total = 0;
  for (uint32_t k = 0; fast && k <= K; k++) {
    total += v.res[k].out_len;
    if (k < K && !zes_chain_link(v, v.res[k], k + 1)) fast = false;
    if (map) map[k] = k;
  }
  if (fast) {
    res.status = 0;
    res.out_len = total;
    res.aux = K + 1;  // (its end bit is where the stream ends)
    return res;
  }
  uint32_t len;
  if (!zes_chain_walk(v, map, &total, &len)) return res;
  res.status = 2;
  res.out_len = total;
  res.aux = len;
  return res;
}
