// zes_api.hip — host side of the C-ABI declared in include/zes.h.
//
// One context per GPU the process drives (zes_init(device): one; zes_init_devices(n): several), each with a private
// HIP stream for its launches, its own pooled device scratch, which only grows until zes_trim, and its own lock.
// No CPU fallback exists here: every compute entry point needs a working gfx950 device and returns ZES_E_DEVICE otherwise.
#include "../../include/zes.h"
#include "zes_kernels.h"
#include "zes_chain.h"
#include "zes_gzbatch.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <functional>
#include <future>
#include <initializer_list>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

extern "C" int zes_gen(uint8_t* out, uint64_t n, uint32_t kind, uint32_t seed);

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  uint32_t gen = 0;  // how often its memory has been given back (release): what a note about its contents records (SurvList)
};

struct KTime {
  double ms = 0;
  uint32_t launches = 0;
};

// ---- the page-locked area of a context ----
// One block per context, allocated at init and kept until shutdown: the host writes tables into it for the copy engines,
// read-backs land in it, and a few kernels write into it through its device address (Ctx::pinned_dev).  Every kind of
// call has its regions in the union, apart from each other; behind the union, each in a place of its own, are what
// runs beside another call (two range pieces in flight, gzip's CRC words) and the small single read-backs.
constexpr size_t PINNED_BYTES = 1 << 20;
constexpr uint32_t INF_GROUP = 4096;             // buffers per T1 group
constexpr uint32_t SEG_GROUP_BUFS = 512;         // T2: buffers whose candidates are searched before the first read-back (round 3: 64 -> 512: 2048 x 64 KiB of zlib text 7.4 -> 3.8 ms with single-block streams taken by the block decoder)
constexpr uint32_t DEFLATE_DIRECT_BUFS = 16384;  // k_layout writes the results of a batch up to this size into the area
constexpr uint32_t DEFLATE_TABLE_BUFS = 14000;   // a larger batch's buffer table goes up from pageable memory
constexpr uint32_t MIRROR_ITEMS = 8192;          // work items whose results the host mirror holds (a call with a larger launch bound keeps the chain kernel)

constexpr size_t t1_cnt_bytes(size_t nbuf) { return 16 + nbuf * 4 + ((nbuf + 3) & ~(size_t)3); }  // T1: counters[4], cnt[nbuf], first bytes [nbuf]

struct RangeSlot {     // a piece of inflate_host_pipelined in flight: its search's counters and k_inf_chain_range's results
  uint32_t counters[6];
  ZesRes res[2];
};

struct PinnedArea {
  union {
    struct {
      ZesRes res[DEFLATE_DIRECT_BUFS];   // k_layout's results, straight from the kernel when the area is mapped
      ZesBuf table[DEFLATE_TABLE_BUFS];  // the buffer table of a batch
    } def;
    struct {                                           // inflate_t1_group, inflate_t1_range, the serial wavefront batch
      uint32_t counters[t1_cnt_bytes(INF_GROUP) / 4];  // (one buffer: k_inf_chain or the block decoder's mirror writes them)
      ZesRes res[INF_GROUP];                           // (one buffer: k_inf_chain writes them)
      ZesInfBuf table[INF_GROUP + 1];                  // the buffers and the sentinel
      ZesInfBuf redo[2];                               // one buffer's blocks decoded again into their own slots
      uint64_t ends[2 * INF_GROUP];                    // the serial wavefront batch: k_inf_decode's two words per stream ([0]: where it ended)
    } t1;
    struct {                   // inflate_jobs: one byte of every buffer of a group, read on the device
      uint8_t bytes[INF_GROUP];
      uint64_t offs[INF_GROUP];
    } first;
    struct {                               // inflate_segments and inflate_segments_run, one group
      ZesInfBuf search[SEG_GROUP_BUFS + 1];  // the candidate search's table
      uint32_t ncand[SEG_GROUP_BUFS];
      uint32_t nsurv;                        // the block-parallel tier's survivor count, going back up
      uint32_t flags[SEG_GROUP_BUFS + 1];    // [0, nb): not-in-store counts, later failure flags; [nb]: declined items
      uint32_t far;                          // matches behind the short marker ring
      ZesRes res[2 * SEG_GROUP_BUFS];        // k_inf_seg_chain: the chains, then where they ended
      ZesSegJob jobs[SEG_GROUP_BUFS];
      uint32_t live[SEG_GROUP_BUFS + 1];     // the items the wave decoder takes: count, items
      ZesSegOut out[SEG_GROUP_BUFS];
    } t2;
  };
  RangeSlot range[2];           // pieces k and k + 1 (slot k & 1)
  ZesRes res1;                  // read_res
  unsigned long long adler[2];  // adler32_locked
  uint32_t crc[2];              // the CRC-32 accumulator words (gzip_core: while the deflate results come back)
  uint8_t head[16], tail[8];    // header and trailer bytes on their way into a device result (gzip, deflate_join)
};

// k_inf_block_par's copy of a one-buffer T1 call's work items (ZesParMirror), as the host reads it
struct ParMirror {
  ZesCandRes cres[MIRROR_ITEMS];
  uint32_t start[MIRROR_ITEMS];  // the bit a candidate's block starts at, rank order
};

struct PinSpan {
  size_t off, len;
};
constexpr bool disjoint(std::initializer_list<PinSpan> s) {
  for (const PinSpan* a = s.begin(); a != s.end(); ++a)
    for (const PinSpan* b = a + 1; b != s.end(); ++b)
      if (a->off < b->off + b->len && b->off < a->off + a->len) return false;
  return true;
}
#define PIN_SPAN(m) PinSpan{offsetof(PinnedArea, m), sizeof(PinnedArea::m)}
#define PIN_HOLDS(m, n) static_assert(sizeof(PinnedArea::m) >= (n), #m " is smaller than its largest user")
static_assert(sizeof(PinnedArea) <= PINNED_BYTES, "the page-locked area does not fit its allocation");
PIN_HOLDS(def.res, sizeof(ZesRes) * DEFLATE_DIRECT_BUFS);
PIN_HOLDS(def.table, sizeof(ZesBuf) * DEFLATE_TABLE_BUFS);
PIN_HOLDS(t1.counters, t1_cnt_bytes(INF_GROUP));
PIN_HOLDS(t1.res, sizeof(ZesRes) * INF_GROUP);
PIN_HOLDS(t1.table, sizeof(ZesInfBuf) * (INF_GROUP + 1));
PIN_HOLDS(t1.redo, sizeof(ZesInfBuf) * 2);
PIN_HOLDS(t1.ends, sizeof(uint64_t) * 2 * INF_GROUP);
PIN_HOLDS(first.bytes, INF_GROUP);
PIN_HOLDS(first.offs, sizeof(uint64_t) * INF_GROUP);
PIN_HOLDS(t2.search, sizeof(ZesInfBuf) * (SEG_GROUP_BUFS + 1));
PIN_HOLDS(t2.ncand, sizeof(uint32_t) * SEG_GROUP_BUFS);
PIN_HOLDS(t2.flags, sizeof(uint32_t) * (SEG_GROUP_BUFS + 1));
PIN_HOLDS(t2.res, sizeof(ZesRes) * 2 * SEG_GROUP_BUFS);
PIN_HOLDS(t2.jobs, sizeof(ZesSegJob) * SEG_GROUP_BUFS);
PIN_HOLDS(t2.live, sizeof(uint32_t) * (SEG_GROUP_BUFS + 1));
PIN_HOLDS(t2.out, sizeof(ZesSegOut) * SEG_GROUP_BUFS);
PIN_HOLDS(range[0].counters, t1_cnt_bytes(1));
PIN_HOLDS(range[0].res, sizeof(ZesRes) * 2);
static_assert(sizeof(ParMirror::cres) >= sizeof(ZesCandRes) * MIRROR_ITEMS, "the mirror is smaller than its launch bound");
static_assert(sizeof(ParMirror::start) >= sizeof(uint32_t) * MIRROR_ITEMS, "the mirror is smaller than its launch bound");
// what one call uses at the same time
static_assert(disjoint({PIN_SPAN(range[0]), PIN_SPAN(range[1])}), "the two range slots overlap");
static_assert(disjoint({PIN_SPAN(def.res), PIN_SPAN(def.table), PIN_SPAN(crc)}), "deflate regions overlap (gzip_core: the CRC words beside the results)");
static_assert(disjoint({PIN_SPAN(t1.counters), PIN_SPAN(t1.res), PIN_SPAN(t1.table), PIN_SPAN(t1.redo), PIN_SPAN(t1.ends)}), "T1 regions overlap");
static_assert(disjoint({PIN_SPAN(first.bytes), PIN_SPAN(first.offs)}), "first-byte regions overlap");
static_assert(disjoint({PIN_SPAN(t2.search), PIN_SPAN(t2.ncand), PIN_SPAN(t2.nsurv), PIN_SPAN(t2.flags), PIN_SPAN(t2.far), PIN_SPAN(t2.res),
                        PIN_SPAN(t2.jobs), PIN_SPAN(t2.live), PIN_SPAN(t2.out)}),
              "T2 regions overlap");

// Every pooled device buffer of a context, once: Ctx has a member per name, for_each_pool walks them (what zes_trim
// gives back and zes_pool_bytes counts).
#define ZES_POOLS(X)                                                                                                              \
  /* deflate scratch */                                                                                                           \
  X(bufs) X(blks) X(idx_a) X(idx_b) X(sdelta) X(tmask) X(mlist) X(hists) X(codes) X(hdrs) X(adler) X(res) X(order)                \
  /* inflate scratch */                                                                                                           \
  X(surv) X(vlong) X(segfail) X(symoff) X(cand) X(cand_sorted) X(counters) X(cres) X(map) X(resume) X(dbg) X(ibufs) X(ibufs2)     \
  X(mvlist) X(scratch) X(sres) X(maps) X(seglist) X(segprefix) X(wins) X(sym16) X(segorder) X(segjobs) X(pw16) X(gwins)           \
  X(seglive) X(segouts)                                                                                                           \
  /* staging for the host-pointer API */                                                                                          \
  X(st_in) X(st_out)                                                                                                              \
  /* CRC-32: the kernel's table (x^(8 * 65536 * m) for m < crc_npow) and its two accumulator words; gzip reader: the input */     \
  /* (host forms), the result as it grows (host forms) and one member's output when it cannot go to its place directly; */        \
  /* member-parallel gzip reader: the bodies behind their 78 9C, the outputs that cannot go to their places directly, the */      \
  /* device tables (gz_walk_dev's members, gz_gather's segments); crcseg: seg_checksum_locked's segs | work | acc for */          \
  /* the CRC-32.  The BGZF writer uses the same: gz_in and gz_acc for a host call's input and result, gz_bodies for a */          \
  /* group's encoder slots, gz_tab for its member records */                                                                      \
  X(crctab) X(crcacc) X(gz_in) X(gz_acc) X(gz_stage) X(gz_bodies) X(gz_outs) X(gz_tab) X(crcseg)                                  \
  /* seg_checksum_locked's segs | work | acc for the Adler-32; the gathered trailers of a checked inflate batch */                \
  X(adlerseg)                                                                                                                     \
  /* zes_pngpix*: the unfiltered scanlines of a batch, a padded slot an image, on their way to k_png_expand; */                   \
  /* ZES_F_PNG_INTERLACED: the unfiltered passes of a batch's Adam7 images, a padded slot an image, on their way to */            \
  /* k_png_deinterlace */                                                                                                         \
  X(png_lines) X(png_passes)                                                                                                      \
  /* zes_gunzip_batch*: the output of a file on the per-file route that cannot be decoded in its place */                         \
  X(gz_batch)

// The survivor list of the block-start search as the block-parallel tier's scan left it in a pool (one buffer): the
// segment-parallel tier's search of the same stream starts from it instead of scanning again.  The note holds until it
// is dropped (the list is about to be rewritten, or another call begins: the bytes behind a pointer may have changed) or
// the pool's memory is given back (ensure, zes_trim, shutdown) - a new block may come back at the old address.
struct SurvList {
  bool ok = false;
  const uint8_t* d_in = nullptr;
  uint64_t in_off = 0, c = 0;
  uint32_t n = 0, gen = 0;
  void note(const DevBuf& list, const uint8_t* din, uint64_t off, uint64_t len, uint32_t nsurv) {
    ok = true, d_in = din, in_off = off, c = len, n = nsurv, gen = list.gen;
  }
  bool holds(const DevBuf& list, const uint8_t* din, uint64_t off, uint64_t len) const {  // this stream's list, whole, still in `list`
    return ok && gen == list.gen && list.p != nullptr && d_in == din && in_off == off && c == len;
  }
  void drop() { ok = false; }
};

struct Ctx {
  bool ready = false;
  int device = -1;
  int want = -1;  // zes_init_devices: the device this context binds to at its first use
  hipStream_t stream = nullptr;
  hipStream_t cs_in = nullptr, cs_out = nullptr;  // copy streams of the pipelined host calls (H2D / D2H beside the kernels)
  hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_k = nullptr;
  hipEvent_t ev_rng[2] = {nullptr, nullptr};  // host inflate in pieces: the results of piece k have come back
  hipStream_t s_adler = nullptr;                     // the Adler-32 pass of a deflate call runs beside the LZ77 kernels
  hipEvent_t ev_a0 = nullptr, ev_a1 = nullptr;
#define X(name) DevBuf name;
  ZES_POOLS(X)
#undef X
  uint32_t crc_npow = 0;
  DevBuf kraft;  // k_inf_scan's table: Kraft contribution of four 3-bit code-length fields at once (not a pool: it stays through zes_trim)
  PinnedArea* pinned = nullptr;
  PinnedArea* pinned_dev = nullptr;  // (null: not mapped; results are then copied back)
  ParMirror* mirror = nullptr;
  ParMirror* mirror_dev = nullptr;   // (null: not mapped; the chain kernel does the work then)
  ZesRes* res_more = nullptr;        // page-locked, grows: the results of a deflate batch larger than DEFLATE_DIRECT_BUFS
  size_t res_more_n = 0;
  // profiling
  bool profiling = false;
  std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> pending;
  std::vector<hipEvent_t> event_pool;
  std::vector<std::pair<std::string, KTime>> last_times;
  std::vector<std::pair<std::string, KTime>> carry;  // times collected in the middle of a call (a nested inflate_jobs) that its last collect_times puts in front of its own
  std::vector<std::string> name_pool;
  int last_tier = 0;
  bool device_chain = false;  // the block-parallel tier follows a single buffer's chain with k_inf_chain too, not on the host (pngpix_core)
  int last_members = 0;  // members the member-parallel gzip reader decoded in the last gunzip call (0: the serial path answered)
  uint32_t last_tiff_segs = 0;  // the last zes_tiff_read_* call: the segments its rectangle touched, the bytes it uploaded (zes_last_tiff_read)
  uint64_t last_tiff_up = 0;
  uint32_t last_gzb[2] = {0, 0};  // files of the last zes_gunzip_batch* call that finished as one batch / on the per-file route
  uint32_t route[ZES_ROUTE_WORDS] = {0};  // zes_stage_lz77_dev's last block: what its kernels did (zes_stage_lz77_route)
  SurvList sv;  // (of `surv`)
  char arch[64] = {0};
  int cus = 0;
  uint64_t hbm = 0;
};
template <class F>
void for_each_pool(Ctx& c, F fn) {
#define X(name) fn(c.name);
  ZES_POOLS(X)
#undef X
}

// One context per device the library drives (zes_init(ngpus); "the batch API is where multi-GPU
// concurrency lives").  zes_init(device) binds context 0 — one process per GPU, what bench.py's ranks do;
// zes_init_devices(n) binds contexts 0 .. n-1 to devices 0 .. n-1, and the host-pointer entry points spread their
// work over them: a batch is partitioned by size (zes_partition, the rule of shard.partition) and every share runs
// on its own host thread against its own context — stream, scratch pools, staging ring, lock — while single calls
// go round robin.  Results of the host forms land in the caller's memory, so no device-to-device gather is needed
// here; HBM-resident results are gathered by shard.py over RCCL.  Which context a thread works on is thread-local.
constexpr int ZES_MAX_DEV = 16;
Ctx g_ctx[ZES_MAX_DEV];
std::mutex g_mus[ZES_MAX_DEV];
std::atomic<int> g_nctx{1};     // contexts in use (written under g_cfg_mu; read by every routed call)
std::mutex g_cfg_mu;             // guards g_nctx and the context -> device binding
thread_local int t_dev = 0;      // the context of the call this thread is inside
thread_local bool t_routed = false;
thread_local int t_last = 0;     // the context that served this thread's last call (what zes_last_inflate_tier / zes_last_kernel_times report on)
#define g (g_ctx[t_dev])
#define g_mu (g_mus[t_dev])
struct UseDev {                  // a call's context for its duration (nested entry points keep the outer one's)
  int prev;
  bool prev_routed;
  explicit UseDev(int d) : prev(t_dev), prev_routed(t_routed) {
    if (!t_routed) t_dev = d;
    t_routed = true;
    t_last = t_dev;
  }
  ~UseDev() {
    t_dev = prev;
    t_routed = prev_routed;
  }
};

#define HIPCHK(x)                                                                              \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) {                                                                    \
      if (getenv("ZES_DEBUG")) fprintf(stderr, "zes: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
      return ZES_E_DEVICE;                                                                     \
    }                                                                                          \
  } while (0)

// gives a buffer's memory back: every place that frees one goes through here, so that a note about what the buffer held
// (SurvList) can tell
hipError_t release(DevBuf& b) {
  const hipError_t e = b.p ? hipFree(b.p) : hipSuccess;
  b.p = nullptr;
  b.cap = 0;
  b.gen++;
  return e;
}

int ensure(DevBuf& b, size_t bytes) {
  if (bytes <= b.cap) return ZES_OK;
  HIPCHK(release(b));
  size_t want = bytes + bytes / 8 + 4096;
  HIPCHK(hipMalloc(&b.p, want));
  b.cap = want;
  return ZES_OK;
}

// up to the next 16-byte boundary: the places of a pooled buffer start at one
uint64_t gz_up16(uint64_t v) { return (v + 15) & ~15ull; }

// Host memory that a copy queued on the stream reads or writes outlives the stream's work on every way out: a function
// that copies from or to memory of its own declares that memory first and a Drain BEHIND it (locals go in reverse order of
// declaration: the guard's wait comes first, then the memory), and calls done() behind its own last synchronisation.  On any
// other way out (HIPCHK, a helper's status) the guard lets the stream finish before the memory goes, and clears a HIP error
// from that wait (the call's status is the one on its way already).
struct Drain {
  bool armed = true;
  void done() { armed = false; }
  ~Drain() {
    if (armed && hipStreamSynchronize(g.stream) != hipSuccess) (void)hipGetLastError();
  }
};

int init_locked(int device) {
  if (g.ready) {
    if (device >= 0 && device != g.device) return ZES_E_ARG;
    // HIP's current device is per thread: a call from a thread that never made one current (a libuv worker, a Python
    // thread) would allocate on device 0 while the stream belongs to g.device
    HIPCHK(hipSetDevice(g.device));
    return ZES_OK;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ZES_E_DEVICE;
  if (device < 0) device = g.want >= 0 ? g.want : 0;
  if (device >= n) return ZES_E_DEVICE;
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  snprintf(g.arch, sizeof g.arch, "%s", prop.gcnArchName);
  g.cus = prop.multiProcessorCount;
  g.hbm = prop.totalGlobalMem;
  HIPCHK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&g.cs_in, hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&g.cs_out, hipStreamNonBlocking));
  for (int k = 0; k < 2; k++) HIPCHK(hipEventCreateWithFlags(&g.ev_up[k], hipEventDisableTiming));
  for (int k = 0; k < 2; k++) HIPCHK(hipEventCreateWithFlags(&g.ev_rng[k], hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&g.ev_k, hipEventDisableTiming));
  HIPCHK(hipStreamCreateWithFlags(&g.s_adler, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&g.ev_a0, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&g.ev_a1, hipEventDisableTiming));
  auto dev_addr = [](void* h) -> void* {
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess) return d;
    (void)hipGetLastError();
    return nullptr;
  };
  HIPCHK(hipHostMalloc((void**)&g.pinned, PINNED_BYTES, hipHostMallocDefault));
  g.pinned_dev = (PinnedArea*)dev_addr(g.pinned);
  if (hipHostMalloc((void**)&g.mirror, sizeof(ParMirror), hipHostMallocDefault) == hipSuccess) {
    g.mirror_dev = (ParMirror*)dev_addr(g.mirror);
  } else {
    (void)hipGetLastError();
    g.mirror = nullptr;
  }
  {
    // units of 2^-7, a field of 0 adds nothing; saturated at 200 so that an over-full group can never sum back to exactly 128
    uint8_t tab[4096];
    for (uint32_t i = 0; i < 4096; i++) {
      uint32_t k = 0;
      for (uint32_t f = 0; f < 4; f++) k += (128u >> ((i >> (3 * f)) & 7u)) & 127u;
      tab[i] = (uint8_t)std::min(k, 200u);
    }
    HIPCHK(hipMalloc(&g.kraft.p, 4096));
    g.kraft.cap = 4096;
    HIPCHK(hipMemcpy(g.kraft.p, tab, 4096, hipMemcpyHostToDevice));
  }
  g.device = device;
  g.ready = true;
  return ZES_OK;
}

// ---- which context serves a call ----
int route_host() {  // host-pointer work: the contexts in turn
  if (t_routed) return t_dev;
  const int n = g_nctx.load();
  if (n <= 1) return 0;
  static std::atomic<uint32_t> rr{0};
  return (int)(rr.fetch_add(1) % (uint32_t)n);
}
// -1: several contexts are bound and none of them drives the device that holds the memory (or the pointer is not device
// memory at all, or the two pointers of a call sit on different devices) — the entry point answers ZES_E_ARG instead of
// letting context 0's kernels touch memory of a device it does not drive
int route_dev(const void* p, const void* p2 = nullptr) {  // device-pointer work: the context of the device that holds the memory
  if (t_routed) return t_dev;
  if (g_nctx.load() <= 1 || !p) return 0;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  if (p2) {
    hipPointerAttribute_t b;
    if (hipPointerGetAttributes(&b, p2) != hipSuccess) {
      (void)hipGetLastError();
      return -1;
    }
    if (b.device != a.device) return -1;
  }
  for (int i = 0, n = g_nctx.load(); i < n; i++)
    if ((g_ctx[i].ready ? g_ctx[i].device : g_ctx[i].want) == a.device) return i;
  return -1;
}
#define ROUTE_DEV(...)                    \
  const int rd_ = route_dev(__VA_ARGS__); \
  if (rd_ < 0) return ZES_E_ARG;          \
  UseDev ud(rd_)
// An entry point's prologue, behind its argument checks and its routing: this context's lock, held by the calling frame
// until it returns (`lk`), and the context brought up under it (`rc`: its first use binds it to its device)
#define LOCK_READY()                    \
  std::lock_guard<std::mutex> lk(g_mu); \
  int rc = init_locked(-1);             \
  if (rc) return rc

// ---- host <-> device staging of the host-pointer entry points ----
// A caller's buffer (a JS Uint8Array, a numpy array) is pageable: the DMA engines cannot read it.  It crosses in
// chunks through a ring of pinned buffers: helper threads copy chunk k+1 into its pinned buffer while the DMA of
// chunk k runs (and the other way round on the way back), so the trip costs max(memcpy, DMA) instead of their sum
// and the memcpy is spread over several cores.  A buffer that already is pinned (zes_host_alloc) is handed to the
// DMA engine as it is.
constexpr size_t STAGE_CHUNK = 8u << 20;
constexpr int STAGE_RING = 4;
constexpr size_t STAGE_DIRECT_MAX = 256u << 10;  // below this one plain copy call is quicker than the ring

struct CopyPool {
  std::vector<std::thread> threads;
  std::mutex mu;
  std::condition_variable cv_work, cv_done;
  uint8_t* dst = nullptr;
  const uint8_t* src = nullptr;
  size_t n = 0, part = 0;
  uint32_t gen = 0, parts = 0;
  std::atomic<uint32_t> next{0};
  uint32_t done = 0, active = 0;
  bool stop = false;

  void worker() {
    uint32_t seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv_work.wait(lk, [&] { return stop || gen != seen; });
      if (stop) return;
      seen = gen;
      active++;  // checked in under the lock: copy() does not return (and the next job is not written) before every
      lk.unlock();  // worker that picked this generation up has checked out again — no claim of an old job can
      const uint32_t did = run_parts();  // meet the fields of a new one
      lk.lock();
      done += did;
      active--;
      if (done >= parts && active == 0) cv_done.notify_all();
    }
  }
  uint32_t run_parts() {
    uint32_t did = 0;
    for (;;) {
      const uint32_t k = next.fetch_add(1);
      if (k >= parts) return did;
      const size_t o = (size_t)k * part;
      memcpy(dst + o, src + o, std::min(part, n - o));
      did++;
    }
  }
  void start() {
    if (!threads.empty()) return;
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned nt = std::max(1u, std::min(7u, hw ? hw / 2 : 2u));  // (two pools + two side threads: 16, a one-GPU box's share)
    for (unsigned i = 0; i + 1 < nt; i++) threads.emplace_back([this] { worker(); });
  }
  // memcpy spread over the pool (the caller takes parts too); plain memcpy when it is short
  void copy(uint8_t* d, const uint8_t* s_, size_t bytes) {
    if (bytes < (512u << 10) || threads.empty()) {
      memcpy(d, s_, bytes);
      return;
    }
    {
      std::lock_guard<std::mutex> lk(mu);
      dst = d;
      src = s_;
      n = bytes;
      part = 256u << 10;
      parts = (uint32_t)((bytes + part - 1) / part);
      next.store(0);
      done = 0;
      gen++;
    }
    cv_work.notify_all();
    const uint32_t did = run_parts();
    std::unique_lock<std::mutex> lk(mu);
    done += did;
    cv_done.wait(lk, [&] { return done >= parts && active == 0; });
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv_work.notify_all();
    for (auto& t : threads) t.join();
    threads.clear();
    stop = false;
  }
  // a process that never calls zes_shutdown still has to get rid of the helpers: destroying a joinable std::thread
  // at exit calls std::terminate (seen as a host process that never exits)
  ~CopyPool() { shutdown(); }
};

// One direction's staging: a ring of pinned chunks, their events, the copy helpers.  Two of them, so that an upload
// and a download of a pipelined call run side by side (each on its own copy stream and its own thread).
struct Stager {
  CopyPool pool;
  uint8_t* buf[STAGE_RING] = {nullptr};
  hipEvent_t ev[STAGE_RING] = {nullptr};
  int ready() {
    if (buf[0]) return ZES_OK;
    for (int k = 0; k < STAGE_RING; k++) {
      HIPCHK(hipHostMalloc((void**)&buf[k], STAGE_CHUNK, hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
    }
    pool.start();
    return ZES_OK;
  }
  void release() {
    pool.shutdown();
    for (int k = 0; k < STAGE_RING; k++) {
      if (buf[k]) (void)hipHostFree(buf[k]);
      if (ev[k]) (void)hipEventDestroy(ev[k]);
      buf[k] = nullptr;
      ev[k] = nullptr;
    }
  }
};
Stager g_ups[ZES_MAX_DEV], g_downs[ZES_MAX_DEV];
#define g_up (g_ups[t_dev])
#define g_down (g_downs[t_dev])

// A thread that runs the side legs of a pipelined host call (one for uploads, one for downloads): submit() hands it
// a task, the returned future gives the task's status.
struct SideThread {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::packaged_task<int()>> q;
  bool stop = false;
  int owner = 0;
  void loop() {
    t_dev = owner;                                     // the context this thread serves
    if (g.device >= 0) (void)hipSetDevice(g.device);  // HIP's current device is per thread
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return stop || !q.empty(); });
      if (q.empty()) return;
      std::packaged_task<int()> t = std::move(q.front());
      q.erase(q.begin());
      lk.unlock();
      t();
      lk.lock();
    }
  }
  std::future<int> submit(std::function<int()> fn) {
    std::packaged_task<int()> t(std::move(fn));
    std::future<int> f = t.get_future();
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!th.joinable()) {
        owner = t_dev;
        th = std::thread([this] { loop(); });
      }
      q.push_back(std::move(t));
    }
    cv.notify_one();
    return f;
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
    stop = false;
  }
  ~SideThread() { shutdown(); }
};
SideThread g_side_ups[ZES_MAX_DEV], g_side_downs[ZES_MAX_DEV];
#define g_side_up (g_side_ups[t_dev])
#define g_side_down (g_side_downs[t_dev])

bool is_pinned(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // an ordinary malloc'd pointer: not an error of ours
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// A caller's large pageable buffer goes through the runtime's own copy call: on the MI355X host hipMemcpy reads and
// writes pageable memory at the rate of pinned memory (1.2 ms per 64 MiB either way, tools/gpu_hostregister_probe.py:
// it page-locks the range for the copy itself), where the staging ring below costs a memcpy of every byte (~1 ms per
// 32 MiB with seven helper threads).  The copy is complete when upload()/download() return; in the pipelined calls
// they run on the side threads.  (Page-locking the caller's buffer in place with hipHostRegister for the whole call
// was as fast — 0.25 ms per 64 MiB to register — and was taken out when a GPU memory fault turned up in a long fuzz
// run with it.  That fault was traced later (ZES_TRACE_KERNELS tail of tools/gpu_fuzz.py seed 77) to k_inf_verify
// reading stale surv[] entries the scan had reserved but not written — fixed in the scan, DESIGN §6 — so registration
// was not its cause.  It stays off because it buys nothing over the runtime's path on this host and would pin a
// caller's pages for the length of the call.)
// The ring remains for buffers of 256 KiB to 4 MiB: the per-call cost of the runtime's path shows there.
constexpr uint64_t RUNTIME_COPY_MIN = 4ull << 20;

// host -> device on `stream` (the library's stream by default).  A pageable source has been read when this returns;
// a PINNED source (or one of <= STAGE_DIRECT_MAX bytes, which the runtime stages itself) is only enqueued: the DMA
// reads it asynchronously, and every caller synchronises `stream` before it returns to its own caller (they all do:
// each entry point ends with the read-back of its result on g.stream, the pipelined ones join their side threads).
int upload(uint8_t* d_dst, const uint8_t* src, uint64_t n, hipStream_t stream = nullptr) {
  if (!stream) stream = g.stream;
  if (!n) return ZES_OK;
  if (n <= STAGE_DIRECT_MAX || is_pinned(src)) {
    HIPCHK(hipMemcpyAsync(d_dst, src, n, hipMemcpyHostToDevice, stream));
    return ZES_OK;
  }
  if (n >= RUNTIME_COPY_MIN && !getenv("ZES_STAGE_RING")) {
    HIPCHK(hipMemcpyAsync(d_dst, src, n, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));  // the caller's memory has been read
    return ZES_OK;
  }
  Stager& S = g_up;
  int rc = S.ready();
  if (rc) return rc;
  uint64_t off = 0;
  for (uint32_t k = 0; off < n; k++, off += STAGE_CHUNK) {
    const int slot = (int)(k % STAGE_RING);
    const size_t len = (size_t)std::min<uint64_t>(STAGE_CHUNK, n - off);
    if (k >= STAGE_RING) HIPCHK(hipEventSynchronize(S.ev[slot]));  // its previous DMA has read the pinned buffer
    S.pool.copy(S.buf[slot], src + off, len);
    HIPCHK(hipMemcpyAsync(d_dst + off, S.buf[slot], len, hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(S.ev[slot], stream));
  }
  // the pinned ring is reused by the next call: its DMAs must have left it (the caller's memory was read above)
  for (int k = 0; k < STAGE_RING; k++) HIPCHK(hipEventSynchronize(S.ev[k]));
  return ZES_OK;
}

// device -> host, complete on return
// (`wait`: with a pinned destination, return with the copy in flight on `stream`; the caller synchronises)
int download(uint8_t* dst, const uint8_t* d_src, uint64_t n, hipStream_t stream = nullptr, bool wait = true) {
  if (!stream) stream = g.stream;
  const bool direct = n <= STAGE_DIRECT_MAX || is_pinned(dst);
  if (n && direct) HIPCHK(hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, stream));
  if (direct) {
    if (wait) HIPCHK(hipStreamSynchronize(stream));
    return ZES_OK;
  }
  if (n >= RUNTIME_COPY_MIN && !getenv("ZES_STAGE_RING")) {
    HIPCHK(hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return ZES_OK;
  }
  Stager& S = g_down;
  int rc = S.ready();
  if (rc) return rc;
  const uint32_t chunks = (uint32_t)((n + STAGE_CHUNK - 1) / STAGE_CHUNK);
  auto issue = [&](uint32_t k) -> int {
    const uint64_t off = (uint64_t)k * STAGE_CHUNK;
    const size_t len = (size_t)std::min<uint64_t>(STAGE_CHUNK, n - off);
    HIPCHK(hipMemcpyAsync(S.buf[k % STAGE_RING], d_src + off, len, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(S.ev[k % STAGE_RING], stream));
    return ZES_OK;
  };
  for (uint32_t k = 0; k < chunks && k < (uint32_t)STAGE_RING - 1; k++)
    if ((rc = issue(k))) return rc;
  for (uint32_t k = 0; k < chunks; k++) {
    if (k + STAGE_RING - 1 < chunks && (rc = issue(k + STAGE_RING - 1))) return rc;  // its slot was emptied in the round before
    HIPCHK(hipEventSynchronize(S.ev[k % STAGE_RING]));
    const uint64_t off = (uint64_t)k * STAGE_CHUNK;
    S.pool.copy(dst + off, S.buf[k % STAGE_RING], (size_t)std::min<uint64_t>(STAGE_CHUNK, n - off));
  }
  return ZES_OK;
}

// a host form's input into a pooled buffer, `at` bytes into it (2: behind the zlib header the raw forms supply)
int stage_in(DevBuf& b, const uint8_t* in, uint64_t n, size_t at = 0) {
  const int rc = ensure(b, at + n + 64);
  return rc ? rc : upload((uint8_t*)b.p + at, in, n);
}

// Decode into a pooled buffer whose size is a guess, like the reference's Uint8WriteStream: run(dst, cap, &n) decodes
// into cap bytes at dst; while it answers ZES_E_NOSPACE with a size beyond cap, the pool grows to that size (exact, as a
// rule: the second attempt fits).  First guess: 4c — a reference-made stream of c bytes rarely inflates beyond that — or
// `at_least`.  Returns run's last status; *n is the result's size then.
template <class Run>
int grow_and_retry(DevBuf& pool, uint64_t c, uint64_t at_least, uint64_t* n, Run run) {
  uint64_t cap = std::max<uint64_t>(at_least, std::max<uint64_t>(c * 4, 1 << 20));
  for (int attempt = 0; attempt < 8; attempt++) {
    int rc = ensure(pool, cap + 64);
    if (rc) return rc;
    rc = run((uint8_t*)pool.p, cap, n);
    if (rc != ZES_E_NOSPACE || *n <= cap) return rc;
    cap = *n;
  }
  return ZES_E_DEVICE;
}

// ---- kernel timing (HIP events on the library's stream) ----
// events are pooled: creating and destroying a pair per launch costs more than recording them
hipEvent_t take_event() {
  if (!g.event_pool.empty()) {
    hipEvent_t e = g.event_pool.back();
    g.event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

struct Timed {
  hipEvent_t a = nullptr, b = nullptr;
  const char* name;
  hipStream_t st;
  explicit Timed(const char* n, hipStream_t stream = nullptr) : name(n), st(stream ? stream : g.stream) {
    if (g.profiling) {
      a = take_event();
      b = take_event();
      (void)hipEventRecord(a, st);
    }
  }
  ~Timed() {
    if (g.profiling) {
      (void)hipEventRecord(b, st);
      g.pending.push_back({name, {a, b}});
    }
    // ZES_TRACE_KERNELS: wait for the launch and name it on stderr (the kernel after the last name printed is the one
    // a GPU fault belongs to)
    static const bool trace = getenv("ZES_TRACE_KERNELS") != nullptr;
    if (trace) {
      const hipError_t e = hipStreamSynchronize(g.stream);
      fprintf(stderr, "zes kernel done: %s (%s)\n", name, hipGetErrorName(e));
      fflush(stderr);
    }
  }
};

void collect_times() {
  if (!g.profiling) return;
  std::map<std::string, KTime> acc;
  std::vector<std::string> order;
  for (auto& p : g.pending) {
    float ms = 0;
    (void)hipEventSynchronize(p.second.second);
    (void)hipEventElapsedTime(&ms, p.second.first, p.second.second);
    if (!acc.count(p.first)) order.push_back(p.first);
    acc[p.first].ms += ms;
    acc[p.first].launches++;
    g.event_pool.push_back(p.second.first);
    g.event_pool.push_back(p.second.second);
  }
  g.pending.clear();
  g.last_times.clear();
  for (auto& e : g.carry) {
    auto it = acc.find(e.first);
    if (it != acc.end()) {
      e.second.ms += it->second.ms;
      e.second.launches += it->second.launches;
      acc.erase(it);
    }
    g.last_times.push_back(e);
  }
  g.carry.clear();
  for (auto& n : order)
    if (acc.count(n)) g.last_times.push_back({n, acc[n]});
}

// The call's report keeps what a driver in front (inflate_jobs, deflate_batch_core) has collected already: the call's last
// collect_times puts it in front of the launches that follow
void keep_times() {
  if (g.profiling) g.carry = g.last_times;
}

// ---- deflate ----
bool deflate_throws(uint64_t n) { return n == 0 || n == 1 || (n % ZES_BLK) == 1; }
uint64_t deflate_bound(uint64_t n) { return ((n < ZES_BLK / 2) ? (uint64_t)ZES_BLK : n * 2) + 6; }

// ZES_DEBUG_PHASES: a deflate kernel's cycle stamps, eight words per block in g.dbg.  phases_arm in front of the
// launches (`set`: the kernel file's zes_*_set_dbg), phases_print behind them: the stamps of the blocks that ran (stamp
// `ran` is set), averaged — stamps 1 .. ran as differences to the stamp before, those behind `ran` as they are — and
// printed by `fmt` (the block count, then the averages in stamp order).
using PhaseSetter = void (*)(unsigned long long*);
int phases_arm(PhaseSetter set, uint32_t nblk) {
  int rc = ensure(g.dbg, (size_t)nblk * 64);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(g.dbg.p, 0, (size_t)nblk * 64, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  set((unsigned long long*)g.dbg.p);
  return ZES_OK;
}
int phases_print(PhaseSetter set, uint32_t nblk, int ran, const char* fmt) {
  HIPCHK(hipStreamSynchronize(g.stream));
  set(nullptr);
  std::vector<unsigned long long> h((size_t)nblk * 8);
  HIPCHK(hipMemcpy(h.data(), g.dbg.p, h.size() * 8, hipMemcpyDeviceToHost));
  double acc[8] = {0};
  uint32_t n = 0;
  for (uint32_t i = 0; i < nblk; i++) {
    const unsigned long long* s = &h[(size_t)i * 8];
    if (!s[ran]) continue;
    n++;
    for (int k = 1; k < 8; k++) acc[k] += (double)(k <= ran ? s[k] - s[k - 1] : s[k]);
  }
  if (n) fprintf(stderr, fmt, n, acc[1] / n, acc[2] / n, acc[3] / n, acc[4] / n, acc[5] / n, acc[6] / n, acc[7] / n);
  return ZES_OK;
}

// The LZ77 launches of the deflate pipeline over the `grid` blocks of g.bufs / g.blks (input at d_in): index (k_lz_sort,
// with use_index k_lz_index for dense blocks and the sort again for what it could not take), matches, tokens into
// g.idx_a and histograms into g.hists.  The whole pipeline and zes_stage_lz77_dev, which the parity tests take as its
// stand-in, both launch through here.  after_index() runs between the index and the match launches.
// heaviest_first: a batch of unlike buffers, the lazy matcher takes the blocks in k_lz_order's order.
// phases: ZES_DEBUG_PHASES stamps of the lazy matcher (printed here) and the parser (armed here: the caller prints them).
// route: null in the pipeline.  The stage entry's one block: behind each index launch its flag word is copied to
// route[0..2], and the word the launch left in idx_b's last slot to route[3] (first sort) and route[4] (k_lz_index).
template <class F>
int launch_lz77(const uint8_t* d_in, uint32_t grid, bool use_index, bool heaviest_first, bool phases, F after_index, uint32_t* route = nullptr) {
  // in the pipeline a block parsed from its match list goes on in the position form (zes_kernels.h: ZES_POS_WORDS); the
  // stage entry hands tokens to the host and asks for the list
  const uint32_t list_form = route ? 1u : 0u;
  int rc;
  const ZesBuf* dbufs = (const ZesBuf*)g.bufs.p;
  ZesBlk* dblks = (ZesBlk*)g.blks.p;
  uint32_t* idx_a = (uint32_t*)g.idx_a.p;
  uint32_t* idx_b = (uint32_t*)g.idx_b.p;
  // dense blocks (text, periodic data) get their index from k_lz_index (LDS-resident class sorts); a block it cannot take
  // goes back to k_lz_sort in a second launch that every other block leaves at once
  {
    Timed t("k_lz_sort");
    hipLaunchKernelGGL(k_lz_sort, dim3(grid), dim3(SORT_THREADS), 0, g.stream, d_in, dbufs, dblks, idx_a, idx_b, idx_a, (uint16_t*)g.sdelta.p,
                       ZES_SORT_MODE_FIRST | (use_index ? ZES_SORT_USE_INDEX : 0u));
  }
  auto note = [&](uint32_t* flag_to, uint32_t* word_to) -> int {  // (copies on the stream, behind the launch they report on)
    HIPCHK(hipMemcpyAsync(flag_to, idx_a + ZES_BLK - 1, 4, hipMemcpyDeviceToHost, g.stream));
    if (word_to) HIPCHK(hipMemcpyAsync(word_to, idx_b + ZES_BLK - 1, 4, hipMemcpyDeviceToHost, g.stream));
    return ZES_OK;
  };
  if (route && (rc = note(&route[0], &route[3]))) return rc;
  if (use_index) {
    {
      Timed t("k_lz_index");
      hipLaunchKernelGGL(k_lz_index, dim3(grid), dim3(IDX_THREADS), 0, g.stream, d_in, dbufs, dblks, idx_a, idx_b, idx_a, (uint16_t*)g.sdelta.p);
    }
    if (route && (rc = note(&route[1], &route[4]))) return rc;
    {
      Timed t("k_lz_sort_redo");
      hipLaunchKernelGGL(k_lz_sort, dim3(grid), dim3(SORT_THREADS), 0, g.stream, d_in, dbufs, dblks, idx_a, idx_b, idx_a, (uint16_t*)g.sdelta.p,
                         ZES_SORT_MODE_REDO);
    }
    if (route && (rc = note(&route[2], nullptr))) return rc;
  }
  if ((rc = after_index())) return rc;
  {
    Timed t("k_lz_match");  // match words go to idx_b (free after the sort)
    hipLaunchKernelGGL(k_lz_match, dim3(grid), dim3(MATCH_THREADS), 0, g.stream, d_in, dbufs, dblks, idx_a, idx_b, (uint32_t*)g.mlist.p);
  }
  if (phases && (rc = phases_arm(zes_lazy_set_dbg, grid))) return rc;
  {
    // the blocks heaviest first (k_lz_order), so that the launch does not end on a tail of text blocks
    const uint32_t* order = nullptr;
    if (heaviest_first) {
      if ((rc = ensure(g.order, (size_t)grid * 4))) return rc;
      Timed t("k_lz_order");
      hipLaunchKernelGGL(k_lz_order, dim3(1), dim3(1024), 0, g.stream, (const uint32_t*)idx_a, grid, (uint32_t*)g.order.p);
      order = (const uint32_t*)g.order.p;
    }
    Timed t("k_lz_match_lazy");  // the blocks k_lz_sort flagged (most positions kept); the others return at once
    hipLaunchKernelGGL(k_lz_match_lazy, dim3(grid), dim3(MATCH_THREADS), 0, g.stream, d_in, dbufs, dblks, idx_a, (const uint32_t*)idx_a,
                       (const uint16_t*)g.sdelta.p, idx_b, (uint32_t*)g.tmask.p, (uint32_t*)g.mlist.p, order);
  }
  if (phases) {  // (this kernel's stamps 6 and 7 are not clocks: averaged as they are, and the text has no place for the last)
    if ((rc = phases_print(zes_lazy_set_dbg, grid, 5,
                           "zes lazy match steps (avg cycles over %u blocks): stage %.0f tail %.0f window chains %.0f entry chains %.0f true chain (only unmerged blocks) %.0f | first wave, window chains: %.0f loop turns\n")))
      return rc;
    if ((rc = phases_arm(zes_parse_set_dbg, grid))) return rc;  // (printed by deflate_batch_core, behind this function)
  }
  {
    Timed t("k_lz_parse_small");  // tokens go to idx_a (free after the match pass)
    // two launches over all blocks: the blocks with a chain mask or a short match list run two to a compute unit
    // (k_lz_parse_small), the others need the exit maps' 128 KiB; each kernel leaves the other's blocks at once
    hipLaunchKernelGGL(k_lz_parse_small, dim3(grid), dim3(PARSE_THREADS), 0, g.stream, d_in, dbufs, dblks, idx_b, idx_a, (uint32_t*)g.hists.p,
                       (const uint32_t*)g.tmask.p, (const uint32_t*)g.mlist.p, list_form);
  }
  {
    Timed t("k_lz_parse");
    hipLaunchKernelGGL(k_lz_parse, dim3(grid), dim3(PARSE_THREADS), 0, g.stream, d_in, dbufs, dblks, idx_b, idx_a, (uint32_t*)g.hists.p,
                       (const uint32_t*)g.tmask.p, (const uint32_t*)g.mlist.p);
  }
  return ZES_OK;
}

// What only a one-buffer call has to say (deflate_one): the range form of the buffer, and its Adler-32 on the way back
struct DeflateRange {
  uint64_t n_read = 0;     // bytes readable from the buffer's start on (the match finder's halo behind it); less than its length: its length
  uint32_t flags = 0;      // ZES_BUF_*
  uint32_t start_bit = 0;  // the first bit of the result lies this far into d_out + out_off
  bool defer = false;      // return behind the launches: the caller synchronises g.stream itself and reads g.pinned->def.res[0]
  uint32_t adler = 1;      // out (not when deferred): Adler-32 of the buffer
};

// Core: count buffers inside d_in / d_out.  Buffers whose status[] comes back non-zero were
// rejected on the host (throw cases, capacity) and are skipped by the device pass.  `one`: with count == 1 only.
int deflate_batch_core(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* d_out,
                       const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status,
                       uint32_t count, DeflateRange* one = nullptr) {
  std::vector<ZesBuf> hb;
  uint64_t nblk_total = 0;
  std::vector<uint32_t> live;
  hb.reserve(count);
  for (uint32_t i = 0; i < count; i++) {
    out_len[i] = 0;
    if (deflate_throws(in_len[i])) {
      status[i] = ZES_E_CORRUPT;
      continue;
    }
    if (out_cap[i] < deflate_bound(in_len[i])) {
      status[i] = ZES_E_NOSPACE;
      out_len[i] = deflate_bound(in_len[i]);
      continue;
    }
    if ((out_off[i] & 15u) || (((uintptr_t)d_out) & 15u)) {
      status[i] = ZES_E_ARG;
      continue;
    }
    status[i] = ZES_OK;
    ZesBuf b;
    b.in_off = in_off[i];
    b.n = in_len[i];
    b.out_off = out_off[i];
    b.cap = out_cap[i];
    b.first_blk = (uint32_t)nblk_total;
    b.nblk = (uint32_t)((in_len[i] + ZES_BLK - 1) / ZES_BLK);
    b.n_read = one ? std::max(one->n_read, in_len[i]) : in_len[i];
    b.flags = one ? one->flags : 0u;
    b.start_bit = one ? one->start_bit : 0u;
    nblk_total += b.nblk;
    hb.push_back(b);
    live.push_back(i);
  }
  if (hb.empty()) return ZES_OK;
  if (nblk_total >= (1ull << 31)) return ZES_E_ARG;
  const uint32_t nbuf = (uint32_t)hb.size(), nblk = (uint32_t)nblk_total;
  int rc;
  if ((rc = ensure(g.bufs, sizeof(ZesBuf) * nbuf))) return rc;
  if ((rc = ensure(g.blks, sizeof(ZesBlk) * nblk))) return rc;
  if ((rc = ensure(g.idx_a, (size_t)nblk * ZES_BLK * 4))) return rc;
  if ((rc = ensure(g.idx_b, (size_t)nblk * ZES_BLK * 4))) return rc;
  if ((rc = ensure(g.sdelta, (size_t)nblk * ZES_BLK * 2 + 64))) return rc;
  if ((rc = ensure(g.tmask, (size_t)nblk * ZES_TMASK_WORDS * 4))) return rc;  // k_lz_match_lazy -> k_lz_parse: the chain's positions
  if ((rc = ensure(g.mlist, (size_t)nblk * ZES_MLIST_WORDS * 4))) return rc;  // k_lz_match -> k_lz_parse: the matches of a match-poor block
  if ((rc = ensure(g.hists, (size_t)nblk * 320 * 4))) return rc;
  if ((rc = ensure(g.codes, (size_t)nblk * 320 * 4))) return rc;
  if ((rc = ensure(g.hdrs, (size_t)nblk * ZES_HDR_WORDS * 4))) return rc;
  if ((rc = ensure(g.adler, (size_t)nbuf * 16))) return rc;
  if ((rc = ensure(g.res, sizeof(ZesRes) * nbuf))) return rc;
  // the buffer table goes up through pinned memory (a one-buffer call passes its entry as a kernel
  // argument instead); the block records and the cleared Adler accumulators are made on the device
  ZesBuf* dbufs = (ZesBuf*)g.bufs.p;
  ZesBlk* dblks = (ZesBlk*)g.blks.p;
  unsigned long long* adler = (unsigned long long*)g.adler.p;
  if (nbuf > 1) {
    if (nbuf <= DEFLATE_TABLE_BUFS) {
      memcpy(g.pinned->def.table, hb.data(), sizeof(ZesBuf) * nbuf);
      HIPCHK(hipMemcpyAsync(g.bufs.p, g.pinned->def.table, sizeof(ZesBuf) * nbuf, hipMemcpyHostToDevice, g.stream));
    } else {
      HIPCHK(hipMemcpy(g.bufs.p, hb.data(), sizeof(ZesBuf) * nbuf, hipMemcpyHostToDevice));
    }
  }
  {
    Timed t("k_make_blks");
    const uint32_t nthr = std::max(nblk, 2u * nbuf);
    hipLaunchKernelGGL(k_make_blks, dim3((nthr + 255) / 256), dim3(256), 0, g.stream, hb[0], nbuf, dbufs, dblks, nblk, adler);
  }
  // Adler-32 (src/adler32.ts:1-10) needs the input and the cleared accumulators, and nobody but k_layout needs its
  // result: it runs on a stream of its own beside the LZ77 kernels — an HBM-bound pass of 64-byte-LDS workgroups next to
  // kernels that hold a block in LDS and wait on it (0.04 ms per 64 MiB off the critical path).
  {
    HIPCHK(hipEventRecord(g.ev_a0, g.stream));
    HIPCHK(hipStreamWaitEvent(g.s_adler, g.ev_a0, 0));
    Timed t("k_adler", g.s_adler);
    if (nbuf == 1) {  // one buffer: 64 KiB chunks, twice the workgroups
      const uint32_t nch = (uint32_t)((hb[0].n + ADLER_CHUNK - 1) / ADLER_CHUNK);
      hipLaunchKernelGGL(k_adler, dim3(nch), dim3(ADLER_THREADS), 0, g.s_adler, d_in, hb[0].in_off, hb[0].n, adler);
    } else {
      hipLaunchKernelGGL(k_adler_blocks, dim3(nblk), dim3(ADLER_THREADS), 0, g.s_adler, d_in, dbufs, dblks, adler);
    }
  }
  HIPCHK(hipEventRecord(g.ev_a1, g.s_adler));
  const bool sort_dbg = getenv("ZES_DEBUG_PHASES") != nullptr;
  if (sort_dbg && (rc = phases_arm(zes_sort_set_dbg, nblk))) return rc;
  static const bool use_index = getenv("ZES_NO_INDEX") == nullptr;
  rc = launch_lz77(d_in, nblk, use_index, nbuf > 1 && nblk > 256, sort_dbg, [&]() -> int {
    if (!sort_dbg) return ZES_OK;
    return phases_print(zes_sort_set_dbg, nblk, 7,
                        "zes sort steps (avg cycles over %u blocks): zero %.0f count %.0f flags %.0f level 2 + compact %.0f stage %.0f three passes %.0f sd/inv %.0f\n");
  });
  if (rc) return rc;
  if (sort_dbg) {  // (the parser's stamps: armed inside launch_lz77, in front of its two parse launches)
    if ((rc = phases_print(zes_parse_set_dbg, nblk, 7, "zes parse steps (avg cycles over %u blocks): A %.0f B %.0f C %.0f D1 %.0f D2 %.0f D3 %.0f out %.0f\n"))) return rc;
    if ((rc = phases_arm(zes_huff_set_dbg, nblk))) return rc;
  }
  ZesRes* res_direct = (nbuf <= DEFLATE_DIRECT_BUFS && g.pinned_dev) ? g.pinned_dev->def.res : nullptr;
  {
    Timed t("k_huff");
    hipLaunchKernelGGL(k_huff, dim3(nblk), dim3(HUFF_THREADS_HOST), 0, g.stream, dblks, (const uint32_t*)g.hists.p,
                       (uint32_t*)g.codes.p, (uint32_t*)g.hdrs.p);
  }
  if (sort_dbg && (rc = phases_print(zes_huff_set_dbg, nblk, 7,
                                     "zes huff steps (avg cycles over %u blocks): rank sorts %.0f both alphabets' levels %.0f codes %.0f run-length coding %.0f its code %.0f header bits %.0f totals+out %.0f\n")))
    return rc;
  {
    HIPCHK(hipStreamWaitEvent(g.stream, g.ev_a1, 0));  // the checksums
    Timed t("k_layout");
    // (the results go straight into the page-locked read-back area when they fit it: no copy command behind the kernels)
    hipLaunchKernelGGL(k_layout, dim3(nbuf), dim3(256), 0, g.stream, d_out, dbufs, dblks, adler, res_direct ? res_direct : (ZesRes*)g.res.p);
  }
  if (sort_dbg && (rc = phases_arm(zes_emit_set_dbg, nblk))) return rc;
  {
    Timed t("k_emit");
    hipLaunchKernelGGL(k_emit, dim3(nblk), dim3(EMIT_THREADS), 0, g.stream, d_out, dbufs, dblks, (uint32_t*)g.idx_a.p,
                       (const uint32_t*)g.codes.p, (const uint32_t*)g.hdrs.p, d_in, (const uint32_t*)g.idx_b.p, (const uint32_t*)g.mlist.p);
  }
  // (this kernel's stamps 2 .. 6 are no clocks but the first wave's cycles in each step, summed over the block's tiles)
  if (sort_dbg && (rc = phases_print(zes_emit_set_dbg, nblk, 1,
                                     "zes emit steps (avg cycles over %u blocks, first wave): whole %.0f = header copy %.0f build %.0f scan %.0f stage %.0f flush %.0f\n")))
    return rc;
  HIPCHK(hipGetLastError());
  ZesRes* r = g.pinned->def.res;
  if (nbuf > DEFLATE_DIRECT_BUFS) {
    if (nbuf > g.res_more_n) {
      if (g.res_more) HIPCHK(hipHostFree(g.res_more));
      g.res_more = nullptr;
      g.res_more_n = 0;
      HIPCHK(hipHostMalloc((void**)&g.res_more, sizeof(ZesRes) * nbuf * 2, hipHostMallocDefault));
      g.res_more_n = (size_t)nbuf * 2;
    }
    r = g.res_more;
  }
  if (!res_direct) HIPCHK(hipMemcpyAsync(r, g.res.p, sizeof(ZesRes) * nbuf, hipMemcpyDeviceToHost, g.stream));
  if (one && one->defer) return ZES_OK;  // (the caller reads def.res after its own synchronisation, deflate_host_pipelined)
  HIPCHK(hipStreamSynchronize(g.stream));
  collect_times();
  for (uint32_t k = 0; k < nbuf; k++) {
    out_len[live[k]] = r[k].out_len;
    status[live[k]] = r[k].status;
  }
  if (one) one->adler = r[0].aux;
  return ZES_OK;
}

// One buffer at d_in+in_off, its result at d_out+out_off (16-byte aligned) with room for cap bytes: inflate_one's mirror.
// Returns the reference-equivalent status; *out_len = bytes produced (a range: bits), or the capacity needed on NOSPACE.
int deflate_one(const uint8_t* d_in, uint64_t in_off, uint64_t n, uint8_t* d_out, uint64_t out_off, uint64_t cap, uint64_t* out_len,
                DeflateRange* range = nullptr) {
  int32_t st = 0;
  const int rc = deflate_batch_core(d_in, &in_off, &n, d_out, &out_off, &cap, out_len, &st, 1, range);
  return rc ? rc : st;
}

// ---- inflate ----
int read_res(ZesRes* out) {
  HIPCHK(hipMemcpyAsync(&g.pinned->res1, g.res.p, sizeof(ZesRes), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  *out = g.pinned->res1;
  return ZES_OK;
}

struct InfJob {
  uint64_t in_off, c, out_off, cap;
  uint64_t out_len;
  int status;  // reference-equivalent status once done
  int tier;    // 0 = not decoded yet
  // a piece of a longer stream on its way through the segment-parallel tier (inflate_segments_pieces): where work item
  // 0 starts, how much output exists in front of out_off, "a chain that ends in front of the piece's last, cut block
  // is fine"; out: the bit behind the last block decoded (relative to in_off), whether it was the stream's final one
  uint32_t start0 = 16, hist = 0;
  bool partial = false, final_seen = false;
  uint64_t end_bit = 0;
  int btype0 = -1;  // BTYPE of the block at bit 16, when the block-parallel tier's scan has sent it along (-1: not known)
  // the caller wants end_bit of the whole stream once it is decoded (zes_inflate_raw_used, the trailer checks): the tiers
  // that do not have it on the host anyway read it back
  bool want_end = false;
};

// a job's entry of a table of buffers: where its stream and its output are; the rest is zero, and each caller's own
ZesInfBuf inf_buf(const InfJob& j) {
  ZesInfBuf b;
  memset(&b, 0, sizeof b);
  b.in_off = j.in_off;
  b.c = j.c;
  b.out_off = j.out_off;
  b.cap = j.cap;
  return b;
}

bool t1_eligible(const InfJob& j, uint32_t flags) { return !(flags & (ZES_F_NO_FASTPATH | ZES_F_PIECES)) && j.c >= 64 && j.c < (1ull << 29); }

// The header test of the block-start search, two launches: k_inf_verify (a lane per survivor, the first VERIFY_STEPS
// code-length symbols: nearly all survivors end there) and k_inf_verify_long (a wave per survivor still alive: the
// real headers, ~300 symbols each).  `total_c`: compressed bytes behind the survivors (sizes the grids).
int launch_verify(const uint8_t* d_in, const ZesInfBuf* dbufs, uint32_t surv_cap, uint32_t* counters, uint32_t* cnt, uint32_t loose,
                  uint64_t total_c) {
  int rc;
  // the list of the long pass: one survivor in ~350 bytes of stream, one in eight of them listed; ten times that
  const uint32_t vlong_cap = (uint32_t)std::min<uint64_t>(total_c / 256 + 4096, surv_cap);
  if ((rc = ensure(g.vlong, (size_t)vlong_cap * 24))) return rc;
  // one lane per survivor: waves for all of them at once (the loop in the kernel takes what is beyond)
  uint32_t nwg = (uint32_t)std::min<uint64_t>(total_c / 16384 + 1, 8192);
  if (const char* e = getenv("ZES_VERIFY_DIV")) nwg = (uint32_t)std::min<uint64_t>(total_c / (uint64_t)atoi(e) + 1, 8192);
  {
    Timed t("k_inf_verify");
    hipLaunchKernelGGL(k_inf_verify, dim3(nwg), dim3(64), 0, g.stream, d_in, dbufs, (const unsigned long long*)g.surv.p, surv_cap, counters,
                       (uint32_t*)g.cand.p, cnt, loose, (uint32_t*)g.vlong.p, vlong_cap,
                       getenv("ZES_VERIFY_STEPS") ? (uint32_t)atoi(getenv("ZES_VERIFY_STEPS")) : 32u);
  }
  {
    Timed t("k_inf_verify_long");
    // one wave per listed survivor (about one in 2800 bytes of stream)
    // (a wave per item, no second item for most waves: 64 MiB of random bytes list 26 000 — 0.076 -> 0.065 ms against a cap of 8192)
    const uint32_t nlong = (uint32_t)std::min<uint64_t>(total_c / 2048 + 1, 32768);
    hipLaunchKernelGGL(k_inf_verify_long, dim3(nlong), dim3(64), 0, g.stream, d_in, dbufs, (const unsigned long long*)g.surv.p, surv_cap,
                       counters, (uint32_t*)g.cand.p, cnt, loose, (const uint32_t*)g.vlong.p, vlong_cap);
  }
  if (getenv("ZES_VERIFY_DBG")) {
    uint32_t hc[4];
    HIPCHK(hipStreamSynchronize(g.stream));
    HIPCHK(hipMemcpy(hc, counters, 16, hipMemcpyDeviceToHost));
    fprintf(stderr, "verify: survivors %u, handed to the wave form %u\n", hc[0], hc[1]);
  }
  return ZES_OK;
}

// ZES_DEBUG_HOSTLAPS: host-side time between the synchronisation points of an inflate call (which round trips a call pays)
void host_lap(const char* what) {
  static const bool on = getenv("ZES_DEBUG_HOSTLAPS") != nullptr;
  if (!on) return;
  static thread_local std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  const auto now = std::chrono::steady_clock::now();
  fprintf(stderr, "zes host lap: %-34s %8.1f us\n", what, std::chrono::duration<double, std::micro>(now - last).count());
  last = now;
}

// ZES_DEBUG_PHASES: average shader-clock cycles per phase of the block decoder (k_inf_block_par*, k_inf_seg_block_par)
int print_par_phases(const unsigned long long* dbg, uint64_t work) {
    std::vector<unsigned long long> h((size_t)work * ZES_PAR_DBG_ROW);
    HIPCHK(hipMemcpy(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost));
    double acc[8] = {0}, t0[3] = {0}, t15[3] = {0}, fb_lanes = 0, fb_waves = 0, hs[5] = {0}, p4[5] = {0}, why[3] = {0};
    uint32_t cntd = 0;
    for (uint32_t i = 0; i < work; i++) {
      const unsigned long long* r = &h[(size_t)i * ZES_PAR_DBG_ROW];
      if (!r[7]) continue;
      cntd++;
      for (int k = 1; k < 8; k++) acc[k] += (double)(r[k] - r[k - 1]);
      for (int k = 0; k < 3; k++) {  // table-phase steps relative to the end of the header phase
        t0[k] += (double)(r[8 + k] - r[1]);
        t15[k] += (double)(r[12 + k] - r[1]);
      }
      hs[0] += (double)(r[16] - r[0]);
      for (int k = 1; k < 5; k++) hs[k] += (double)(r[16 + k] - r[15 + k]);
      for (int k = 0; k < 5; k++) p4[k] += (double)r[24 + k];
      fb_lanes += (double)r[11];
      fb_waves += (double)r[15];
      for (int k = 0; k < 3; k++) why[k] += (double)r[29 + k];
    }
    fprintf(stderr, "zes phases (avg cycles over %u blocks): hdr %.0f tables %.0f compose %.0f count %.0f emit %.0f resolve %.0f flush %.0f\n",
            cntd, acc[1] / cntd, acc[2] / cntd, acc[3] / cntd, acc[4] / cntd, acc[5] / cntd, acc[6] / cntd, acc[7] / cntd);
    fprintf(stderr, "zes table steps, cycles since the header: first wave window %.0f landing %.0f fill %.0f | last wave %.0f %.0f %.0f\n",
            t0[0] / cntd, t0[1] / cntd, t0[2] / cntd, t15[0] / cntd, t15[1] / cntd, t15[2] / cntd);
    fprintf(stderr, "zes header steps (avg cycles): staging %.0f fixed fields + code-length code %.0f code lengths %.0f lit/len tables %.0f distance tables %.0f\n",
            hs[0] / cntd, hs[1] / cntd, hs[2] / cntd, hs[3] / cntd, hs[4] / cntd);
    fprintf(stderr, "zes resolve steps (avg cycles): carry+clear %.0f fill %.0f jumping %.0f copy %.0f | %.1f barrier rounds per block\n", p4[0] / cntd,
            p4[1] / cntd, p4[2] / cntd, p4[3] / cntd, p4[4] / cntd);
    {
      double c0 = 0, c15 = 0;
      for (uint32_t i = 0; i < work; i++) {
        const unsigned long long* r = &h[(size_t)i * ZES_PAR_DBG_ROW];
        if (!r[7]) continue;
        c0 += (double)(r[22] - r[3]);
        c15 += (double)(r[23] - r[3]);
      }
      fprintf(stderr, "zes count pass, cycles since its start: first wave through %.0f, last wave %.0f\n", c0 / cntd, c15 / cntd);
    }
    fprintf(stderr, "zes 8-bit table path: %.2f lanes in %.2f waves per block fell back to the generic construction (segment shape or list full %.2f, three positions under one token %.2f, look-back %.2f)\n", fb_lanes / cntd, fb_waves / cntd, why[0] / cntd, why[1] / cntd, why[2] / cntd);
    return ZES_OK;
}

// The block-parallel tier's launches, each spelled out once.
// The search of a table of buffers for block starts: k_inf_scan (the cheap tests at every bit position; the survivors go
// to g.surv, so whatever a later call knew about that list is void) and the header test.  Which rules the two apply:
struct SearchMode { uint32_t scan, loose; };
// T1 looks for the reference's own blocks (ZES_F_LOOSE_CANDIDATES: for headers any encoder writes)
SearchMode t1_search_mode(uint32_t flags) { return (flags & ZES_F_LOOSE_CANDIDATES) ? SearchMode{1u, 1u} : SearchMode{2u, 0u}; }
// T2: other encoders do not follow the reference's run-length rules for code lengths: loose candidates (the BFINAL rule
// of the scan holds for every encoder's streams: it stays on; only the verify rules are the reference's own)
constexpr SearchMode T2_SEARCH = {0u, 1u};
int launch_search(const uint8_t* d_in, const ZesInfBuf* dbufs, uint32_t nbuf, uint32_t chunks, uint32_t surv_cap, uint32_t* counters,
                  uint32_t* cnt, uint8_t* first, SearchMode mode, uint64_t total_c) {
  {
    Timed t("k_inf_scan");
    g.sv.drop();
    hipLaunchKernelGGL(k_inf_scan, dim3(chunks), dim3(INF_SCAN_THREADS), 0, g.stream, d_in, dbufs, nbuf, (unsigned long long*)g.surv.p,
                       surv_cap, counters, first, mode.scan, (const uint8_t*)g.kraft.p);
  }
  return launch_verify(d_in, dbufs, surv_cap, counters, cnt, mode.loose, total_c);
}
// The block decoder over `items` work items of the table's buffers (two: the variant whose transfer tables look at two
// windows, for compressible data).  redo null: the first decode, a work item per candidate — every item finds its own
// rank in the unsorted list and leaves the sorted one for the chain check.  redo set: chain members decoded again into
// their own slots, work item -> slot through redo[], slot -> candidate through the chain kernel's map.
void launch_block_par(const char* name, bool two, uint32_t items, const uint8_t* d_in, uint8_t* d_out, const ZesInfBuf* dbufs, uint32_t nbuf,
                      const uint32_t* cnt, unsigned long long* dbg, const uint32_t* redo, const ZesParMirror& mir) {
  Timed t(name);
  hipLaunchKernelGGL(two ? k_inf_block_par2 : k_inf_block_par, dim3(items), dim3(PAR_THREADS), 0, g.stream, d_in, d_out, dbufs, nbuf, cnt,
                     (const uint32_t*)g.cand_sorted.p, redo ? (const uint32_t*)g.map.p : nullptr, (ZesCandRes*)g.cres.p, dbg, redo,
                     redo ? nullptr : (const uint32_t*)g.cand.p, redo ? nullptr : (uint32_t*)g.cand_sorted.p, mir);
}

// scratch of a T1 search + decode over nbuf buffers with room for `cands` candidates in all
int t1_pools(uint32_t nbuf, uint32_t surv_cap, uint64_t cands, size_t counter_bytes, uint32_t nres) {
  int rc;
  if ((rc = ensure(g.ibufs, sizeof(ZesInfBuf) * (nbuf + 1)))) return rc;
  if ((rc = ensure(g.surv, (size_t)surv_cap * 8))) return rc;
  if ((rc = ensure(g.cand, (size_t)cands * 4))) return rc;
  if ((rc = ensure(g.cand_sorted, (size_t)cands * 4))) return rc;
  if ((rc = ensure(g.cres, sizeof(ZesCandRes) * cands))) return rc;
  if ((rc = ensure(g.counters, counter_bytes))) return rc;
  return ensure(g.res, sizeof(ZesRes) * nres);
}

// T1's verdict on one buffer taken on the host: zes_chain.h's rule — k_inf_chain's — on what the block decoder left in
// page-locked memory (start[k] = the bit candidate k's block starts at, rank order; hc: the search's counters, survivors
// in word 0, candidates in word 4; b: the buffer's table entry; work: work items launched).  map: see zes_chain_decide.
ZesRes t1_host_chain(const uint32_t* start, const ZesCandRes* cres, const uint32_t* hc, uint32_t surv_cap, const ZesInfBuf& b, uint64_t work,
                     uint32_t* map) {
  const ZesChainView v = {start, cres, std::min(hc[4], b.cand_cap), 0u};
  // (no survivors: nothing that looks like this format; more than the list holds: a poisoned count)
  const uint32_t nwork = hc[0] != 0 && hc[0] <= surv_cap ? (uint32_t)std::min<uint64_t>(v.n, work) : 0u;
  return zes_chain_decide(v, hc[4], b.cand_cap, nwork, 16u + (uint64_t)b.start_rel, map);
}

// T1 over a group of buffers: every launch covers all of them (scan, verify, sort, one decode work
// item per candidate block, chain check), two host synchronisations for the whole group.  Jobs the
// tier settles get tier = 1; the others are left for the per-buffer tiers.
struct T1Group {  // the group between the steps of inflate_t1_group
  const uint8_t* d_in;
  uint8_t* d_out;
  InfJob* jobs;
  const uint32_t* ids;
  uint32_t nbuf, flags;
  bool check_first, one;  // one buffer: one synchronisation per call (t1_decode)
  ZesInfBuf* hb;          // page-locked: the table, ...
  uint32_t* hc;           // ... the search's counters, ...
  ZesRes* hres;           // ... the chain results
  uint64_t chunks = 0, cands = 0, total_c = 0, work = 0;  // work: work items launched
  uint32_t surv_cap = 0;
  size_t cnt_bytes = 0;
  const ZesInfBuf* dbufs = nullptr;
  uint32_t *counters = nullptr, *cnt = nullptr;
  unsigned long long* dbg = nullptr;
  bool hostchain = false;  // the host walks the chain (t1_decode decides)
  std::vector<uint32_t> ncand;
  std::vector<ZesRes> r1;  // every buffer's verdict
};
// a step's answer beside ZES_OK and an error: nothing more for this tier, what it has not settled goes to the per-buffer tiers
constexpr int T1_OVER = 1;

// what the scan sent along of buffer i's first byte: the BTYPE of the block at bit 16 and the CM nibble (src/zlib.ts:13-16).
// true: not a deflate stream, the job is settled
bool t1_first_byte(T1Group& t, uint32_t i, uint8_t fb) {
  InfJob& j = t.jobs[t.ids[i]];
  if (fb & 0x40u) j.btype0 = (fb >> 4) & 3;
  if (!t.check_first || (fb & 15u) == 8u) return false;
  j.status = ZES_E_NOT_DEFLATE;
  j.tier = -1;
  return true;
}

// step 1: the table of buffers, the pools sized for it, both on their way to the device
int t1_table(T1Group& t) {
  int rc;
  g.sv.drop();  // (g.surv is about to be rewritten)
  ZesInfBuf* hb = t.hb;
  for (uint32_t i = 0; i < t.nbuf; i++) {
    const InfJob& j = t.jobs[t.ids[i]];
    ZesInfBuf& b = hb[i] = inf_buf(j);
    b.first_chunk = (uint32_t)t.chunks;
    b.cand_base = (uint32_t)t.cands;
    // a reference-made stream has one block per 131072 bytes of output: more candidates than the caller's capacity
    // has blocks (plus room for false ones) means another encoder wrote the stream — counted as an overflow, and the
    // sort never sees more than this many (a zlib stream with 250-byte blocks has 250 000 of them)
    b.cand_cap = (uint32_t)std::min<uint64_t>(j.c / 64 + 64, j.cap / ZES_BLK + 65);
    b.own_rel = 0xFFFFFFFFu;
    t.chunks += (j.c + INF_SCAN_BYTES - 1) / INF_SCAN_BYTES;
    t.cands += b.cand_cap;
    t.total_c += j.c;
  }
  if (t.chunks >= (1ull << 31) || t.cands >= (1ull << 31)) return T1_OVER;  // leave the jobs to the per-buffer tiers
  const uint32_t nbuf = t.nbuf;
  memset(&hb[nbuf], 0, sizeof(ZesInfBuf));
  hb[nbuf].first_chunk = (uint32_t)t.chunks;
  hb[nbuf].cand_base = (uint32_t)t.cands;
  if (t.one) {  // see t1_decode
    hb[1].work_first = ZES_WORK_AUTO;
    hb[1].cand_cap = hb[0].cand_cap;
  }
  t.surv_cap = (uint32_t)std::min<uint64_t>(t.total_c / 4 + 1024ull * nbuf, 1ull << 30);
  t.cnt_bytes = t1_cnt_bytes(nbuf);
  if ((rc = t1_pools(nbuf, t.surv_cap, t.cands, t.cnt_bytes, nbuf))) return rc;
  if ((rc = ensure(g.map, (size_t)t.cands * 4))) return rc;
  t.dbufs = (const ZesInfBuf*)g.ibufs.p;
  t.counters = (uint32_t*)g.counters.p;
  t.cnt = t.counters + 4;
  if (t.one) {  // table and cleared counters straight from kernel arguments
    hipLaunchKernelGGL(k_inf_set_table1, dim3(1), dim3(64), 0, g.stream, hb[0], hb[1], (ZesInfBuf*)g.ibufs.p, t.counters,
                       (uint32_t)(t.cnt_bytes / 4));
  } else {
    HIPCHK(hipMemcpyAsync(g.ibufs.p, hb, sizeof(ZesInfBuf) * (nbuf + 1), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemsetAsync(g.counters.p, 0, t.cnt_bytes, g.stream));
  }
  return ZES_OK;
}

// step 3: a decode work item per candidate.
// One buffer: nothing has to come back before the decode is launched.  The grid is sized for the most
// blocks the caller's capacity can hold (plus room for false candidates); the kernels take the real
// candidate count from device memory (table sentinel ZES_WORK_AUTO) and the host reads counters and
// result together — one synchronisation per call.  Several buffers: the counts come back first.
int t1_decode(T1Group& t) {
  int rc;
  const uint32_t nbuf = t.nbuf;
  ZesInfBuf* hb = t.hb;
  uint32_t* hc = t.hc;
  if (!t.one) {
    HIPCHK(hipMemcpyAsync(hc, g.counters.p, t.cnt_bytes, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));  // the table upload has completed too: hb may be rewritten
    const uint8_t* hfirst = (const uint8_t*)(hc + 4 + nbuf);
    for (uint32_t i = 0; i < nbuf; i++)
      if (t1_first_byte(t, i, hfirst[i])) hc[4 + i] = 0;  // no candidates are looked at
    const uint32_t nsurv0 = hc[0];
    if (nsurv0 != 0 && nsurv0 <= t.surv_cap)  // (else: nothing that looks like this format, or a poisoned count)
      for (uint32_t i = 0; i < nbuf; i++) {
        t.ncand[i] = hc[4 + i];
        hb[i].work_first = (uint32_t)t.work;
        if (t.ncand[i] > 0 && t.ncand[i] <= hb[i].cand_cap) t.work += t.ncand[i];
      }
    hb[nbuf].work_first = (uint32_t)t.work;
    if (t.work == 0) return T1_OVER;
    HIPCHK(hipMemcpyAsync(g.ibufs.p, hb, sizeof(ZesInfBuf) * (nbuf + 1), hipMemcpyHostToDevice, g.stream));
  } else {
    t.work = hb[1].cand_cap;  // the launch bound written into the sentinel
  }
  if (getenv("ZES_DEBUG_PHASES")) {
    if ((rc = ensure(g.dbg, (size_t)t.work * ZES_PAR_DBG_ROW * 8))) return rc;
    HIPCHK(hipMemsetAsync(g.dbg.p, 0, (size_t)t.work * ZES_PAR_DBG_ROW * 8, g.stream));
    t.dbg = (unsigned long long*)g.dbg.p;
  }
  // compressible data (the streams are shorter than 0.7 of the room for their outputs): the variant whose transfer
  // tables look at two windows; incompressible data runs ~4 % faster in the smaller kernel
  uint64_t total_cap = 0;
  for (uint32_t i = 0; i < nbuf; i++) total_cap += t.jobs[t.ids[i]].cap;
  const bool two = t.total_c * 10 < total_cap * 7;
  // One buffer and a launch bound the mirror area holds: every work item also puts its result and its block's start bit
  // into page-locked host memory, work item 0 the counters, and the HOST follows the chain after the one synchronisation —
  // what k_inf_chain does, on a few hundred 16-byte records: no chain kernel behind this one (11 us + a kernel boundary of
  // a 0.8 ms call).  Only a chain that needs the slots moved (false candidates between the blocks) still runs that kernel,
  // for its map.
  ZesParMirror mir{};
  if (t.one && !g.device_chain && t.work <= MIRROR_ITEMS && g.mirror_dev && g.pinned_dev) {
    mir.cres_host = g.mirror_dev->cres;
    mir.start_host = g.mirror_dev->start;
    mir.counters = t.counters;
    mir.counters_host = g.pinned_dev->t1.counters;
    mir.counter_words = (uint32_t)(t.cnt_bytes / 4);
    t.hostchain = true;
  }
  launch_block_par(two ? "k_inf_block_par2" : "k_inf_block_par", two, (uint32_t)t.work, t.d_in, t.d_out, t.dbufs, nbuf, t.cnt, t.dbg, nullptr, mir);
  return ZES_OK;
}

// k_inf_chain over the group, its results on their way to t.hres
int t1_device_chain(T1Group& t) {
  Timed tm("k_inf_chain");
  // one buffer: the kernel puts its result and the counters straight into the page-locked read-back area (no copy
  // commands behind the kernels: ~10 us of a 0.8 ms call)
  const bool direct = t.one && g.pinned_dev;
  hipLaunchKernelGGL(k_inf_chain, dim3(t.nbuf), dim3(256), 0, g.stream, t.dbufs, (const uint32_t*)t.cnt, (const uint32_t*)g.cand_sorted.p,
                     (const ZesCandRes*)g.cres.p, (const uint32_t*)nullptr, (uint32_t*)g.map.p,
                     direct ? g.pinned_dev->t1.res : (ZesRes*)g.res.p, (const uint32_t*)t.counters, (uint32_t)(t.cnt_bytes / 4),
                     direct ? g.pinned_dev->t1.counters : (uint32_t*)nullptr);
  if (!direct) {
    if (t.one) HIPCHK(hipMemcpyAsync(t.hc, g.counters.p, t.cnt_bytes, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(t.hres, g.res.p, sizeof(ZesRes) * t.nbuf, hipMemcpyDeviceToHost, g.stream));
  }
  return ZES_OK;
}

// step 4: every buffer's verdict in t.r1, from k_inf_chain or — one buffer — the host's walk on the mirror; behind it
// the one-buffer call learns what the several-buffer one read back in t1_decode
int t1_verdicts(T1Group& t) {
  int rc;
  uint32_t* hc = t.hc;
  if (!t.hostchain && (rc = t1_device_chain(t))) return rc;
  host_lap("(work before the block-parallel tier)");
  HIPCHK(hipStreamSynchronize(g.stream));
  host_lap("T1: search + decode + chain");
  if (t.hostchain) {
    ZesRes r = t1_host_chain(g.mirror->start, g.mirror->cres, hc, t.surv_cap, t.hb[0], t.work, nullptr);
    if (r.status == 2) {  // the slots are shifted: the chain kernel's map is needed (rare)
      if ((rc = t1_device_chain(t))) return rc;
      HIPCHK(hipStreamSynchronize(g.stream));
      r = t.hres[0];
    } else {
      t.hres[0] = r;
    }
    if (getenv("ZES_DEBUG")) {
      const ZesCandRes* hcr = g.mirror->cres;
      const uint32_t* hst = g.mirror->start;
      fprintf(stderr, "zes T1 host chain: nsurv %u cnt %u cap %u work %llu -> status %d out_len %llu | start0 %u", hc[0], hc[4], t.hb[0].cand_cap,
              (unsigned long long)t.work, r.status, (unsigned long long)r.out_len, hst[0]);
      for (uint32_t k = 0; k < std::min<uint32_t>(hc[4], 10u); k++)
        fprintf(stderr, " [%u: start %u end %llu len %u fl %u]", k, hst[k], (unsigned long long)hcr[k].end_bit, hcr[k].out_len, hcr[k].flags);
      fprintf(stderr, "\n");
    }
  }
  const uint32_t nsurv = hc[0];
  if (t.one) {
    const InfJob& j = t.jobs[t.ids[0]];
    if (t1_first_byte(t, 0, ((const uint8_t*)(hc + 5))[0])) return T1_OVER;
    t.ncand[0] = hc[4];
    if (nsurv != 0 && nsurv <= t.surv_cap && !(t.flags & ZES_F_LOOSE_CANDIDATES))  // the scan ran to its end and its list is whole
      g.sv.note(g.surv, t.d_in, j.in_off, j.c, nsurv);
    // nothing that looks like this format, a poisoned count, or more candidates than were launched
    if (nsurv == 0 || nsurv > t.surv_cap || t.ncand[0] == 0 || t.ncand[0] > t.hb[0].cand_cap || t.ncand[0] > t.work) return T1_OVER;
    t.hb[0].work_first = 0;
    t.work = t.ncand[0];
  }
  t.r1.assign(t.hres, t.hres + t.nbuf);
  if (t.dbg && (rc = print_par_phases(t.dbg, t.work))) return rc;
  if (getenv("ZES_DEBUG")) {
    for (uint32_t i = 0, shown_b = 0; i < t.nbuf && shown_b < 4; i++) {
      const ZesRes& r = t.r1[i];
      if (r.status == 0) continue;
      shown_b++;
      const uint32_t nc = std::min(t.ncand[i], t.hb[i].cand_cap);
      fprintf(stderr, "zes T1: buf %u c=%llu nsurv(all)=%u ncand=%u chain status=%d aux=%u out_len=%llu\n", t.ids[i],
              (unsigned long long)t.hb[i].c, nsurv, t.ncand[i], r.status, r.aux, (unsigned long long)r.out_len);
      if (r.status != 1 || nc == 0) continue;
      std::vector<ZesCandRes> hcr(nc);
      std::vector<uint32_t> hcand(nc);
      HIPCHK(hipMemcpy(hcr.data(), (const ZesCandRes*)g.cres.p + t.hb[i].cand_base, sizeof(ZesCandRes) * nc, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(hcand.data(), (const uint32_t*)g.cand_sorted.p + t.hb[i].cand_base, 4 * (size_t)nc, hipMemcpyDeviceToHost));
      const ZesChainView v = {hcand.data(), hcr.data(), nc, 16u};
      int shown = 0;
      for (uint32_t k = 0; k < nc && shown < 6; k++) {  // candidates that do not link to the next one (the last: not decoded)
        if (k + 1 < nc ? zes_chain_link(v, hcr[k], k + 1) : (hcr[k].flags & ZES_CAND_OK) != 0) continue;
        fprintf(stderr, "  cand %u start=%u end_bit=%llu next_start=%u out_len=%u flags=%u\n", k, (uint32_t)zes_chain_start(v, k),
                (unsigned long long)hcr[k].end_bit, k + 1 < nc ? (uint32_t)zes_chain_start(v, k + 1) : 0, hcr[k].out_len, hcr[k].flags);
        shown++;
      }
    }
  }
  return ZES_OK;
}

// the end bit of the block at index idx of the device's result list
int cand_end_bit(size_t idx, uint64_t* end_bit) {
  ZesCandRes last;
  HIPCHK(hipMemcpy(&last, (const ZesCandRes*)g.cres.p + idx, sizeof last, hipMemcpyDeviceToHost));
  *end_bit = last.end_bit;
  return ZES_OK;
}

// step 5, for a buffer whose candidate list holds false positives between the blocks: every true block decoded fine, but
// the blocks behind a false candidate sit one (or more) slots too far right.  The chain kernel left the true
// chain in map[] (true block k = candidate map[k]) and has checked it block by block, so the blocks only
// have to move: through a scratch copy, because sources and destinations overlap.  A block whose slot was cut
// off by the caller's capacity (typically the last one) is decoded again, straight into its own slot.
// r: the buffer's verdict, status 2 -> 0 (repaired) or 1; out_len already holds the chain's total.
int t1_repair_slots(T1Group& t, uint32_t i, ZesRes& r) {
  int rc;
  const ZesInfBuf* hb = t.hb;
  const uint32_t K = r.aux;
  InfJob& j = t.jobs[t.ids[i]];
  std::vector<uint32_t> hmap(K);
  HIPCHK(hipMemcpyAsync(hmap.data(), (const uint32_t*)g.map.p + hb[i].cand_base, (size_t)K * 4, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  if (j.want_end && K && (rc = cand_end_bit(hb[i].cand_base + hmap[K - 1], &j.end_bit))) return rc;
  std::vector<uint32_t> mv_src, mv_dst, redo;
  for (uint32_t k = 0; k < K; k++) {
    if (hmap[k] == k) continue;
    if ((uint64_t)(hmap[k] + 1u) * ZES_BLK <= j.cap) {
      mv_src.push_back(hmap[k]);
      mv_dst.push_back(k);
    } else {
      redo.push_back(k);
    }
  }
  const uint32_t nmv = (uint32_t)mv_src.size(), nre = (uint32_t)redo.size();
  if ((rc = ensure(g.mvlist, (size_t)(3 * nmv + nre + 4) * 4))) return rc;
  uint32_t* dl = (uint32_t*)g.mvlist.p;  // [src slots][dst slots][0..nmv)[redo]
  if (nmv) {
    if ((rc = ensure(g.scratch, (size_t)nmv * ZES_BLK))) return rc;
    std::vector<uint32_t> up(3 * (size_t)nmv);
    for (uint32_t q = 0; q < nmv; q++) {
      up[q] = mv_src[q];
      up[nmv + q] = mv_dst[q];
      up[2 * (size_t)nmv + q] = q;
    }
    HIPCHK(hipMemcpy(dl, up.data(), up.size() * 4, hipMemcpyHostToDevice));
    Timed tm("k_inf_move_slots");
    uint8_t* outb = t.d_out + j.out_off;
    hipLaunchKernelGGL(k_inf_move_slots, dim3(nmv * 32u), dim3(256), 0, g.stream, (uint8_t*)g.scratch.p, (const uint8_t*)outb,
                       (const uint32_t*)(dl + 2 * (size_t)nmv), (const uint32_t*)dl, nmv);
    hipLaunchKernelGGL(k_inf_move_slots, dim3(nmv * 32u), dim3(256), 0, g.stream, outb, (const uint8_t*)g.scratch.p,
                       (const uint32_t*)(dl + nmv), (const uint32_t*)(dl + 2 * (size_t)nmv), nmv);
  }
  bool ok = true;
  if (nre) {
    HIPCHK(hipMemcpy(dl + 3 * (size_t)nmv, redo.data(), (size_t)nre * 4, hipMemcpyHostToDevice));
    // a two-entry table for this buffer alone: K work items in all
    ZesInfBuf* one = g.pinned->t1.redo;
    one[0] = hb[i];
    one[0].work_first = 0;
    one[1] = hb[i];
    one[1].work_first = K;
    if ((rc = ensure(g.ibufs2, sizeof(ZesInfBuf) * 2))) return rc;
    HIPCHK(hipMemcpyAsync(g.ibufs2.p, one, sizeof(ZesInfBuf) * 2, hipMemcpyHostToDevice, g.stream));
    // cnt / candidates / map / results are indexed from this buffer's region: the table's cand_base does that
    launch_block_par("k_inf_block_par", false, nre, t.d_in, t.d_out, (const ZesInfBuf*)g.ibufs2.p, 1u, (const uint32_t*)t.cnt + i, nullptr,
                     (const uint32_t*)(dl + 3 * (size_t)nmv), ZesParMirror{});
    std::vector<ZesCandRes> hcr(nre);
    for (uint32_t q = 0; q < nre; q++)
      HIPCHK(hipMemcpyAsync(&hcr[q], (const ZesCandRes*)g.cres.p + hb[i].cand_base + redo[q], sizeof(ZesCandRes), hipMemcpyDeviceToHost,
                            g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (uint32_t q = 0; q < nre; q++) ok = ok && zes_chain_redone(hcr[q], redo[q] + 1u == K);
  }
  r.status = ok ? 0 : 1;
  return ZES_OK;
}

// step 6: tier, length, status and — where asked for — the stream's end bit of every accepted buffer
int t1_publish(T1Group& t) {
  int rc;
  // end bits that are still on the device (a group's chains were judged there): one segmented copy (k_gz_gather, 8 bytes a
  // buffer out of its closing block's record) and one read-back for all of them, not a copy command per buffer
  std::vector<ZesGzSeg> segs;
  std::vector<uint32_t> who;
  for (uint32_t i = 0; i < t.nbuf; i++) {
    const ZesRes& r = t.r1[i];
    if (r.status != 0) continue;
    InfJob& j = t.jobs[t.ids[i]];
    if (j.want_end && t.hres[i].status == 0 && r.aux) {  // (t1_repair_slots has filled it in for a status 2)
      if (t.hostchain) {
        j.end_bit = g.mirror->cres[r.aux - 1].end_bit;
      } else {
        segs.push_back(ZesGzSeg{sizeof(ZesCandRes) * ((uint64_t)t.hb[i].cand_base + r.aux - 1) + offsetof(ZesCandRes, end_bit), 0, 8, 0u, 0u});
        who.push_back(t.ids[i]);
      }
    }
    j.tier = 1;
    j.out_len = r.out_len;
    j.status = r.out_len > j.cap ? ZES_E_NOSPACE : ZES_OK;
  }
  if (segs.size() == 1) return cand_end_bit(segs[0].src_off / sizeof(ZesCandRes), &t.jobs[who[0]].end_bit);
  if (!segs.empty()) {
    const size_t o_dst = (size_t)gz_up16(sizeof(ZesGzSeg) * segs.size());
    for (size_t k = 0; k < segs.size(); k++) segs[k].dst_off = o_dst + 8 * k;
    if ((rc = ensure(g.crcseg, o_dst + 8 * segs.size()))) return rc;
    HIPCHK(hipMemcpyAsync(g.crcseg.p, segs.data(), sizeof(ZesGzSeg) * segs.size(), hipMemcpyHostToDevice, g.stream));
    {
      Timed tm("k_gz_gather");
      hipLaunchKernelGGL(k_gz_gather, dim3((uint32_t)segs.size(), 1), dim3(GZ_GATHER_THREADS), 0, g.stream, (const uint8_t*)g.cres.p,
                         (uint8_t*)g.crcseg.p, (const ZesGzSeg*)g.crcseg.p);
    }
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> ends(segs.size());
    HIPCHK(hipMemcpyAsync(ends.data(), (const uint8_t*)g.crcseg.p + o_dst, 8 * ends.size(), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    for (size_t k = 0; k < who.size(); k++) t.jobs[who[k]].end_bit = ends[k];
  }
  return ZES_OK;
}

int inflate_t1_group(const uint8_t* d_in, uint8_t* d_out, InfJob* jobs, const uint32_t* ids, uint32_t nbuf, bool check_first, uint32_t flags) {
  int rc;
  T1Group t{d_in, d_out, jobs, ids, nbuf, flags, check_first, nbuf == 1, g.pinned->t1.table, g.pinned->t1.counters, g.pinned->t1.res};
  t.ncand.resize(nbuf);
  const auto over = [](int r) { return r == T1_OVER ? ZES_OK : r; };
  if ((rc = t1_table(t))) return over(rc);
  // (k_inf_verify, measured on 64 MiB: 8192 workgroups 0.33 ms, 2048 0.26 ms, 512 0.36 ms — about one survivor in 256 input
  // bytes, and a lane should get a few of them)
  if ((rc = launch_search(d_in, t.dbufs, nbuf, (uint32_t)t.chunks, t.surv_cap, t.counters, t.cnt, (uint8_t*)(t.cnt + nbuf), t1_search_mode(flags),
                          t.total_c)))
    return rc;
  if ((rc = t1_decode(t))) return over(rc);
  if ((rc = t1_verdicts(t))) return over(rc);
  for (uint32_t i = 0; i < nbuf; i++)
    if (t.r1[i].status == 2 && (rc = t1_repair_slots(t, i, t.r1[i]))) return rc;
  return t1_publish(t);
}

// T1 over one PIECE of a reference-made stream: the blocks that start inside bits [lo_bit, own_bit) of the piece at
// d_in + in_off (c readable bytes: the piece and enough behind it for its last block, <= 144 KiB, and for the header
// of the block after it).  exact: the first block starts at lo_bit (known from the piece before); else the chain
// starts at the first block start found at or behind lo_bit.  Block k of the piece goes to d_out + out_off + k * 131072.
// handled = false: not a clean chain of reference-made blocks (the caller decodes the stream some other way).
struct RangeRes {
  bool handled = false;
  uint64_t out_len = 0, first_bit = 0, end_bit = 0;
  uint32_t nblocks = 0;
  bool final_block = false;
};
// A piece as both forms below see it: what is known before anything runs (skip: not for this tier; nothing: too short
// to hold a block start), how its lists are sized, and how what comes back for it is read.
struct RangePiece {
  bool skip = false, nothing = false, exact = false;
  uint64_t lo_bit = 0;
  uint32_t chunks = 0, surv_cap = 0, cand_cap = 0;
  uint32_t bound = 0;  // work items launched (range_begin launches over a bound, not over the candidate count)
};
uint32_t range_cand_cap(uint64_t c) { return (uint32_t)std::min<uint64_t>(c / 64 + 64, 1ull << 23); }  // (not from the output's capacity: a short output still gets its size)
uint32_t range_surv_cap(uint64_t c) { return (uint32_t)std::min<uint64_t>(c / 4 + 1024ull, 1ull << 30); }
// the piece and, unless skip or nothing, its table entry b0 and the sentinel b1 (the caller adds where the output goes)
RangePiece range_piece(uint64_t in_off, uint64_t c, uint64_t lo_bit, uint64_t own_bit, bool exact, ZesInfBuf* b0, ZesInfBuf* b1) {
  RangePiece pd;
  pd.exact = exact;
  pd.lo_bit = lo_bit;
  if (c >= (1ull << 29) || lo_bit < 16) pd.skip = true;
  else if (c * 8 < lo_bit + 64) pd.nothing = true;
  if (pd.skip || pd.nothing) return pd;
  pd.chunks = (uint32_t)((c + INF_SCAN_BYTES - 1) / INF_SCAN_BYTES);
  pd.surv_cap = range_surv_cap(c);
  pd.cand_cap = pd.bound = range_cand_cap(c);
  memset(b0, 0, sizeof *b0);
  memset(b1, 0, sizeof *b1);
  b0->in_off = in_off;
  b0->c = c;
  b0->cand_cap = pd.cand_cap;
  b0->start_rel = (uint32_t)(lo_bit - 16);
  b0->own_rel = (uint32_t)std::min<uint64_t>(own_bit >= 16 ? own_bit - 16 : 0, 0xFFFFFFFEull);
  b0->range_flags = (exact ? 0u : ZES_START_ANY) | ZES_OWN_ONLY;
  b1->first_chunk = pd.chunks;
  b1->cand_base = pd.cand_cap;
  return pd;
}
// scratch for a piece of up to c bytes
int range_pools(uint64_t c, size_t counter_bytes) { return t1_pools(1, range_surv_cap(c), range_cand_cap(c), counter_bytes, 2); }
// a range without a block start (a piece in the middle of one block): nothing to decode, and that is an answer
void range_nothing(const RangePiece& pd, RangeRes* rr) {
  if (pd.exact) return;
  rr->handled = true;
  rr->first_bit = rr->end_bit = pd.lo_bit;
}
// the search's counters (survivors in word 0, candidates in word 4): true when the piece has candidates that were, or
// can now be, decoded; false: *rr is the answer (not handled: a list overflowed, or more candidates than work items)
bool range_found(const RangePiece& pd, const uint32_t* hc, RangeRes* rr) {
  const uint32_t nsurv = hc[0], ncand = hc[4];
  if (nsurv > pd.surv_cap || ncand > pd.cand_cap) return false;
  if (nsurv == 0 || ncand == 0) {
    range_nothing(pd, rr);
    return false;
  }
  return ncand <= pd.bound;
}
// k_inf_chain_range's two records
void range_result(const ZesRes* hres, RangeRes* rr) {
  if (hres[0].status != 0) return;
  rr->handled = true;
  rr->out_len = hres[0].out_len;
  rr->nblocks = hres[0].aux & 0x7FFFFFFFu;
  rr->final_block = (hres[0].aux >> 31) != 0;
  rr->end_bit = hres[1].out_len;
  rr->first_bit = hres[1].aux;
}

void launch_chain_range(const ZesInfBuf* dbufs, const uint32_t* cnt, unsigned long long* acc) {
  Timed t("k_inf_chain");
  hipLaunchKernelGGL(k_inf_chain_range, dim3(1), dim3(256), 0, g.stream, dbufs, cnt, (const uint32_t*)g.cand_sorted.p, (const ZesCandRes*)g.cres.p,
                     (ZesRes*)g.res.p, acc);
}

int inflate_t1_range(const uint8_t* d_in, uint64_t in_off, uint64_t c, uint64_t lo_bit, uint64_t own_bit, bool exact, uint8_t* d_out,
                     uint64_t out_off, uint64_t cap, uint32_t flags, RangeRes* rr) {
  int rc;
  *rr = RangeRes();
  ZesInfBuf* hb = g.pinned->t1.table;
  const RangePiece pd = range_piece(in_off, c, lo_bit, own_bit, exact, &hb[0], &hb[1]);
  if (pd.skip) return ZES_OK;
  if (pd.nothing) {
    range_nothing(pd, rr);
    return ZES_OK;
  }
  hb[0].out_off = out_off;
  hb[0].cap = cap;
  const size_t cnt_bytes = 16 + 4 + 4;  // counters[4], cnt[1], first byte
  if ((rc = range_pools(c, cnt_bytes))) return rc;
  const ZesInfBuf* dbufs = (const ZesInfBuf*)g.ibufs.p;
  uint32_t* counters = (uint32_t*)g.counters.p;
  uint32_t* cnt = counters + 4;
  HIPCHK(hipMemcpyAsync(g.ibufs.p, hb, sizeof(ZesInfBuf) * 2, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemsetAsync(g.counters.p, 0, cnt_bytes, g.stream));
  // (the scan's rule that a BFINAL position far from the end is no block start uses the end of the piece: a piece in
  // the middle of a stream merely keeps a few more survivors near its own end)
  if ((rc = launch_search(d_in, dbufs, 1u, pd.chunks, pd.surv_cap, counters, cnt, (uint8_t*)(cnt + 1), t1_search_mode(flags), c))) return rc;
  uint32_t* hc = g.pinned->t1.counters;
  HIPCHK(hipMemcpyAsync(hc, g.counters.p, cnt_bytes, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  if (!range_found(pd, hc, rr)) return ZES_OK;
  const uint32_t ncand = hc[4];
  hb[1].work_first = ncand;
  HIPCHK(hipMemcpyAsync(g.ibufs.p, hb, sizeof(ZesInfBuf) * 2, hipMemcpyHostToDevice, g.stream));
  launch_block_par("k_inf_block_par", c * 10 < cap * 7, ncand, d_in, d_out, dbufs, 1u, cnt, nullptr, nullptr, ZesParMirror{});
  launch_chain_range(dbufs, cnt, nullptr);
  ZesRes* hres = g.pinned->t1.res;
  HIPCHK(hipMemcpyAsync(hres, g.res.p, sizeof(ZesRes) * 2, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  if (getenv("ZES_RANGE_DBG")) {
    std::vector<uint32_t> hcand(ncand);
    std::vector<ZesCandRes> hcr(ncand);
    HIPCHK(hipMemcpy(hcand.data(), g.cand_sorted.p, ncand * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hcr.data(), g.cres.p, ncand * sizeof(ZesCandRes), hipMemcpyDeviceToHost));
    fprintf(stderr, "range: c=%llu lo=%llu own=%llu exact=%d nsurv=%u ncand=%u status=%u\n", (unsigned long long)c, (unsigned long long)lo_bit,
            (unsigned long long)own_bit, (int)exact, hc[0], ncand, hres[0].status);
    for (uint32_t k = 0; k < ncand && k < 12; k++)
      fprintf(stderr, "  cand[%u]=%u flags=%u out_len=%llu end_bit=%llu\n", k, hcand[k], hcr[k].flags, (unsigned long long)hcr[k].out_len,
              (unsigned long long)hcr[k].end_bit);
  }
  range_result(hres, rr);
  return ZES_OK;
}

// The same in two halves, for the host call that decodes a stream piece by piece while its neighbours are on the link
// (inflate_host_pipelined): range_begin enqueues everything piece k needs — no look at a result in between: the
// block decoder is launched over a bound and takes the candidate count from device memory (ZES_WORK_AUTO), the piece's
// place in the output is the block count of the pieces before it, kept on the device (k_inf_chain_range adds to it,
// k_inf_set_table_range reads it) — and range_finish waits for the read-backs of that piece only.  The host enqueues
// piece k + 1 before it waits for piece k: the device never waits for the host between pieces.
constexpr size_t RANGE_ACC_OFF = 64;  // g.counters: the pieces' block count so far, behind the counter words of a piece's search
static unsigned long long* range_acc() { return (unsigned long long*)((uint8_t*)g.counters.p + RANGE_ACC_OFF); }
// scratch for pieces of up to cmax bytes, before anything is in flight (growing a buffer frees the old one)
int range_reserve(uint64_t cmax) {
  int rc;
  if ((rc = range_pools(cmax, 128))) return rc;
  if ((rc = ensure(g.vlong, (size_t)std::min<uint64_t>(cmax / 256 + 4096, range_surv_cap(cmax)) * 24))) return rc;
  HIPCHK(hipMemsetAsync(range_acc(), 0, 8, g.stream));
  return ZES_OK;
}
int range_begin(int slot, RangePiece& pd, const uint8_t* d_in, uint64_t in_off, uint64_t c, uint64_t lo_bit, uint64_t own_bit, bool exact,
                uint8_t* d_out, uint64_t dcap, bool two, uint32_t flags) {
  int rc;
  ZesInfBuf b0, b1;
  pd = range_piece(in_off, c, lo_bit, own_bit, exact, &b0, &b1);
  if (!pd.skip && !pd.nothing) {
    // the most blocks the output can hold, and room for false candidates
    pd.bound = (uint32_t)std::min<uint64_t>(pd.cand_cap, dcap / ZES_BLK + 65);
    b1.cand_cap = pd.bound;
    b1.work_first = ZES_WORK_AUTO;
    const ZesInfBuf* dbufs = (const ZesInfBuf*)g.ibufs.p;
    uint32_t* counters = (uint32_t*)g.counters.p;
    uint32_t* cnt = counters + 4;
    hipLaunchKernelGGL(k_inf_set_table_range, dim3(1), dim3(64), 0, g.stream, b0, b1, (ZesInfBuf*)g.ibufs.p, counters, 6u,
                       (const unsigned long long*)range_acc(), (unsigned long long)dcap);
    if ((rc = launch_search(d_in, dbufs, 1u, pd.chunks, pd.surv_cap, counters, cnt, (uint8_t*)(cnt + 1), t1_search_mode(flags), c))) return rc;
    launch_block_par("k_inf_block_par", two, pd.bound, d_in, d_out, dbufs, 1u, cnt, nullptr, nullptr, ZesParMirror{});
    launch_chain_range(dbufs, cnt, range_acc());
    RangeSlot& hs = g.pinned->range[slot];
    HIPCHK(hipMemcpyAsync(hs.counters, g.counters.p, sizeof hs.counters, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipMemcpyAsync(hs.res, g.res.p, sizeof hs.res, hipMemcpyDeviceToHost, g.stream));
  }
  HIPCHK(hipEventRecord(g.ev_rng[slot], g.stream));
  return ZES_OK;
}
int range_finish(int slot, const RangePiece& pd, RangeRes* rr) {
  *rr = RangeRes();
  HIPCHK(hipEventSynchronize(g.ev_rng[slot]));
  if (pd.skip) return ZES_OK;
  if (pd.nothing) range_nothing(pd, rr);
  else if (range_found(pd, g.pinned->range[slot].counters, rr)) range_result(g.pinned->range[slot].res, rr);
  return ZES_OK;
}

// T2 for the buffers the block-parallel tier did not settle: segment-parallel decode of any valid stream
// (blocks of every type, 32 KiB history across blocks).  The candidate search runs buffer by buffer; the segment
// decode — nearly all of the time — and the window pass take all buffers of a group in one launch.  A buffer whose
// stream is not a clean chain of blocks keeps tier 0: the serial tiers then reproduce the reference's result.
#ifndef ZES_SEG_MIN_C
#define ZES_SEG_MIN_C 4096
#endif
constexpr uint64_t SEG_MIN_C = ZES_SEG_MIN_C;  // shorter streams go straight to the serial wavefront (round 3: 32768 -> 4096: 29 KB of zlib stream can be 4 MiB of periodic data — 12.5 ms by the serial wavefront, 2.8 ms here)
constexpr size_t SERIAL_BATCH_MIN_JOBS = 16;        // this many left-over streams of a call: one serial wavefront each, side by side
constexpr uint64_t SERIAL_BATCH_MAX_C = 8ull << 10;  // (round 3: 128 KiB -> 8 KiB)  // (longer ones go to the segment-parallel tier: its block decoder is ~15 times a lone wave)
constexpr uint64_t SEG_PIECES_MIN_C = 48ull << 20;  // streams from this size on go through the tier in pieces of 32 MiB (inflate_segments_pieces)
constexpr uint32_t SEG_GROUP_WORK = 8192;    // work items per segment launch (each owns a 64 KiB map)

// The device words of one group of nb buffers, as word offsets into g.counters: the search's scan/verify words and its
// candidate count per buffer; then what a segment run over nr <= nb of the buffers keeps (chain segments that are not in
// the symbol store, per buffer; failure flags, per buffer; the counter of matches behind the short marker ring); the
// first-byte sink of the search (a byte per buffer).
struct SegWords {
  size_t scan, cnt, novf, fail, far, sink, sink_words, total;  // (novf .. far: one piece, cleared before a run starts)
};
constexpr SegWords seg_words(size_t nb, size_t nr) {
  SegWords w{};
  w.scan = 0;
  w.cnt = 4;
  w.novf = w.cnt + nb;
  w.fail = w.novf + nr;
  w.far = w.fail + nr;
  w.sink = w.novf + 2 * nb + 4;
  w.sink_words = (nb + 3) / 4;
  w.total = w.sink + 4 + w.sink_words;
  return w;
}
constexpr bool seg_words_apart(size_t nb, size_t nr) {
  const SegWords w = seg_words(nb, nr);
  return disjoint({PinSpan{w.scan, 4}, PinSpan{w.cnt, nb}, PinSpan{w.novf, nr}, PinSpan{w.fail, nr}, PinSpan{w.far, 1}, PinSpan{w.sink, w.sink_words}}) && w.far + 1 <= w.sink &&
         w.sink + w.sink_words <= w.total && w.fail == w.novf + nr && w.far == w.fail + nr;
}
static_assert(seg_words_apart(SEG_GROUP_BUFS, SEG_GROUP_BUFS) && seg_words_apart(SEG_GROUP_BUFS, 1) && seg_words_apart(1, 1), "T2 device words overlap");
static_assert(seg_words(SEG_GROUP_BUFS, 1).total == 4 + SEG_GROUP_BUFS + 2 * SEG_GROUP_BUFS + 4 + 4 + (SEG_GROUP_BUFS + 3) / 4,
              "the group's counter scratch is not the size inflate_segments has always asked for");

// One segment run between the steps of inflate_segments_run: buffers ids[0..nb) with their sorted candidate lists at
// cand_sorted + cbase[k], ncand[k] entries.
struct T2Run {
  const uint8_t* d_in;
  uint8_t* d_out;
  InfJob* jobs;
  const uint32_t *ids, *cbase, *ncand;
  uint32_t nb;
  ZesSegJob* hj;   // page-locked: the job table, ...
  uint32_t* hs;    // ... [0, nb): not-in-store counts, later failure flags; [nb]: declined items, ...
  ZesRes* hres;    // ... the chains, then where they ended
  uint32_t *novf_d, *fail_d, *far_d;  // device words (SegWords)
  uint32_t work = 0, ratio = 0;       // work items; 16-bit symbols per compressed byte in the symbol store (0: no store)
  uint64_t share_syms = 0, bump_syms = 0;
  bool blockpar = false;              // the block decoder goes first
  uint32_t* fail_list = nullptr;      // what it declined: count, items
  std::vector<uint32_t> last_stuck;   // per buffer: the item its chain stood in front of when that item went to the wave decoder
  std::vector<uint32_t> novf;         // verdicts: hs and hres, copied out of the page-locked area before it is used again
  std::vector<ZesRes> hr;
  std::vector<char> go;               // the buffer's bytes are to be written
};
constexpr int T2_OVER = 1;  // a step's answer beside ZES_OK and an error: nothing more for this run
constexpr uint32_t T2_NONE = 0xFFFFFFFFu;

// step 1: the symbol store's size, the job table, the pools, table and cleared words on their way, the items' order
int t2_plan(T2Run& t) {
  int rc;
  const uint32_t nb = t.nb;
  ZesSegJob* hj = t.hj;
  uint64_t csum = 0;
  for (uint32_t k = 0; k < nb; k++) csum += t.jobs[t.ids[k]].c + 64;
  // symbol store: `ratio` 16-bit symbols per compressed byte (a segment that inflates further is decoded twice);
  // as many as a 2 GiB store holds, up to DEFLATE's own limit of 1032 bytes per compressed byte
  t.ratio = (uint32_t)std::min<uint64_t>(1032, (2ull << 30) / (2 * csum)) & ~1u;
  if (t.ratio < 4) t.ratio = 0;
  // behind the shares: a common area of a quarter of their size (at least 64 MiB), handed out by need to blocks whose
  // share is too small for them (a false candidate inside the block has cut it short, or the block inflates further)
  t.share_syms = (uint64_t)csum * t.ratio;
  t.bump_syms = t.ratio ? std::max<uint64_t>(t.share_syms / 4, 32ull << 20) & ~7ull : 0;
  if (t.ratio && ensure(g.sym16, (size_t)(t.share_syms + t.bump_syms) * 2 + 64)) t.ratio = 0;  // no memory for it: two decodes
  uint64_t sym_base = 0;
  for (uint32_t k = 0; k < nb; k++) {
    const InfJob& j = t.jobs[t.ids[k]];
    hj[k].in_off = j.in_off;
    hj[k].c = j.c;
    hj[k].sym_base = sym_base;
    hj[k].cand_base = t.cbase[k];
    hj[k].ncand = t.ncand[k];
    hj[k].work_first = t.work;
    hj[k].nseg = 0;
    hj[k].start0 = j.start0;
    hj[k].flags = j.partial ? ZES_SEG_PARTIAL : 0u;
    t.work += t.ncand[k] + 1;
    sym_base += (j.c + 64) * t.ratio / 2;
  }
  const uint32_t work = t.work;
  if ((rc = ensure(g.segjobs, sizeof(ZesSegJob) * nb))) return rc;
  if ((rc = ensure(g.sres, sizeof(ZesSegRes) * work))) return rc;
  if ((rc = ensure(g.maps, (size_t)work * ZES_WINDOW * 2))) return rc;
  if ((rc = ensure(g.seglist, (size_t)work * 4))) return rc;
  if ((rc = ensure(g.segprefix, (size_t)work * 8))) return rc;
  if ((rc = ensure(g.segorder, (size_t)work * 4))) return rc;
  if ((rc = ensure(g.symoff, (size_t)work * 8 + 8))) return rc;  // per work item: where its symbols are; behind them: the common area's fill
  if ((rc = ensure(g.res, sizeof(ZesRes) * nb * 2))) return rc;  // (second half: where a chain ended, k_inf_seg_chain)
  HIPCHK(hipMemcpyAsync(g.segjobs.p, hj, sizeof(ZesSegJob) * nb, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemsetAsync(t.novf_d, 0, (size_t)(t.far_d + 1 - t.novf_d) * 4, g.stream));  // (not-in-store counts, failure flags, far-match counter)
  hipLaunchKernelGGL(k_inf_seg_order, dim3(nb), dim3(1024), 0, g.stream, (const ZesSegJob*)g.segjobs.p, (const uint32_t*)g.cand_sorted.p,
                     (uint32_t*)g.segorder.p);
  return ZES_OK;
}

// ZES_T2_DBG: what work items first .. first + count have come to so far (numbered from 0)
int t2_dump_items(uint32_t first, uint32_t count) {
  std::vector<ZesSegRes> sr(count);
  HIPCHK(hipMemcpy(sr.data(), (const ZesSegRes*)g.sres.p + first, sr.size() * sizeof(ZesSegRes), hipMemcpyDeviceToHost));
  for (size_t w = 0; w < sr.size(); w++)
    fprintf(stderr, "   item %zu: end_bit %llu out_len %llu flags %u next %u\n", w, (unsigned long long)sr[w].end_bit,
            (unsigned long long)sr[w].out_len, sr[w].flags, sr[w].next);
  return ZES_OK;
}

// step 2: every work item first goes to the block decoder of the block-parallel tier in its any-encoder form
// (k_inf_seg_block_par: a workgroup per block, 1024 lanes decoding 1024 bit segments of it) — a wave that decodes a
// block token by token gets through ~13 MB/s.  What it declines (an item whose block is stored or fixed, is followed
// by a block that is not on the list, or is longer than 128 KiB) is listed, and the wave decoder runs for the list.
int t2_block_decoder(T2Run& t) {
  int rc;
  const uint32_t work = t.work;
  t.blockpar = t.ratio != 0 && !getenv("ZES_NO_SEG_PAR");
  if (t.blockpar) {
    if ((rc = ensure(g.segfail, ((size_t)work + 1) * 4))) return rc;
    t.fail_list = (uint32_t*)g.segfail.p;
    HIPCHK(hipMemsetAsync(t.fail_list, 0, 4, g.stream));
    HIPCHK(hipMemsetAsync((uint64_t*)g.symoff.p + work, 0, 8, g.stream));
    unsigned long long* pdbg = nullptr;
    if (getenv("ZES_DEBUG_PHASES")) {
      if ((rc = ensure(g.dbg, (size_t)work * ZES_PAR_DBG_ROW * 8))) return rc;
      HIPCHK(hipMemsetAsync(g.dbg.p, 0, (size_t)work * ZES_PAR_DBG_ROW * 8, g.stream));
      pdbg = (unsigned long long*)g.dbg.p;
    }
    {
      Timed tm("k_inf_seg_block_par");
      hipLaunchKernelGGL(k_inf_seg_block_par, dim3(work), dim3(PAR_THREADS), 0, g.stream, t.d_in, (const ZesSegJob*)g.segjobs.p, t.nb,
                         (const uint32_t*)g.cand_sorted.p, (ZesSegRes*)g.sres.p, (uint32_t*)g.maps.p, (uint32_t*)g.sym16.p, t.ratio, t.fail_list,
                         (unsigned long long*)((uint64_t*)g.symoff.p + work), (uint64_t)((t.share_syms / 2 + 3) & ~3ull), t.bump_syms,
                         (uint64_t*)g.symoff.p, pdbg);
    }
    if (pdbg) {
      HIPCHK(hipStreamSynchronize(g.stream));
      if ((rc = print_par_phases(pdbg, work))) return rc;
    }
  }
  if (getenv("ZES_T2_DBG")) {
    (void)hipStreamSynchronize(g.stream);
    std::vector<uint32_t> fl(work + 1, 0);
    if (t.fail_list) (void)hipMemcpy(fl.data(), t.fail_list, fl.size() * 4, hipMemcpyDeviceToHost);
    fprintf(stderr, "zes T2 items after the block decoder (fail list: %u:", fl[0]);
    for (uint32_t i = 0; i < fl[0] && i < 16; i++) fprintf(stderr, " %u", fl[1 + i]);
    fprintf(stderr, ")\n");
    (void)t2_dump_items(0, work);
  }
  return ZES_OK;
}

// the chain of every buffer of the run (work item 0 -> the item that starts where it ended -> ... -> the final block),
// read back with the not-in-store counts and the block decoder's declined count
int t2_chains(T2Run& t) {
  const uint32_t nb = t.nb;
  HIPCHK(hipMemsetAsync(t.novf_d, 0, (size_t)nb * 4, g.stream));
  {
    Timed tm("k_inf_seg_chain");  // (one launch: a workgroup per buffer of the group)
    hipLaunchKernelGGL(k_inf_seg_chain, dim3(nb), dim3(256), 0, g.stream, (const ZesSegJob*)g.segjobs.p, (const ZesSegRes*)g.sres.p,
                       (uint32_t*)g.seglist.p, (uint64_t*)g.segprefix.p, (ZesRes*)g.res.p, t.novf_d);
  }
  HIPCHK(hipMemcpyAsync(t.hs, t.novf_d, (size_t)nb * 4, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipMemcpyAsync(t.hres, g.res.p, sizeof(ZesRes) * nb * 2, hipMemcpyDeviceToHost, g.stream));
  if (t.blockpar) HIPCHK(hipMemcpyAsync(t.hs + nb, t.fail_list, 4, hipMemcpyDeviceToHost, g.stream));
  host_lap("(host work since)");
  HIPCHK(hipStreamSynchronize(g.stream));  // (the job table upload has completed too: hj may be rewritten)
  host_lap("T2: decode / chains");
  return ZES_OK;
}

// The wave decoder, a wave per work item: `items` of them from `list`, fewer if *count (device) says so.  It runs with the
// short marker ring (three waves per CU instead of two); a match that reaches behind the ring takes its symbols from the
// symbol store, so a segment that has outgrown its share of the store and then meets such a match cannot go on: far_d
// counts those, and the whole run goes through the full ring (rare: streams that inflate by more than the store's
// symbols per compressed byte).
void t2_launch_waves(const T2Run& t, bool short_ring, uint32_t items, const uint32_t* list, const uint32_t* count) {
  Timed tm("k_inf_seg_scan");
  hipLaunchKernelGGL(short_ring ? k_inf_seg_scan_short : k_inf_seg_scan, dim3(items), dim3(64), 0, g.stream, t.d_in, (const ZesSegJob*)g.segjobs.p,
                     t.nb, (const uint32_t*)g.cand_sorted.p, (ZesSegRes*)g.sres.p, (uint32_t*)g.maps.p, (uint32_t*)g.sym16.p, t.ratio, list, t.far_d,
                     count, (uint64_t*)g.symoff.p);
}

// The undecoded item buffer k's chain stands in front of (status 1: no chain; 3: the chain of a piece, as far as it got)
// and has not stood in front of before; T2_NONE: none, or the same item again (it has been to the wave decoder — the
// stream is not for this tier), or a piece of a longer stream whose chain got through half the piece: what that stands
// in front of is, as a rule, the block the piece's end cuts — the next piece starts there.
uint32_t t2_stuck_at(const T2Run& t, uint32_t k) {
  const ZesRes &chain = t.hres[k], &end = t.hres[t.nb + k];
  uint32_t w = T2_NONE;
  if (chain.status == 1 && chain.out_len != 0) w = (uint32_t)(chain.out_len - 1);
  else if (chain.status == 3 && end.aux != 0) w = end.aux - 1u;
  if (w == T2_NONE || w == t.last_stuck[k]) return T2_NONE;
  if (chain.status == 3 && end.out_len >= t.jobs[t.ids[k]].c * 4) return T2_NONE;
  return w;
}

// step 3 behind the block decoder.  The chains are tried on what it left BEFORE the wave decoder gets the declined items:
// an item that starts on a false candidate is declined (its "block" is garbage) and nobody's chain leads to it — but
// the lone wave that decodes it on may take milliseconds to find that out (256 x 1 MiB of zlib text: 6.9 of 32 ms).
// Chains that stand in front of an undecoded item (a stored or fixed block, a block behind an unlisted start): exactly
// those items go to the wave decoder (a zlib stream's last block is often a fixed one: one small item per stream, where
// the declined list of 256 streams of 1 MiB also held ~200 false candidates that cost the lone waves 6.8 ms), and the
// chains are followed again; a few rounds.  *everything: the wave decoder is to take all that was declined — a far
// match behind the short ring, or the rounds are used up (or were not tried) with a chain still in front of an
// undecoded item: streams with many stored or fixed blocks, or whose blocks mostly follow blocks that are not on the
// thinned list.
int t2_handover(T2Run& t, bool* everything) {
  int rc;
  const uint32_t nb = t.nb;
  *everything = false;
  if ((rc = t2_chains(t))) return rc;
  const uint32_t ndecl = t.hs[nb];
  if (getenv("ZES_DEBUG")) fprintf(stderr, "zes T2: %u work items, %u declined by the block decoder\n", t.work, ndecl);
  if (!ndecl) return ZES_OK;
  t.last_stuck.assign(nb, T2_NONE);
  // (No rounds when an eighth of all items were declined: a stream of blocks of a few hundred bytes — zlib with memLevel 1 —
  // is thinned to 2048 items of a dozen blocks each, every one of them handed over behind its first block: four
  // rounds of one lone wave each were 16 of that stream's 31 ms before the launch that takes them all.)
  const bool many = ndecl >= 16 && (uint64_t)ndecl * 8 >= t.work;
  for (int round = 0; !many && round < 4; round++) {
    uint32_t* hl = g.pinned->t2.live;
    uint32_t n = 0;
    for (uint32_t k = 0; k < nb; k++) {
      const uint32_t w = t2_stuck_at(t, k);
      if (w == T2_NONE) continue;
      t.last_stuck[k] = w;
      hl[++n] = t.hj[k].work_first + w;
    }
    if (!n) break;
    hl[0] = n;
    if ((rc = ensure(g.seglive, ((size_t)nb + 1) * 4))) return rc;
    HIPCHK(hipMemcpyAsync(g.seglive.p, hl, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, g.stream));
    t2_launch_waves(t, true, n, (const uint32_t*)g.seglive.p + 1, (const uint32_t*)g.seglive.p);
    HIPCHK(hipMemcpyAsync(&g.pinned->t2.far, t.far_d, 4, hipMemcpyDeviceToHost, g.stream));
    if ((rc = t2_chains(t))) return rc;
    if (g.pinned->t2.far != 0) {  // a far match behind the short ring: the full-ring pass decides
      *everything = true;
      return ZES_OK;
    }
  }
  for (uint32_t k = 0; k < nb; k++)
    if (t2_stuck_at(t, k) != T2_NONE) *everything = true;
  return ZES_OK;
}

// step 3 without the block decoder, or when the handover has not settled the run: everything that was declined (no
// block decoder: every item, in k_inf_seg_order's order) goes to the wave decoder in one launch, after a far match
// every item again with the full ring, and the chains are followed again
int t2_everything(T2Run& t) {
  t2_launch_waves(t, true, t.work, t.blockpar ? (const uint32_t*)t.fail_list + 1 : (const uint32_t*)g.segorder.p, t.fail_list);
  HIPCHK(hipMemcpyAsync(&g.pinned->t2.far, t.far_d, 4, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  if (g.pinned->t2.far != 0) t2_launch_waves(t, false, t.work, (const uint32_t*)g.segorder.p, nullptr);
  return t2_chains(t);
}

// step 4: every buffer's verdict.  A chain to the final block (a piece: as far as it got) that fits the output: go; one
// that does not fit: the caller learns the size without the output passes; anything else is left to the serial tiers.
int t2_verdicts(T2Run& t) {
  const uint32_t nb = t.nb;
  t.novf.assign(t.hs, t.hs + nb);  // (the page-locked area is used again by the output passes)
  t.hr.assign(t.hres, t.hres + 2 * nb);
  t.go.assign(nb, 0);
  int rc;
  bool any = false;
  for (uint32_t k = 0; k < nb; k++) {
    InfJob& j = t.jobs[t.ids[k]];
    ZesRes& r = t.hr[k];
    if (getenv("ZES_DEBUG"))
      fprintf(stderr, "zes T2: c=%llu candidates=%u chain status=%d segments=%u (%u decoded twice) out_len=%llu\n", (unsigned long long)j.c,
              t.ncand[k], r.status, r.aux, t.novf[k], (unsigned long long)r.out_len);
    if (getenv("ZES_T2_DBG") && (rc = t2_dump_items(t.hj[k].work_first, t.ncand[k] + 1))) return rc;  // what every work item came to
    if (r.status == 3 && j.partial) r.status = 0;  // a piece's chain, as far as it got
    if (r.status != 0 || r.aux == 0) continue;
    j.end_bit = t.hr[nb + k].out_len;
    j.final_seen = t.hr[nb + k].status != 0;
    if (r.out_len > j.cap) {
      j.tier = 2;
      j.out_len = r.out_len;
      j.status = ZES_E_NOSPACE;
      continue;
    }
    t.go[k] = 1;
    any = true;
    t.hj[k].nseg = r.aux;
  }
  return any ? ZES_OK : T2_OVER;
}

// step 5: the output passes — the 32 KiB window in front of every segment, the symbols translated into bytes, and the
// segments that are not in the symbol store decoded again, buffer by buffer
int t2_output(T2Run& t) {
  int rc;
  const uint32_t nb = t.nb, work = t.work;
  ZesSegJob* hj = t.hj;
  const uint32_t* cs = (const uint32_t*)g.cand_sorted.p;
  if ((rc = ensure(g.wins, (size_t)work * ZES_WINDOW))) return rc;
  HIPCHK(hipMemcpyAsync(g.segjobs.p, hj, sizeof(ZesSegJob) * nb, hipMemcpyHostToDevice, g.stream));
  // where every buffer's bytes go (and how much output exists in front: a later piece of a long stream)
  if ((rc = ensure(g.segouts, sizeof(ZesSegOut) * nb))) return rc;
  ZesSegOut* ho = g.pinned->t2.out;
  uint32_t max_tr = 0, min_tr = 0xFFFFFFFFu;
  for (uint32_t k = 0; k < nb; k++) {
    const InfJob& j = t.jobs[t.ids[k]];
    ho[k].out_off = j.out_off;
    ho[k].cap = j.cap;
    ho[k].nseg = (t.go[k] && t.novf[k] < t.hr[k].aux) ? t.hr[k].aux : 0u;
    ho[k].hist = j.hist;
    if (ho[k].nseg) {
      max_tr = std::max(max_tr, ho[k].nseg);
      min_tr = std::min(min_tr, ho[k].nseg);
    }
  }
  HIPCHK(hipMemcpyAsync(g.segouts.p, ho, sizeof(ZesSegOut) * nb, hipMemcpyHostToDevice, g.stream));
  {
    // windows: groups of maps composed in parallel, the groups chained, every window finished in parallel
    uint32_t max_nseg = 0;
    for (uint32_t k = 0; k < nb; k++) max_nseg = std::max(max_nseg, hj[k].nseg);
    const uint32_t max_groups = (max_nseg + SEGWIN_GROUP - 1) / SEGWIN_GROUP;
    if ((rc = ensure(g.pw16, (size_t)work * ZES_WINDOW * 2))) return rc;
    if ((rc = ensure(g.gwins, ((size_t)work / SEGWIN_GROUP + nb + 1) * ZES_WINDOW))) return rc;  // (work_first / group) + buffer index + group
    Timed tm("k_inf_seg_windows");
    hipLaunchKernelGGL(k_inf_seg_win_group, dim3(max_groups, nb), dim3(1024), 0, g.stream, (const uint32_t*)g.maps.p,
                       (const uint32_t*)g.seglist.p, (const ZesSegJob*)g.segjobs.p, (uint32_t*)g.pw16.p);
    hipLaunchKernelGGL(k_inf_seg_win_top, dim3(nb), dim3(1024), 0, g.stream, (const uint32_t*)g.pw16.p, (const ZesSegJob*)g.segjobs.p,
                       (uint8_t*)g.gwins.p, (const uint8_t*)t.d_out, (const ZesSegOut*)g.segouts.p);
    hipLaunchKernelGGL(k_inf_seg_win_fin, dim3(max_nseg, nb), dim3(1024), 0, g.stream, (const uint32_t*)g.pw16.p,
                       (const ZesSegJob*)g.segjobs.p, (const uint8_t*)g.gwins.p, (uint8_t*)g.wins.p);
  }
  if (max_tr) {
    // symbols -> bytes: one launch over (segments, workgroups per segment, buffers)
    Timed tm("k_inf_seg_translate");
    // few long segments: split each over several workgroups (by the buffer with the fewest)
    const uint32_t ny = std::max(1u, std::min(16u, 2048u / std::max(1u, min_tr * std::min(nb, 8u))));
    hipLaunchKernelGGL(k_inf_seg_translate, dim3(max_tr, ny, nb), dim3(256), 0, g.stream, t.d_out, (const ZesSegJob*)g.segjobs.p,
                       (const ZesSegOut*)g.segouts.p, cs, (const ZesSegRes*)g.sres.p, (const uint32_t*)g.seglist.p,
                       (const uint64_t*)g.segprefix.p, (const uint8_t*)g.wins.p, (const uint32_t*)g.sym16.p, (const uint64_t*)g.symoff.p, t.fail_d);
  }
  for (uint32_t k = 0; k < nb; k++) {
    if (!t.go[k] || t.novf[k] == 0) continue;
    const InfJob& j = t.jobs[t.ids[k]];
    const uint32_t nseg = t.hr[k].aux, wf = hj[k].work_first;
    Timed tm("k_inf_seg_decode");
    hipLaunchKernelGGL(k_inf_seg_decode, dim3(nseg), dim3(64), 0, g.stream, t.d_in, j.in_off, j.c, t.d_out, j.out_off, j.cap, cs + t.cbase[k],
                       (const ZesSegRes*)g.sres.p + wf, (const uint32_t*)g.seglist.p + wf, (const uint64_t*)g.segprefix.p + wf,
                       (const uint8_t*)g.wins.p + (size_t)wf * ZES_WINDOW, t.fail_d + k, t.novf[k] < nseg ? 1u : 0u, j.start0, j.hist);
  }
  HIPCHK(hipMemcpyAsync(t.hs, t.fail_d, (size_t)nb * 4, hipMemcpyDeviceToHost, g.stream));
  host_lap("(host work since)");
  HIPCHK(hipStreamSynchronize(g.stream));
  host_lap("T2: windows + translate");
  return ZES_OK;
}

// step 6: the jobs this run has settled
int t2_publish(T2Run& t) {
  for (uint32_t k = 0; k < t.nb; k++) {
    if (!t.go[k] || t.hs[k] != 0) continue;  // (a match behind the first byte of the stream: the serial tiers decide)
    InfJob& j = t.jobs[t.ids[k]];
    j.tier = 2;
    j.out_len = t.hr[k].out_len;
    j.status = ZES_OK;
  }
  return ZES_OK;
}

// `w`: the run's device words (seg_words(buffers of the group, nb))
int inflate_segments_run(const uint8_t* d_in, uint8_t* d_out, InfJob* jobs, const uint32_t* ids, const uint32_t* cbase, const uint32_t* ncand,
                         uint32_t nb, const SegWords& w) {
  int rc;
  uint32_t* words = (uint32_t*)g.counters.p;
  T2Run t{d_in, d_out, jobs, ids, cbase, ncand, nb, g.pinned->t2.jobs, g.pinned->t2.flags, g.pinned->t2.res, words + w.novf, words + w.fail, words + w.far};
  if ((rc = t2_plan(t))) return rc;
  if ((rc = t2_block_decoder(t))) return rc;
  bool everything = true;  // (no block decoder: the wave decoder takes every item)
  if (t.blockpar && (rc = t2_handover(t, &everything))) return rc;
  if (everything && (rc = t2_everything(t))) return rc;
  if ((rc = t2_verdicts(t))) return rc == T2_OVER ? ZES_OK : rc;
  if ((rc = t2_output(t))) return rc;
  return t2_publish(t);
}

// One group of the tier between the steps of inflate_segments: buffers ids[0..nb), their candidate lists side by side in
// g.cand / g.cand_sorted (buffer k's at cbase[k], room for ccap[k]).
struct T2Group {
  const uint8_t* d_in;
  uint8_t* d_out;
  InfJob* jobs;
  const uint32_t* ids;
  uint32_t nb;
  SegWords w;
  std::vector<uint32_t> cbase, ccap;
  uint32_t surv_cap = 0;  // of a buffer searched by itself
  uint32_t *counters = nullptr, *cnt = nullptr;
  uint8_t* sink = nullptr;
  const ZesInfBuf* dbufs = nullptr;  // the table of the search that is running
  std::vector<char> searched;        // the several-buffer search has settled this buffer's list
  std::vector<uint32_t> nc;          // candidates per buffer, read back
};

// step 1: where every buffer's candidates go, the pools, the cleared device words.
// (range_cand_cap / range_surv_cap are c / 64 + 64 and c / 4 + 1024 below their upper bounds of 2^23 and 2^30: so for
// every c this tier is given — streams below SEG_PIECES_MIN_C, pieces of up to 448 MiB: 448 MiB / 64 + 64 < 2^23.)
int t2_group_table(T2Group& G) {
  int rc;
  const uint32_t nb = G.nb;
  G.cbase.resize(nb);
  G.ccap.resize(nb);
  G.searched.assign(nb, 0);
  uint64_t cands = 0, max_c = 0;
  for (uint32_t k = 0; k < nb; k++) {
    const InfJob& j = G.jobs[G.ids[k]];
    G.cbase[k] = (uint32_t)cands;
    G.ccap[k] = range_cand_cap(j.c);
    cands += G.ccap[k];
    max_c = std::max(max_c, j.c);
  }
  G.surv_cap = range_surv_cap(max_c);
  G.w = seg_words(nb, nb);
  if ((rc = ensure(g.ibufs, sizeof(ZesInfBuf) * 2))) return rc;
  if ((rc = ensure(g.surv, (size_t)G.surv_cap * 8))) return rc;
  if ((rc = ensure(g.cand, (size_t)cands * 4))) return rc;
  if ((rc = ensure(g.cand_sorted, (size_t)cands * 4))) return rc;
  if ((rc = ensure(g.counters, G.w.total * 4))) return rc;
  if ((rc = ensure(g.mvlist, SEG_BUCKETS * 4))) return rc;
  G.counters = (uint32_t*)g.counters.p + G.w.scan;
  G.cnt = (uint32_t*)g.counters.p + G.w.cnt;
  G.sink = (uint8_t*)((uint32_t*)g.counters.p + G.w.sink);
  HIPCHK(hipMemsetAsync(g.counters.p, 0, G.w.total * 4, g.stream));
  G.dbufs = (const ZesInfBuf*)g.ibufs.p;
  return ZES_OK;
}

// a buffer's entry of a search table of this tier
ZesInfBuf t2_search_buf(const T2Group& G, uint32_t k) {
  const InfJob& j = G.jobs[G.ids[k]];
  ZesInfBuf b = inf_buf(j);
  b.cand_base = G.cbase[k];
  b.cand_cap = G.ccap[k];
  b.start_rel = j.start0 - 16u;  // (a piece of a longer stream: nothing in front of its first block is searched)
  return b;
}

// step 2, several buffers (a batch of another encoder's streams): one scan and one header test over all of them, the lists
// sorted by one launch; only a buffer with more candidates than a segment run takes (tiny blocks) is thinned, by
// itself, afterwards.  (256 streams of 1 MiB: the searches one after the other were 36 ms of launches.)
int t2_search_group(T2Group& G) {
  int rc;
  const uint32_t nb = G.nb;
  ZesInfBuf* hb = g.pinned->t2.search;
  uint64_t chunks = 0, total_c = 0;
  for (uint32_t k = 0; k < nb; k++) {
    hb[k] = t2_search_buf(G, k);
    hb[k].first_chunk = (uint32_t)chunks;
    chunks += (hb[k].c + INF_SCAN_BYTES - 1) / INF_SCAN_BYTES;
    total_c += hb[k].c;
  }
  memset(&hb[nb], 0, sizeof(ZesInfBuf));
  hb[nb].first_chunk = (uint32_t)chunks;
  const uint32_t surv_all = (uint32_t)std::min<uint64_t>(total_c / 4 + 1024ull * nb, 1ull << 30);
  if ((rc = ensure(g.ibufs, sizeof(ZesInfBuf) * (nb + 1)))) return rc;
  if ((rc = ensure(g.surv, (size_t)surv_all * 8))) return rc;
  G.dbufs = (const ZesInfBuf*)g.ibufs.p;
  HIPCHK(hipMemcpyAsync(g.ibufs.p, hb, sizeof(ZesInfBuf) * (nb + 1), hipMemcpyHostToDevice, g.stream));
  if ((rc = launch_search(G.d_in, G.dbufs, nb, (uint32_t)chunks, surv_all, G.counters, G.cnt, G.sink, T2_SEARCH, total_c))) return rc;
  {
    Timed t("k_inf_ranksort");
    hipLaunchKernelGGL(k_inf_ranksort, dim3(nb), dim3(1024), 0, g.stream, G.dbufs, (const uint32_t*)G.cnt, (const uint32_t*)g.cand.p,
                       (uint32_t*)g.cand_sorted.p, SEG_BUCKETS);
  }
  uint32_t* hc0 = g.pinned->t2.ncand;
  HIPCHK(hipMemcpyAsync(hc0, G.cnt, (size_t)nb * 4, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  bool redo = false;
  for (uint32_t k = 0; k < nb; k++) {
    G.searched[k] = hc0[k] <= SEG_BUCKETS;  // (the others: thinned, from a search of their own)
    redo = redo || !G.searched[k];
  }
  if (redo) {  // a table of its own for those searches: the one the sort used stays as it is
    if ((rc = ensure(g.ibufs2, sizeof(ZesInfBuf) * 2))) return rc;
    G.dbufs = (const ZesInfBuf*)g.ibufs2.p;
  }
  return ZES_OK;
}

// step 2, one buffer by itself (the search has the chip to itself), and its list thinned
int t2_search_one(T2Group& G, uint32_t k) {
  int rc;
  uint32_t* cntk = G.cnt + k;
  HIPCHK(hipMemsetAsync(cntk, 0, 4, g.stream));
  const ZesInfBuf b0 = t2_search_buf(G, k);
  const uint32_t chunks = (uint32_t)((b0.c + INF_SCAN_BYTES - 1) / INF_SCAN_BYTES);
  ZesInfBuf b1;
  memset(&b1, 0, sizeof b1);
  b1.first_chunk = chunks;
  hipLaunchKernelGGL(k_inf_set_table1, dim3(1), dim3(64), 0, g.stream, b0, b1, const_cast<ZesInfBuf*>(G.dbufs), G.counters, 4u);
  // The block-parallel tier has just searched this very stream and declined it (another encoder's): its scan's
  // survivors are still in g.surv — the scan applies the same tests for both tiers, the reference's own rules are the
  // verify kernels' — so only their count goes back into place (0.06 of the 1.65 ms of 64 MiB of zlib text).
  const bool reuse = G.nb == 1 && g.sv.holds(g.surv, G.d_in, b0.in_off, b0.c) && b0.start_rel == 0u && g.sv.n <= G.surv_cap;
  g.sv.drop();
  if (reuse) {  // the header test alone
    g.pinned->t2.nsurv = g.sv.n;
    HIPCHK(hipMemcpyAsync(G.counters, &g.pinned->t2.nsurv, 4, hipMemcpyHostToDevice, g.stream));
    rc = launch_verify(G.d_in, G.dbufs, G.surv_cap, G.counters, cntk, T2_SEARCH.loose, b0.c);
  } else {
    rc = launch_search(G.d_in, G.dbufs, 1u, chunks, G.surv_cap, G.counters, cntk, G.sink, T2_SEARCH, b0.c);
  }
  if (rc) return rc;
  // one candidate per bucket of the stream, in order (at most SEG_BUCKETS segments whatever the block size)
  Timed t("k_inf_cand_thin");
  const uint32_t bucket_bits = (uint32_t)((b0.c * 8 + SEG_BUCKETS - 1) / SEG_BUCKETS);
  HIPCHK(hipMemsetAsync(g.mvlist.p, 0xFF, SEG_BUCKETS * 4, g.stream));
  hipLaunchKernelGGL(k_inf_cand_bucket, dim3((uint32_t)std::min<uint64_t>(b0.cand_cap / 256 + 1, 1024)), dim3(256), 0, g.stream,
                     (const uint32_t*)g.cand.p + b0.cand_base, (const uint32_t*)cntk, b0.cand_cap, bucket_bits, (uint32_t*)g.mvlist.p);
  hipLaunchKernelGGL(k_inf_cand_compact, dim3(1), dim3(1024), 0, g.stream, (const uint32_t*)g.mvlist.p,
                     (uint32_t*)g.cand_sorted.p + b0.cand_base, cntk);
  return ZES_OK;
}

// step 3: the candidate counts, back on the host
int t2_group_counts(T2Group& G) {
  const uint32_t nb = G.nb;
  uint32_t* hc = g.pinned->t2.ncand;
  HIPCHK(hipMemcpyAsync(hc, G.cnt, (size_t)nb * 4, hipMemcpyDeviceToHost, g.stream));
  host_lap("(host work since)");
  HIPCHK(hipStreamSynchronize(g.stream));
  host_lap("T2: search (verify, thinning)");
  G.nc.assign(hc, hc + nb);
  if (getenv("ZES_T2_DBG")) {  // the candidate lists, for a comparison with a map of the stream (tools/gpu_t2_candidates.py)
    for (uint32_t k = 0; k < nb; k++) {
      std::vector<uint32_t> hcand(std::min<uint32_t>(G.nc[k], SEG_BUCKETS));
      if (!hcand.empty()) HIPCHK(hipMemcpy(hcand.data(), (const uint32_t*)g.cand_sorted.p + G.cbase[k], hcand.size() * 4, hipMemcpyDeviceToHost));
      fprintf(stderr, "zes T2 candidates buf %u (%zu):", k, hcand.size());
      for (uint32_t v : hcand) fprintf(stderr, " %u", v + 16u);
      fprintf(stderr, "\n");
    }
  }
  return ZES_OK;
}

// step 4: segment runs, as many buffers as fit the work-item budget at a time
int t2_group_runs(T2Group& G) {
  int rc;
  std::vector<uint32_t> rid, rbase, rn;
  for (uint32_t k = 0; k < G.nb;) {
    uint32_t work = 0;
    rid.clear();
    rbase.clear();
    rn.clear();
    for (; k < G.nb; k++) {
      if (G.nc[k] > SEG_BUCKETS) continue;  // (a poisoned count; a stream without a second block start is still one block for the block decoder)
      if (!rid.empty() && work + G.nc[k] + 1 > SEG_GROUP_WORK) break;
      rid.push_back(G.ids[k]);
      rbase.push_back(G.cbase[k]);
      rn.push_back(G.nc[k]);
      work += G.nc[k] + 1;
    }
    const uint32_t nr = (uint32_t)rid.size();
    if (nr && (rc = inflate_segments_run(G.d_in, G.d_out, G.jobs, rid.data(), rbase.data(), rn.data(), nr, seg_words(G.nb, nr)))) return rc;
  }
  return ZES_OK;
}

int inflate_segments(const uint8_t* d_in, uint8_t* d_out, InfJob* jobs, const std::vector<uint32_t>& all) {
  int rc;
  for (size_t g0 = 0; g0 < all.size(); g0 += SEG_GROUP_BUFS) {
    T2Group G{d_in, d_out, jobs, all.data() + g0, (uint32_t)std::min<size_t>(SEG_GROUP_BUFS, all.size() - g0)};
    if ((rc = t2_group_table(G))) return rc;
    if (G.nb > 1 && (rc = t2_search_group(G))) return rc;
    for (uint32_t k = 0; k < G.nb; k++)
      if (!G.searched[k] && (rc = t2_search_one(G, k))) return rc;
    if ((rc = t2_group_counts(G))) return rc;
    if ((rc = t2_group_runs(G))) return rc;
  }
  return ZES_OK;
}

// A stream of stored blocks only (tier 2 as well: parallel, any encoder).  Leaves j.tier at 0 if it is anything else.
constexpr uint64_t STORED_MIN_C = 65536;  // below this the serial wavefront is as quick
// A stream too long for this tier's 32-bit bit positions (512 MiB of compressed data and more) goes through it piece by
// piece: a piece starts at the block behind the last one decoded (work item 0 at that bit, the candidate search from
// there), its chain is accepted as far as the piece holds whole blocks, and the 32 KiB in front of its first segment
// are the output so far.  (src/inflate.ts:16-40 has no size limit; reference-made streams of this size take
// inflate_pieces, the block-parallel tier's form of the same.)  ZES_SEG_PIECE_MB: piece size, for tests.
int inflate_segments_pieces(const uint8_t* d_in, uint8_t* d_out, InfJob& j) {
  static const uint64_t piece = [] {
    const char* e = getenv("ZES_SEG_PIECE_MB");
    const uint64_t mb = e ? strtoull(e, nullptr, 10) : 0;
    return mb ? (mb << 20) : (32ull << 20);  // (a piece of 32 MiB has about as many blocks as the tier takes work items: no thinning)
  }();
  int rc;
  uint64_t pos_bit = 16, out_base = 0;
  uint64_t piece_now = piece;  // (grows when a piece does not hold its first block whole: an encoder with very long blocks)
  bool nospace = false;  // the caller's room ran out: the pieces behind are only measured (the chain's lengths need no output)
  for (int guard = 0; guard < (1 << 20); guard++) {
    // the piece: from a 16-byte boundary at least two bytes in front of the block (work item 0 starts at bit >= 16 of it).
    // Not t1_piece_origin's rule, which always steps one boundary back: here it is the nearest boundary that leaves the
    // two bytes.  Both keep the block at bit >= 16; they give different bit positions inside the piece (start0 here, the
    // range's lo_bit there), which the kernels see, so each tier keeps its own.
    const uint64_t pb = pos_bit >> 3;
    const uint64_t byte0 = pb >= 2 ? ((pb - 2) & ~15ull) : 0;
    std::vector<InfJob> sub(1);
    const uint64_t room = (nospace || j.cap <= out_base) ? 0 : j.cap - out_base;
    sub[0] = InfJob{j.in_off + byte0, std::min<uint64_t>(j.c - byte0, piece_now), j.out_off + std::min(out_base, j.cap), room, 0, ZES_OK, 0};
    sub[0].start0 = (uint32_t)(pos_bit - 8 * byte0);
    sub[0].hist = nospace ? 0u : (uint32_t)std::min<uint64_t>(out_base, ZES_WINDOW);
    sub[0].partial = byte0 + sub[0].c < j.c;  // (the last piece must end with the stream's final block)
    const std::vector<uint32_t> one(1, 0u);
    if ((rc = inflate_segments(d_in, d_out, sub.data(), one))) return rc;
    const bool stuck = sub[0].tier != 2 || (sub[0].status == ZES_OK && !sub[0].final_seen && 8 * byte0 + sub[0].end_bit <= pos_bit);
    if (stuck && sub[0].partial && piece_now < (448ull << 20)) {  // no whole block in this piece: a longer one, same start
      piece_now = std::min<uint64_t>(piece_now * 4, 448ull << 20);
      continue;
    }
    if (sub[0].tier != 2) return ZES_OK;  // not this way: the serial tiers decide
    piece_now = piece;
    if (sub[0].status == ZES_E_NOSPACE) nospace = true;
    else if (sub[0].status != ZES_OK) return ZES_OK;
    out_base += sub[0].out_len;
    if (sub[0].final_seen) {
      j.tier = 2;
      j.status = (nospace || out_base > j.cap) ? ZES_E_NOSPACE : ZES_OK;
      j.out_len = out_base;
      j.end_bit = 8 * byte0 + sub[0].end_bit;
      return ZES_OK;
    }
    const uint64_t next_bit = 8 * byte0 + sub[0].end_bit;
    if (!sub[0].partial || next_bit <= pos_bit) return ZES_OK;  // no final block where the data ends, or no progress
    pos_bit = next_bit;
  }
  return ZES_OK;
}

int inflate_stored(const uint8_t* d_in, uint8_t* d_out, InfJob& j) {
  int rc;
  const uint64_t cap_entries = std::min<uint64_t>(j.c / 5 + 1, 1ull << 22);
  if ((rc = ensure(g.res, sizeof(ZesRes)))) return rc;
  if ((rc = ensure(g.scratch, (size_t)cap_entries * sizeof(ZesStoredBlk)))) return rc;
  ZesRes hr;
  hr.status = 1;
  // up to 128 MiB: every byte position tested for a stored block's header, the chain from the first one marked by
  // pointer doubling (k_inf_stored_find / k_inf_stored_rank); what that cannot settle, and longer streams: the walk
  constexpr uint64_t STORED_PAR_MAX_C = 128ull << 20;
  constexpr uint32_t STORED_CHUNK_H = 16384, STORED_SLOTS_H = 8;
  if (j.c >= (2ull << 20) && j.c <= STORED_PAR_MAX_C && !getenv("ZES_NO_STORED_PAR")) {  // (a short stream's walk is quicker than two launches)
    const uint32_t nchunks = (uint32_t)((j.c + STORED_CHUNK_H - 1) / STORED_CHUNK_H);
    if ((rc = ensure(g.mvlist, (size_t)nchunks * (STORED_SLOTS_H + 1) * 4))) return rc;
    uint32_t* slots = (uint32_t*)g.mvlist.p;
    uint32_t* counts = slots + (size_t)nchunks * STORED_SLOTS_H;
    {
      Timed t("k_inf_stored_find");
      hipLaunchKernelGGL(k_inf_stored_find, dim3(nchunks), dim3(256), 0, g.stream, d_in, j.in_off, (uint32_t)j.c, slots, counts);
    }
    {
      Timed t("k_inf_stored_rank");
      hipLaunchKernelGGL(k_inf_stored_rank, dim3(1), dim3(1024), 0, g.stream, d_in, j.in_off, (uint32_t)j.c, (const uint32_t*)slots,
                         (const uint32_t*)counts, nchunks, cap_entries, (ZesStoredBlk*)g.scratch.p, (ZesRes*)g.res.p);
    }
    if ((rc = read_res(&hr))) return rc;
  }
  if (hr.status != 0) {
    Timed t("k_inf_stored_walk");
    hipLaunchKernelGGL(k_inf_stored_walk, dim3(1), dim3(64), 0, g.stream, d_in, j.in_off, j.c, cap_entries, (ZesStoredBlk*)g.scratch.p,
                       (ZesRes*)g.res.p);
    if ((rc = read_res(&hr))) return rc;
  }
  if (hr.status != 0) return ZES_OK;
  j.tier = 2;
  j.out_len = hr.out_len;
  j.status = hr.out_len > j.cap ? ZES_E_NOSPACE : ZES_OK;
  if (j.want_end && hr.aux) {  // behind the last stored block's last byte
    ZesStoredBlk last;
    HIPCHK(hipMemcpy(&last, (const ZesStoredBlk*)g.scratch.p + hr.aux - 1, sizeof last, hipMemcpyDeviceToHost));
    j.end_bit = 8 * (last.src + last.len);
  }
  if (j.status == ZES_OK && hr.aux) {
    Timed t("k_inf_stored_copy");
    hipLaunchKernelGGL(k_inf_stored_copy, dim3(hr.aux), dim3(256), 0, g.stream, d_in, j.in_off, d_out, j.out_off, (const ZesStoredBlk*)g.scratch.p);
    HIPCHK(hipStreamSynchronize(g.stream));
  }
  return ZES_OK;
}

// T3 then T4 for one buffer the parallel tiers did not settle.
int inflate_slow(const uint8_t* d_in, uint8_t* d_out, InfJob& j) {
  int rc;
  if ((rc = ensure(g.res, 2 * sizeof(ZesRes)))) return rc;  // (k_inf_exact: [1].out_len = where its reader stopped)
  if ((rc = ensure(g.resume, 16))) return rc;
  ZesRes hr;
  bool have_resume = false;
  // T3: one wavefront, any valid stream
  if (j.c >= 3) {
#ifdef WD_PROFILE
    if ((rc = ensure(g.dbg, 64))) return rc;
    HIPCHK(hipMemsetAsync(g.dbg.p, 0, 64, g.stream));
    zes_wd_set_dbg((unsigned long long*)g.dbg.p);
#endif
    {
      const ZesInfBuf b0 = inf_buf(j);
      if ((rc = ensure(g.ibufs, sizeof(ZesInfBuf) * 2))) return rc;
      hipLaunchKernelGGL(k_inf_set_table1, dim3(1), dim3(64), 0, g.stream, b0, b0, (ZesInfBuf*)g.ibufs.p, (uint32_t*)nullptr, 0u);
      Timed t("k_inf_decode_seq");
      hipLaunchKernelGGL(k_inf_decode, dim3(1), dim3(64), 0, g.stream, d_in, d_out, (const ZesInfBuf*)g.ibufs.p, (ZesRes*)g.res.p,
                         (uint64_t*)g.resume.p);
    }
    if ((rc = read_res(&hr))) return rc;
#ifdef WD_PROFILE
    {
      unsigned long long h[8];
      HIPCHK(hipMemcpy(h, g.dbg.p, 64, hipMemcpyDeviceToHost));
      const double n = (double)std::max<unsigned long long>(h[5], 1);
      fprintf(stderr, "zes wave decoder: %llu tokens, cycles per token: lit/len entry %.1f, literal path %.1f, distance entry %.1f, copy %.1f, flush test %.1f; kernel %.1f\n",
              h[5], h[0] / n, h[1] / n, h[2] / n, h[3] / n, h[4] / n, h[6] / n);
    }
#endif
    if (hr.status == 0) {
      j.tier = 3;
      j.out_len = hr.out_len;
      j.status = hr.out_len > j.cap ? ZES_E_NOSPACE : ZES_OK;
      if (j.want_end) HIPCHK(hipMemcpy(&j.end_bit, g.resume.p, 8, hipMemcpyDeviceToHost));  // (k_inf_decode puts it there when done)
      return ZES_OK;
    }
    have_resume = true;
  }
  // T4: exact restatement from the failing block on
  {
    Timed t("k_inf_exact");
    hipLaunchKernelGGL(k_inf_exact, dim3(1), dim3(64), 0, g.stream, d_in, j.in_off, j.c, d_out, j.out_off, j.cap,
                       have_resume ? (const uint64_t*)g.resume.p : (const uint64_t*)nullptr, (ZesRes*)g.res.p);
  }
  if ((rc = read_res(&hr))) return rc;
  if (j.want_end) {
    ZesRes r2;
    HIPCHK(hipMemcpy(&r2, (const ZesRes*)g.res.p + 1, sizeof r2, hipMemcpyDeviceToHost));
    j.end_bit = r2.out_len;
  }
  j.tier = 4;
  j.out_len = hr.out_len;
  j.status = hr.status;
  return ZES_OK;
}

// A reference-made stream too long for 32-bit bit positions (c >= 512 MiB), or any stream when ZES_F_PIECES asks for it
// (testing aid): T1 piece by piece.  A piece = the blocks that start inside the next `piece` bytes behind the end of
// the piece before; it is handed over with enough bytes behind it for its last block and the header behind that.
constexpr uint64_t T1_PIECE = 256ull << 20;
constexpr uint64_t T1_PIECE_SLACK = 1ull << 20;
// Where the buffer of a piece that starts at stream bit `bit` begins: a 16-byte boundary, one in front of the bit's own
// (the block search starts 16 bits into a buffer: keep the piece's first block behind that)
uint64_t t1_piece_origin(uint64_t bit) {
  uint64_t byte0 = (bit >> 3) & ~15ull;
  if (byte0 >= 16) byte0 -= 16;
  return byte0;
}
int inflate_pieces(const uint8_t* d_in, uint8_t* d_out, InfJob& j, uint32_t flags) {
  uint64_t piece = T1_PIECE;
  if (flags & ZES_F_PIECES) piece = 1ull << 20;  // testing aid: 1 MiB pieces
  uint64_t pos_bit = 16, total = 0, blocks = 0;
  for (uint32_t round = 0; round < (1u << 20); round++) {
    const uint64_t byte0 = t1_piece_origin(pos_bit);
    const uint64_t rel = pos_bit - 8 * byte0;
    const uint64_t pc = std::min<uint64_t>(j.c - byte0, piece + T1_PIECE_SLACK);
    const uint64_t done_bytes = blocks * ZES_BLK;
    RangeRes rr;
    int rc = inflate_t1_range(d_in, j.in_off + byte0, pc, rel, rel + piece * 8, true, d_out, j.out_off + std::min(done_bytes, j.cap),
                              j.cap > done_bytes ? j.cap - done_bytes : 0, flags, &rr);
    if (rc) return rc;
    if (!rr.handled || rr.nblocks == 0) return ZES_OK;  // not a clean chain: the other tiers decide
    blocks += rr.nblocks;
    total += rr.out_len;
    pos_bit = 8 * byte0 + rr.end_bit;
    if (rr.final_block) {
      j.tier = 1;
      j.out_len = total;
      j.end_bit = pos_bit;
      j.status = total > j.cap ? ZES_E_NOSPACE : ZES_OK;
      return ZES_OK;
    }
    if (pos_bit >= j.c * 8) return ZES_OK;
  }
  return ZES_OK;
}

// One byte of each of a group's buffers (byte `at` of jobs[ids[k]], k < nb <= INF_GROUP), gathered on the device
// (k_inf_first_bytes) and read back in one piece: *bytes points at them, in the page-locked area, until the next call.
int gather_bytes(const uint8_t* d_in, const std::vector<InfJob>& jobs, const uint32_t* ids, uint32_t nb, uint32_t at, const uint8_t** bytes) {
  int rc;
  if ((rc = ensure(g.ibufs, (size_t)INF_GROUP * 8 + INF_GROUP))) return rc;
  uint64_t* ho = g.pinned->first.offs;
  for (uint32_t k = 0; k < nb; k++) ho[k] = jobs[ids[k]].in_off + at;
  uint8_t* dfirst = (uint8_t*)g.ibufs.p + (size_t)INF_GROUP * 8;
  HIPCHK(hipMemcpyAsync(g.ibufs.p, ho, (size_t)nb * 8, hipMemcpyHostToDevice, g.stream));
  hipLaunchKernelGGL(k_inf_first_bytes, dim3((nb + 255) / 256), dim3(256), 0, g.stream, d_in, (const uint64_t*)g.ibufs.p, dfirst, nb);
  HIPCHK(hipMemcpyAsync(g.pinned->first.bytes, dfirst, nb, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  *bytes = g.pinned->first.bytes;
  return ZES_OK;
}

// All jobs of a call: T1 in groups, then the stragglers one by one.  jobs[i].status must be ZES_OK
// for the buffers to decode (anything else is left untouched).  firsts[i] = first byte of buffer i.
int inflate_jobs(const uint8_t* d_in, uint8_t* d_out, std::vector<InfJob>& jobs, const uint8_t* firsts, uint32_t flags) {
  g.last_tier = 0;
  g.sv.drop();  // (a survivor list serves the call that made it: the bytes behind a pointer may have changed since)
  std::vector<uint32_t> ids;
  std::vector<uint32_t> todo;
  std::vector<uint32_t> small;  // buffers T1 does not take and whose first byte is still on the device
  for (uint32_t i = 0; i < jobs.size(); i++) {
    InfJob& j = jobs[i];
    j.out_len = 0;
    j.tier = 0;
    if (j.status) continue;
    if (j.c == 0 || (firsts && (firsts[i] & 15u) != 8u)) {  // src/zlib.ts:13-16
      j.status = ZES_E_NOT_DEFLATE;
      j.tier = -1;
      continue;
    }
    todo.push_back(i);
    if (t1_eligible(j, flags)) ids.push_back(i);
    else if (!firsts) small.push_back(i);
  }
  int rc;
  // first bytes nobody supplied: T1 gets them back with its counters; the buffers T1 does not take are
  // gathered here (device kernel + one read-back per group)
  for (size_t g0 = 0; g0 < small.size(); g0 += INF_GROUP) {
    const uint32_t nb = (uint32_t)std::min<size_t>(INF_GROUP, small.size() - g0);
    const uint8_t* fb = nullptr;
    if ((rc = gather_bytes(d_in, jobs, small.data() + g0, nb, 0, &fb))) return rc;
    for (uint32_t k = 0; k < nb; k++)
      if ((fb[k] & 15u) != 8u) {
        jobs[small[g0 + k]].status = ZES_E_NOT_DEFLATE;
        jobs[small[g0 + k]].tier = -1;
      }
  }
  for (size_t g0 = 0; g0 < ids.size(); g0 += INF_GROUP) {
    const uint32_t nb = (uint32_t)std::min<size_t>(INF_GROUP, ids.size() - g0);
    if ((rc = inflate_t1_group(d_in, d_out, jobs.data(), ids.data() + g0, nb, firsts == nullptr, flags))) return rc;
  }
  // streams too long for the block-parallel tier's 32-bit bit positions (and ZES_F_PIECES): the same tier, piece by piece
  for (uint32_t i : todo) {
    InfJob& j = jobs[i];
    if (j.tier != 0 || j.status != ZES_OK || (flags & ZES_F_NO_FASTPATH)) continue;
    if (!(j.c >= (1ull << 29) || ((flags & ZES_F_PIECES) && j.c >= 64))) continue;
    if (firsts == nullptr) {  // the CM nibble (src/zlib.ts:13-16) was not checked on the way for this one
      HIPCHK(hipMemcpyAsync(g.pinned->first.bytes, d_in + j.in_off, 1, hipMemcpyDeviceToHost, g.stream));
      HIPCHK(hipStreamSynchronize(g.stream));
      if ((g.pinned->first.bytes[0] & 15u) != 8u) {
        j.status = ZES_E_NOT_DEFLATE;
        j.tier = -1;
        continue;
      }
    }
    if ((rc = inflate_pieces(d_in, d_out, j, flags))) return rc;
  }
  // Many streams the block-parallel tier left over (a batch of another encoder's streams): one serial wavefront
  // per stream, all at once — 512 of them run side by side, where the per-buffer tiers would take the streams one
  // after the other.  Streams that fail here go on to the per-buffer tiers.
  {
    std::vector<uint32_t> rest;
    for (uint32_t i : todo)
      if (jobs[i].tier == 0 && jobs[i].status == ZES_OK && jobs[i].c >= 3 && jobs[i].c < SERIAL_BATCH_MAX_C) rest.push_back(i);
    if (rest.size() >= SERIAL_BATCH_MIN_JOBS) {
      for (size_t g0 = 0; g0 < rest.size(); g0 += INF_GROUP) {
        const uint32_t nb = (uint32_t)std::min<size_t>(INF_GROUP, rest.size() - g0);
        ZesInfBuf* hb = g.pinned->t1.table;
        for (uint32_t k = 0; k < nb; k++) hb[k] = inf_buf(jobs[rest[g0 + k]]);
        if ((rc = ensure(g.ibufs, sizeof(ZesInfBuf) * nb))) return rc;
        if ((rc = ensure(g.res, sizeof(ZesRes) * nb))) return rc;
        if ((rc = ensure(g.resume, (size_t)16 * nb))) return rc;
        HIPCHK(hipMemcpyAsync(g.ibufs.p, hb, sizeof(ZesInfBuf) * nb, hipMemcpyHostToDevice, g.stream));
        {
          Timed t("k_inf_decode_seq");
          hipLaunchKernelGGL(k_inf_decode, dim3(nb), dim3(64), 0, g.stream, d_in, d_out, (const ZesInfBuf*)g.ibufs.p, (ZesRes*)g.res.p,
                             (uint64_t*)g.resume.p);
        }
        ZesRes* hres = g.pinned->t1.res;
        HIPCHK(hipMemcpyAsync(hres, g.res.p, sizeof(ZesRes) * nb, hipMemcpyDeviceToHost, g.stream));
        bool want_end = false;  // (k_inf_decode leaves the bit behind a stream it finished in the first of its two words)
        for (uint32_t k = 0; k < nb; k++) want_end = want_end || jobs[rest[g0 + k]].want_end;
        const uint64_t* hend = g.pinned->t1.ends;
        if (want_end) HIPCHK(hipMemcpyAsync(g.pinned->t1.ends, g.resume.p, (size_t)16 * nb, hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
        for (uint32_t k = 0; k < nb; k++) {
          if (hres[k].status != 0) continue;
          InfJob& j = jobs[rest[g0 + k]];
          j.tier = 3;
          j.out_len = hres[k].out_len;
          j.status = hres[k].out_len > j.cap ? ZES_E_NOSPACE : ZES_OK;
          if (j.want_end) j.end_bit = hend[2 * k];
        }
      }
    }
  }
  if (!(flags & ZES_F_NO_FASTPATH)) {
    {
      // the stored-blocks walk is a launch and a read-back per buffer: with several buffers left, only those whose first
      // block IS a stored one (BTYPE, bits 1-2 of the byte behind the zlib header; gathered by one launch per group) try it
      // (a buffer the block-parallel tier has looked at comes with its first BTYPE: no attempt, and no launch to find out)
      std::vector<uint32_t> st;
      for (uint32_t i : todo)
        if (jobs[i].tier == 0 && jobs[i].status == ZES_OK && jobs[i].c >= STORED_MIN_C && (jobs[i].btype0 < 0 || jobs[i].btype0 == 0)) st.push_back(i);
      std::vector<char> want(st.size(), 1);
      if (st.size() >= 2) {
        for (size_t g0 = 0; g0 < st.size(); g0 += INF_GROUP) {
          const uint32_t nb = (uint32_t)std::min<size_t>(INF_GROUP, st.size() - g0);
          const uint8_t* fb = nullptr;
          if ((rc = gather_bytes(d_in, jobs, st.data() + g0, nb, 2, &fb))) return rc;
          for (uint32_t k = 0; k < nb; k++) want[g0 + k] = ((fb[k] >> 1) & 3u) == 0u;
        }
      }
      for (size_t q = 0; q < st.size(); q++)
        if (want[q] && (rc = inflate_stored(d_in, d_out, jobs[st[q]]))) return rc;
    }
    // (ZES_SEG_PIECE_MB set: every stream goes piece by piece, for tests)
    static const bool force_pieces = getenv("ZES_SEG_PIECE_MB") != nullptr;
    std::vector<uint32_t> segs;
    for (uint32_t i : todo)
      if (jobs[i].tier == 0 && jobs[i].status == ZES_OK && jobs[i].c >= SEG_MIN_C && jobs[i].c < SEG_PIECES_MIN_C && !force_pieces) segs.push_back(i);
    if (!segs.empty() && (rc = inflate_segments(d_in, d_out, jobs.data(), segs))) return rc;
    // Longer streams: the same tier, piece by piece.  Not only the ones beyond 32-bit bit positions (512 MiB): the tier
    // takes at most SEG_BUCKETS work items per buffer, so a long stream's candidates are thinned, every item is then
    // several blocks long, and all but the first of them are decoded by a lone wave — 155 MiB of zlib -1 text
    // (400 MiB): 88 ms in one go, 12.7 ms in five pieces.
    for (uint32_t i : todo)
      if (jobs[i].tier == 0 && jobs[i].status == ZES_OK && (jobs[i].c >= SEG_PIECES_MIN_C || (force_pieces && jobs[i].c >= SEG_MIN_C)) &&
          (rc = inflate_segments_pieces(d_in, d_out, jobs[i])))
        return rc;
  }
  int worst = 0;
  for (uint32_t i : todo) {
    if (jobs[i].tier == 0 && jobs[i].status == ZES_OK && (rc = inflate_slow(d_in, d_out, jobs[i]))) return rc;
    worst = std::max(worst, jobs[i].tier);
  }
  collect_times();
  g.last_tier = worst;
  return ZES_OK;
}

// One buffer at d_in+in_off (16-byte aligned), result at d_out+out_off (16-byte aligned).
// Returns the reference-equivalent status; *out_len = bytes produced (or needed on NOSPACE).
// end_bit (optional): on ZES_OK, the bit behind the stream's final block, relative to d_in + in_off (the raw stream starts at 16)
int inflate_one(const uint8_t* d_in, uint64_t in_off, uint64_t c, uint8_t* d_out, uint64_t out_off, uint64_t cap,
                uint64_t* out_len, uint32_t flags, int first_byte /* -1: still on the device */, uint64_t* end_bit = nullptr) {
  std::vector<InfJob> jobs(1);
  jobs[0] = InfJob{in_off, c, out_off, cap, 0, ZES_OK, 0};
  jobs[0].want_end = end_bit != nullptr;
  const uint8_t fb = (uint8_t)first_byte;
  int rc = inflate_jobs(d_in, d_out, jobs, first_byte < 0 ? nullptr : &fb, flags & ~ZES_F_CHECK_ADLER);
  if (rc) return rc;
  *out_len = jobs[0].out_len;
  if (end_bit) *end_bit = jobs[0].end_bit;
  return jobs[0].status;
}

int adler32_locked(const uint8_t* d_in, uint64_t n, uint32_t* adler_out);
int adler32_batch_locked(const uint8_t* d, const ZesCrcSeg* segs, uint32_t count, uint32_t* adler);

uint32_t get_le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
uint32_t get_le32(const uint8_t* p) { return get_le16(p) | get_le16(p + 2) << 16; }
void put_le16(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
}
void put_le32(uint8_t* p, uint32_t v) {
  put_le16(p, v);
  put_le16(p + 2, v >> 16);
}
uint32_t get_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
void put_be32(uint8_t* p, uint32_t v) {  // (the zlib trailer, src/zlib.ts:37-40)
  for (int k = 0; k < 4; k++) p[k] = (uint8_t)(v >> (24 - 8 * k));
}

// Adler-32 of a concatenation from its pieces' (src/adler32.ts:1-10): s1 adds up; a piece's s2 also sees len * (s1 so far - 1)
struct AdlerJoin {
  uint64_t s1 = 1, s2 = 0;
  void add(uint32_t adler, uint64_t len) {
    s2 = (s2 + (adler >> 16) + (len % 65521u) * ((s1 + 65520u) % 65521u)) % 65521u;
    s1 = (s1 + (adler & 0xFFFFu) + 65520u) % 65521u;
  }
  uint32_t value() const { return (uint32_t)((s2 << 16) | s1); }
};

// segs[i].len bytes from src + src_off to dst + dst_off for every i, in one launch (k_gz_gather); the table goes through g.gz_tab
int gz_gather(const uint8_t* src, uint8_t* dst, const std::vector<ZesGzSeg>& segs) {
  if (segs.empty()) return ZES_OK;
  int rc;
  uint64_t longest = 0;
  for (const ZesGzSeg& s : segs) longest = std::max(longest, s.len);
  if ((rc = ensure(g.gz_tab, sizeof(ZesGzSeg) * segs.size()))) return rc;
  HIPCHK(hipMemcpyAsync(g.gz_tab.p, segs.data(), sizeof(ZesGzSeg) * segs.size(), hipMemcpyHostToDevice, g.stream));
  const uint32_t ny = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((longest + GZ_GATHER_PIECE - 1) / GZ_GATHER_PIECE, 1), 256);
  Timed t("k_gz_gather");
  hipLaunchKernelGGL(k_gz_gather, dim3((uint32_t)segs.size(), ny), dim3(GZ_GATHER_THREADS), 0, g.stream, src, dst, (const ZesGzSeg*)g.gz_tab.p);
  HIPCHK(hipGetLastError());
  return ZES_OK;
}

// ---- BGZF members: the rule, and the walk over a file on the host and on the device ----
// One member at h[0, avail) of a file with `left` bytes from its start on: does it qualify, and what does it say
// (the rule of k_gz_walk, which does the same on the device)
bool gz_member(const uint8_t* h, uint64_t avail, uint64_t left, ZesGzMember* m) {
  if (avail < 12 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4) return false;
  const uint32_t hlen = 12 + ((uint32_t)h[10] | (uint32_t)h[11] << 8);
  if (hlen > ZES_GZ_HLEN_MAX || hlen > avail) return false;
  uint32_t p = 12, size = 0;
  while (p + 4 <= hlen) {
    const uint32_t sl = (uint32_t)h[p + 2] | (uint32_t)h[p + 3] << 8;
    if (p + 4 + sl > hlen) break;
    if (!size && h[p] == 'B' && h[p + 1] == 'C' && sl == 2) size = ((uint32_t)h[p + 4] | (uint32_t)h[p + 5] << 8) + 1;
    p += 4 + sl;
  }
  if (p != hlen || !size || hlen + 8 > size || size > left) return false;
  m->size = size;
  m->hlen = hlen;
  return true;
}

// The members of the file h[0, c) from byte 0 on, each one to each(pos, member); true when they reach the file's end
template <class F>
bool gz_walk_host(const uint8_t* h, uint64_t c, F each) {
  for (uint64_t pos = 0; pos < c;) {
    ZesGzMember m;
    if (!gz_member(h + pos, c - pos, c - pos, &m)) return false;
    each(pos, m);
    pos += m.size;
  }
  return true;
}

// The same on the device (k_gz_walk, one wave).  Precondition: gz_walk_room(cap) has succeeded, so that g.gz_tab holds the head
// and a table of `cap` members (sizing is the caller's statement: a table that cannot be sized means "not applicable" to
// one caller and an error to the other).  The head comes down, and the table (head.count members) when accept(head) says
// so; else tab stays empty.
int gz_walk_room(uint64_t cap) { return ensure(g.gz_tab, sizeof(ZesGzWalk) + sizeof(ZesGzMember) * (size_t)cap); }
template <class F>
int gz_walk_dev(const uint8_t* d, uint64_t c, uint32_t cap, F accept, std::vector<ZesGzMember>& tab) {
  tab.clear();
  ZesGzWalk head;
  ZesGzWalk* d_head = (ZesGzWalk*)g.gz_tab.p;
  {
    Timed t("k_gz_walk");
    hipLaunchKernelGGL(k_gz_walk, dim3(1), dim3(64), 0, g.stream, d, c, d_head, (ZesGzMember*)(d_head + 1), cap);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&head, d_head, sizeof head, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  if (!accept(head)) return ZES_OK;
  tab.resize(head.count);
  HIPCHK(hipMemcpyAsync(tab.data(), d_head + 1, sizeof(ZesGzMember) * tab.size(), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return ZES_OK;
}

// the segments gathered into `pool` and brought down: `bytes` in all at h_dst (no segments: nothing happens)
int gather_down(DevBuf& pool, const uint8_t* src, const std::vector<ZesGzSeg>& segs, uint8_t* h_dst, size_t bytes) {
  if (segs.empty()) return ZES_OK;
  int rc;
  if ((rc = ensure(pool, bytes))) return rc;
  if ((rc = gz_gather(src, (uint8_t*)pool.p, segs))) return rc;
  HIPCHK(hipMemcpyAsync(h_dst, pool.p, bytes, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return ZES_OK;
}

// ZES_F_CHECK_ADLER: the Adler-32 trailer of a zlib stream of c bytes whose final block ends at bit end_bit (relative to the
// header's first byte) is the 4 bytes from *t on, big-endian; false when they are not all there
bool adler_trailer_at(uint64_t end_bit, uint64_t c, uint64_t* t) {
  *t = (end_bit + 7) / 8;
  return end_bit >= 16 && *t + 4 <= c;
}

// ZES_F_CHECK_ADLER of one stream: its trailer must exist and hold the Adler-32 of the n result bytes at d_res.  The
// stream's bytes are at h_in (host) or d_in (device).
int check_adler_trailer(const uint8_t* h_in, const uint8_t* d_in, uint64_t c, uint64_t end_bit, const uint8_t* d_res, uint64_t n) {
  uint64_t t;
  if (!adler_trailer_at(end_bit, c, &t)) return ZES_E_CHECKSUM;
  uint8_t b[4];
  if (h_in) memcpy(b, h_in + t, 4);
  else HIPCHK(hipMemcpy(b, d_in + t, 4, hipMemcpyDeviceToHost));
  uint32_t ad = 0;
  int rc = adler32_locked(d_res, n, &ad);
  if (rc) return rc;
  return ad == get_be32(b) ? ZES_OK : ZES_E_CHECKSUM;
}

// ZES_F_CHECK_ADLER for the jobs of the inflate_jobs call in front that had want_end set.  Of those that ended ZES_OK: their
// trailers (the streams in the caller's memory at h_in[k] when given, else inside d_in: one gather of 4-byte segments into
// g.adlerseg and one read-back) against the Adler-32 of their outputs (one k_adler_seg launch).  A job that fails gets
// ZES_E_CHECKSUM; any other status stays, and a job whose trailer is cut short costs no launch.  The launches of both
// calls show in the call's times.
int check_adler_jobs(const uint8_t* d_in, const uint8_t* const* h_in, const uint8_t* d_out, std::vector<InfJob>& jobs) {
  keep_times();
  std::vector<uint32_t> who;
  std::vector<ZesGzSeg> segs;  // the trailers: from the job's stream to 4 bytes each, in the order of `who`
  for (uint32_t k = 0; k < jobs.size(); k++) {
    InfJob& j = jobs[k];
    if (j.status != ZES_OK) continue;
    uint64_t t;
    if (!adler_trailer_at(j.end_bit, j.c, &t)) {
      j.status = ZES_E_CHECKSUM;
      continue;
    }
    segs.push_back(ZesGzSeg{t, 4 * who.size(), 4, 0u, 0u});
    who.push_back(k);
  }
  const size_t n = who.size();
  std::vector<uint8_t> trail(4 * n);
  int rc = ZES_OK;
  if (h_in) {
    for (size_t q = 0; q < n; q++) memcpy(&trail[4 * q], h_in[who[q]] + segs[q].src_off, 4);
  } else {
    for (size_t q = 0; q < n; q++) segs[q].src_off += jobs[who[q]].in_off;
    rc = gather_down(g.adlerseg, d_in, segs, trail.data(), trail.size());
  }
  std::vector<ZesCrcSeg> csegs(n);
  for (size_t q = 0; q < n; q++) csegs[q] = ZesCrcSeg{jobs[who[q]].out_len ? jobs[who[q]].out_off : 0, jobs[who[q]].out_len};
  std::vector<uint32_t> ad(n);
  if (!rc && !(rc = adler32_batch_locked(d_out, csegs.data(), (uint32_t)n, ad.data())))
    for (size_t q = 0; q < n; q++)
      if (ad[q] != get_be32(&trail[4 * q])) jobs[who[q]].status = ZES_E_CHECKSUM;
  collect_times();
  return rc;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------
extern "C" {

const char* zes_strerror(int status) {
  switch (status) {
    case ZES_OK: return "ok";
    case ZES_E_NOT_DEFLATE: return "Not compressed by deflate";
    case ZES_E_BTYPE3: return "Not supported BTYPE : 3";
    case ZES_E_CORRUPT: return "Data is corrupted";
    case ZES_E_INSUFFICIENT: return "Data length is insufficient";
    case ZES_E_LACK: return "Lack of data length";
    case ZES_E_NOSPACE: return "zes: output capacity too small";
    case ZES_E_DEVICE: return "zes: HIP device error (no gfx950 device or runtime failure)";
    case ZES_E_ARG: return "zes: bad argument";
    case ZES_E_NOTRANGE: return "zes: not a clean chain of reference-made blocks in this range";
    case ZES_E_GZIP: return "zes: not a valid gzip member (header or trailer)";
    case ZES_E_CHECKSUM: return "zes: checksum mismatch";
    case ZES_E_ZIP: return "zes: not a valid ZIP archive or entry (end record, directory or local header)";
    case ZES_E_UNSUPPORTED: return "zes: unsupported ZIP feature (ZIP64, several disks, encryption, a method other than 0 or 8)";
    case ZES_E_PNG: return "zes: not a valid PNG file (signature, chunk chain or header), or image data that does not fit its header";
    case ZES_E_TIFF: return "zes: not a valid TIFF file (header, directory chain or tags), or image data that does not fit its directory";
    default: return "zes: unknown status";
  }
}

int zes_init(int device) {
  UseDev ud(0);
  std::lock_guard<std::mutex> lk(g_mu);
  return init_locked(device);
}

int zes_init_devices(int n) {
  int have = 0;
  if (hipGetDeviceCount(&have) != hipSuccess || have <= 0) return ZES_E_DEVICE;
  // ZES_OVERSUBSCRIBE: more contexts than devices, context i on device i % devices (exercises the multi-device paths on a one-GPU box)
  const bool over = getenv("ZES_OVERSUBSCRIBE") != nullptr;
  if (n <= 0) n = have;
  if (n > ZES_MAX_DEV || (n > have && !over)) return ZES_E_ARG;
  std::lock_guard<std::mutex> cfg(g_cfg_mu);
  for (int i = 0; i < n; i++) {
    std::lock_guard<std::mutex> lk(g_mus[i]);
    const int dev = i % have;
    if (g_ctx[i].ready ? g_ctx[i].device != dev : (g_ctx[i].want >= 0 && g_ctx[i].want != dev)) return ZES_E_ARG;  // bound elsewhere already
    g_ctx[i].want = dev;
  }
  if (n > g_nctx.load()) g_nctx.store(n);
  for (int i = 0; i < n; i++) {  // bring every context up now: a first batch should not pay for it
    UseDev ud(i);
    LOCK_READY();
  }
  return ZES_OK;
}

static int shutdown_one(void);
int zes_shutdown(void) {
  std::lock_guard<std::mutex> cfg(g_cfg_mu);
  int rc = ZES_OK;
  for (int i = 0; i < ZES_MAX_DEV; i++) {
    t_dev = i;  // (not a routed call: every context in turn)
    const int r = shutdown_one();
    if (r && !rc) rc = r;
    g_ctx[i].want = -1;
  }
  t_dev = 0;
  g_nctx.store(1);
  return rc;
}

// every pooled device buffer of the current context
static void free_scratch_locked() {
  for_each_pool(g, [](DevBuf& b) { (void)release(b); });
}

int zes_trim(void) {
  std::lock_guard<std::mutex> cfg(g_cfg_mu);
  const int keep = t_dev;
  for (int i = 0; i < ZES_MAX_DEV; i++) {
    t_dev = i;  // (not a routed call: every context in turn)
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g.ready) continue;
    (void)hipSetDevice(g.device);
    (void)hipStreamSynchronize(g.stream);
    free_scratch_locked();  // (the scan's constant table, g.kraft, stays)
  }
  t_dev = keep;
  return ZES_OK;
}

static int shutdown_one(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g.ready) return ZES_OK;
  (void)hipSetDevice(g.device);
  (void)hipStreamSynchronize(g.stream);
  free_scratch_locked();
  (void)release(g.kraft);
  if (g.pinned) (void)hipHostFree(g.pinned);
  if (g.mirror) (void)hipHostFree(g.mirror);
  if (g.res_more) (void)hipHostFree(g.res_more);
  g.pinned = g.pinned_dev = nullptr;
  g.mirror = g.mirror_dev = nullptr;
  g.res_more = nullptr;
  g.res_more_n = 0;
  g_side_up.shutdown();
  g_side_down.shutdown();
  g_up.release();
  g_down.release();
  for (hipEvent_t e : g.event_pool) (void)hipEventDestroy(e);
  g.event_pool.clear();
  (void)hipStreamDestroy(g.stream);
  (void)hipStreamDestroy(g.cs_in);
  (void)hipStreamDestroy(g.cs_out);
  for (int k = 0; k < 2; k++) (void)hipEventDestroy(g.ev_up[k]);
  for (int k = 0; k < 2; k++) (void)hipEventDestroy(g.ev_rng[k]);
  (void)hipEventDestroy(g.ev_k);
  (void)hipStreamDestroy(g.s_adler);
  (void)hipEventDestroy(g.ev_a0);
  (void)hipEventDestroy(g.ev_a1);
  g.s_adler = nullptr;
  g.stream = g.cs_in = g.cs_out = nullptr;
  g.ready = false;
  return ZES_OK;
}

int zes_host_alloc(uint64_t n, void** p) {
  UseDev ud(0);  // (page-locked memory belongs to the process: always through context 0)
  if (!p) return ZES_E_ARG;
  *p = nullptr;
  LOCK_READY();
  HIPCHK(hipHostMalloc(p, n ? n : 1, hipHostMallocPortable));  // (page-locked for every device the library drives)
  return ZES_OK;
}

int zes_host_free(void* p) {
  if (!p) return ZES_OK;
  // page-locked memory belongs to the process, not to a stream: it can be given back after zes_shutdown too (a JS
  // finalizer may run that late), and hipHostFree waits by itself for device work that still uses the block
  std::lock_guard<std::mutex> lk(g_mu);
  if (g.ready) (void)hipSetDevice(g.device);
  HIPCHK(hipHostFree(p));
  return ZES_OK;
}

int zes_device_info(char* name, int cap, int* cus, uint64_t* hbm_bytes) {
  LOCK_READY();
  if (name && cap > 0) snprintf(name, (size_t)cap, "%s", g.arch);
  if (cus) *cus = g.cus;
  if (hbm_bytes) *hbm_bytes = g.hbm;
  return ZES_OK;
}

int zes_deflate_bound(uint64_t n, uint64_t* cap) {
  if (!cap) return ZES_E_ARG;
  *cap = deflate_bound(n);
  return ZES_OK;
}

int zes_deflate_batch_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* d_out,
                          const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t count) {
  ROUTE_DEV(d_in, d_out);
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return ZES_E_ARG;
  LOCK_READY();
  return deflate_batch_core(d_in, in_off, in_len, d_out, out_off, out_cap, out_len, status, count);
}

int zes_deflate_dev(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len) {
  ROUTE_DEV(d_in, d_out);
  if (!out_len) return ZES_E_ARG;
  LOCK_READY();
  return deflate_one(d_in, 0, n, d_out, 0, cap, out_len);
}

// The conveyor of the two pipelined host calls below: the caller's buffer goes up piece by piece on g.cs_in (one side
// thread), finished windows of the result go down on g.cs_out (another), and g.stream waits for a piece's upload by its
// event, ev_up[k & 1].  What a piece is, when the next one is sent up and when a window goes down is the caller's.
// The side tasks use this object and, through `rule` and `stamp`, the caller's frame: declare it behind everything they
// touch, so that it is destroyed first — its destructor waits for both tasks on every way out of the caller.
// A download into pinned memory is only enqueued (download(..., wait = false)): a caller that has sent anything leaves
// through drain(), which synchronises g.cs_out.
struct HostPipe {
  const uint8_t* src;  // the caller's buffer, n bytes
  uint8_t* d_src;      // its place on the device
  uint64_t n;
  uint32_t np;                                       // pieces
  std::function<uint64_t(uint32_t)> rule;            // upload k carries [cut(k), cut(k + 1)): cut(k) = min(n, rule(k)) for 0 < k < np
  std::function<void(const char*, uint32_t)> stamp;  // ZES_PIPE_DBG's timeline ("up done", "down issued"): may be empty
  std::future<int> f_up, f_down;
  bool in_flight = false;  // a window may still be on its way into the caller's memory
  ~HostPipe() {  // no side task may outlive the frame whose variables it uses, no copy the call
    (void)settle();
    if (in_flight) (void)hipStreamSynchronize(g.cs_out);  // (an error's way out: drain() was not reached)
  }
  static int settle(std::future<int>& f) { return f.valid() ? f.get() : (int)ZES_OK; }
  int settle() {  // both side tasks done: the first one's error, else the second's
    const int ru = settle(f_up), rd = settle(f_down);
    return ru ? ru : rd;
  }
  uint64_t cut(uint32_t k) const { return k == 0 ? 0ull : k >= np ? n : std::min<uint64_t>(n, rule(k)); }
  int up(uint32_t k) {  // (an upload of no bytes still records its event)
    const uint64_t a = cut(k), b = cut(k + 1);
    const int r = upload(d_src + a, src + a, b - a, g.cs_in);
    if (r == ZES_OK) HIPCHK(hipEventRecord(g.ev_up[k & 1], g.cs_in));
    if (stamp) stamp("up done", k);
    return r;
  }
  void submit_up(uint32_t k) { f_up = g_side_up.submit([this, k] { return up(k); }); }
  // piece k is up, or on its way with its event recorded: g.stream waits for it (`next`: a piece to send up first, so
  // that its upload starts in front of the wait's enqueue: the pipelined inflate, whose uploads lead by two)
  int ready(uint32_t k, uint32_t next = UINT32_MAX) {
    if (const int rc = settle(f_up)) return rc;
    if (next < np) submit_up(next);
    HIPCHK(hipStreamWaitEvent(g.stream, g.ev_up[k & 1], 0));
    return ZES_OK;
  }
  // bytes [a, b) of the result on their way to the caller, behind the window sent before (`k`: for the timeline)
  int send(uint8_t* out, const uint8_t* d_out, uint64_t a, uint64_t b, uint32_t k) {
    if (const int rc = settle(f_down)) return rc;
    in_flight = true;
    f_down = g_side_down.submit([this, out, d_out, a, b, k] {
      const int r = download(out + a, d_out + a, b - a, g.cs_out, false);
      if (stamp) stamp("down issued", k);
      return r;
    });
    return ZES_OK;
  }
  // the one tail: both side tasks done, a last window [a, b) if there is one, and every byte sent has arrived
  int drain(uint8_t* out = nullptr, const uint8_t* d_out = nullptr, uint64_t a = 0, uint64_t b = 0) {
    int rc = settle();
    if (rc) return rc;
    in_flight = in_flight || b > a;
    if (b > a && (rc = download(out + a, d_out + a, b - a, g.cs_out, false))) return rc;
    HIPCHK(hipStreamSynchronize(g.cs_out));
    in_flight = false;
    return ZES_OK;
  }
};

// Host deflate of a large buffer in pieces of 256 blocks (one workgroup per CU), so that the three legs overlap: while
// the kernels work on piece k, piece k+1 crosses PCIe on one copy stream and the finished bytes of piece k-1 go back
// on another.  A piece is a block range (the machinery of zes_deflate_range_dev): it is emitted straight at its place
// in the output stream — bit offset = all bits before it, known when the piece before has finished — and continues
// the last dword of the piece before (ZES_BUF_CONT).  78 9C and the Adler-32 of the whole input (combined from the
// pieces': src/adler32.ts:1-10 is associative) are put into the caller's buffer by the host.  Same bytes as the
// one-pass path (tests/test_gpu_configs.py::test_pipelined_host_calls).
constexpr uint64_t PIPE_PIECE = 256ull * ZES_BLK;  // 32 MiB
constexpr uint64_t PIPE_MIN = PIPE_PIECE + PIPE_PIECE / 2;
constexpr uint64_t PIPE_HALO = 4096;  // a piece's match finder reads up to 258 bytes behind it: uploads are cut this far behind the piece ends
static int deflate_host_pipelined(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  int rc;
  const uint64_t bound = deflate_bound(n);
  if ((rc = ensure(g.st_in, n + 64))) return rc;
  if ((rc = ensure(g.st_out, bound + 64))) return rc;
  const uint8_t* d_in = (const uint8_t*)g.st_in.p;
  uint8_t* d_out = (uint8_t*)g.st_out.p;
  const uint32_t np = (uint32_t)((n + PIPE_PIECE - 1) / PIPE_PIECE);
  const bool pdbg = getenv("ZES_PIPE_DBG") != nullptr;
  const auto t00 = std::chrono::steady_clock::now();
  auto stamp = [&](const char* what, uint32_t k) {
    if (pdbg) fprintf(stderr, "  pipe %-14s %u  %.3f ms\n", what, k, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t00).count());
  };
  uint64_t pos = 16;  // bit position of the next piece in the output stream (behind 78 9C)
  uint64_t sent = 0;  // bytes of the output already on their way to the caller
  AdlerJoin adler;    // of the pieces so far
  const bool out_fits = cap >= bound;  // (else: count first, the caller gets the size needed)
  uint64_t pend_lo = 0, pend_hi = 0;   // bytes of the output finished by the piece before, not yet sent
  HostPipe pipe{in, (uint8_t*)g.st_in.p, n, np, [](uint32_t k) { return (uint64_t)k * PIPE_PIECE + PIPE_HALO; }, stamp};
  if ((rc = pipe.up(0))) return rc;
  for (uint32_t k = 0; k < np; k++) {
    const uint64_t lo = (uint64_t)k * PIPE_PIECE, len = std::min<uint64_t>(PIPE_PIECE, n - lo);
    const uint64_t o_off = (pos >> 7) << 4;  // 16-byte aligned byte offset; the piece starts start_bit bits into it
    DeflateRange piece{std::min<uint64_t>(n - lo, len + 258), ZES_BUF_RANGE | (k + 1 < np ? ZES_BUF_NOTFINAL : 0u) | (k ? ZES_BUF_CONT : 0u),
                       (uint32_t)(pos - o_off * 8), true};  // readable, flags, start bit, deferred
    uint64_t bits = 0;
    if ((rc = pipe.ready(k))) return rc;
    if ((rc = deflate_one(d_in, lo, len, d_out, o_off, bound + 64 - o_off, &bits, &piece))) return rc;
    // beside the kernels: the next piece up, the bytes the piece before finished down
    stamp("launched", k);
    if (k + 1 < np) pipe.submit_up(k + 1);
    if (out_fits && pend_hi > pend_lo) {
      if ((rc = pipe.send(out, d_out, pend_lo, pend_hi, k))) return rc;
      sent = pend_hi;
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    collect_times();
    stamp("kernels done", k);
    const ZesRes* r = g.pinned->def.res;
    if (r[0].status) return r[0].status;
    pos += r[0].out_len;
    adler.add(r[0].aux, len);
    pend_lo = sent;
    pend_hi = (k + 1 < np) ? (pos >> 3) : ((pos + 7) >> 3);  // whole bytes; the last piece's padded end
  }
  const uint64_t raw_end = (pos + 7) >> 3, total = raw_end + 4;
  if (out_fits && (rc = pipe.drain(out, d_out, pend_lo, pend_hi))) return rc;  // (total <= bound <= cap)
  *out_len = total;
  if (total > cap) return ZES_E_NOSPACE;
  // a capacity below the bound that still holds the result: nothing has gone down so far, one copy now
  if (!out_fits && (rc = download(out, d_out, raw_end, g.cs_out, true))) return rc;
  stamp("all down", np);
  out[0] = 0x78;  // src/zlib.ts:29-34
  out[1] = 0x9C;
  put_be32(out + raw_end, adler.value());
  return ZES_OK;
}

int zes_deflate(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  UseDev ud(route_host());
  if (!out_len || (!in && n) || !out) return ZES_E_ARG;
  *out_len = 0;
  if (deflate_throws(n)) return ZES_E_CORRUPT;
  const uint64_t bound = deflate_bound(n);
  {
    LOCK_READY();
    if (n >= PIPE_MIN && !getenv("ZES_NO_PIPELINE")) return deflate_host_pipelined(in, n, out, cap, out_len);
    if ((rc = ensure(g.st_out, bound + 64))) return rc;
    if ((rc = stage_in(g.st_in, in, n))) return rc;
    uint64_t dl = 0;
    if ((rc = deflate_one((const uint8_t*)g.st_in.p, 0, n, (uint8_t*)g.st_out.p, 0, bound, &dl))) return rc;
    *out_len = dl;
    if (dl > cap) return ZES_E_NOSPACE;
    return download(out, (const uint8_t*)g.st_out.p, dl);
  }
}

int zes_inflate_dev(const uint8_t* d_in, uint64_t c, uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  host_lap("(outside the library)");
  ROUTE_DEV(d_in, d_out);
  if (!out_len) return ZES_E_ARG;
  if ((((uintptr_t)d_in) & 15u) || (((uintptr_t)d_out) & 15u)) return ZES_E_ARG;
  LOCK_READY();
  if (!(flags & ZES_F_CHECK_ADLER)) return inflate_one(d_in, 0, c, d_out, 0, cap, out_len, flags, -1);
  uint64_t eb = 0;
  rc = inflate_one(d_in, 0, c, d_out, 0, cap, out_len, flags, -1, &eb);
  return rc ? rc : check_adler_trailer(nullptr, d_in, c, eb, d_out, *out_len);
}

int zes_inflate_batch_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint8_t* d_out,
                          const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t count,
                          uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (!in_off || !in_len || !out_off || !out_cap || !out_len || !status) return ZES_E_ARG;
  if ((((uintptr_t)d_in) & 15u) || (((uintptr_t)d_out) & 15u)) return ZES_E_ARG;
  LOCK_READY();
  for (uint32_t i = 0; i < count; i++) status[i] = ((in_off[i] & 15u) || (out_off[i] & 15u)) ? ZES_E_ARG : ZES_OK;
  std::vector<InfJob> jobs(count);
  for (uint32_t i = 0; i < count; i++) jobs[i] = InfJob{in_off[i], in_len[i], out_off[i], out_cap[i], 0, status[i], 0};
  const bool check = (flags & ZES_F_CHECK_ADLER) != 0;
  if (check)
    for (InfJob& j : jobs) j.want_end = true;
  rc = inflate_jobs(d_in, d_out, jobs, nullptr, flags & ~ZES_F_CHECK_ADLER);  // the first bytes (CM nibble, src/zlib.ts:13) are read on the way
  if (rc) return rc;
  if (check) {
    if ((rc = check_adler_jobs(d_in, nullptr, d_out, jobs))) return rc;
  }
  for (uint32_t i = 0; i < count; i++) {
    status[i] = jobs[i].status;
    out_len[i] = jobs[i].out_len;
  }
  return ZES_OK;
}

// Host inflate of a long reference-made stream in pieces, so that the three legs overlap: the stream is cut into equal
// bit ranges (as shard.inflate_split cuts it over GPUs); while the block-parallel tier decodes the blocks that start in
// range k (inflate_t1_range), a helper thread sends range k+1 up on one copy stream and the output of range k-1 down on
// another.  The ranges must chain (each one's first block where the one before ended, full blocks everywhere but at
// the end, BFINAL last); anything else — another encoder's stream, a false block start — and the call starts over on
// the one-pass path below, which has every tier.  *done = false then.
constexpr uint64_t PIPE_IN_MIN = 8ull << 20;
static int inflate_host_pipelined(const uint8_t* in, uint64_t c, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags,
                                  zes_alloc_fn alloc, void* user, bool* done) {
  *done = false;
  int rc;
  // Piece boundaries (multiples of 64 KiB).  A piece costs ~0.3 ms of launches and read-backs whatever its size, so
  // pieces of up to 32 MiB keep pace with their uploads; what cannot overlap anything is the LAST piece's decode and
  // download: from 48 MiB on the last piece is a small one (64 MiB of incompressible data: 8 + 24 + 24 + 8).
  std::vector<uint64_t> B;
  {
    uint64_t pb = std::min<uint64_t>(32ull << 20, std::max<uint64_t>(4ull << 20, ((c / 2 + 65535) >> 16) << 16));
    if (const char* e = getenv("ZES_PIPE_PIECE_MB")) pb = std::max<uint64_t>(1, strtoull(e, nullptr, 10)) << 20;  // (measurements)
    uint64_t last = 0;
    if (c >= (48ull << 20)) last = std::min<uint64_t>(8ull << 20, ((c / 8) >> 16) << 16);
    // ... and the FIRST piece's upload and decode, before the first byte can come down: a small one as well, when the
    // output is long enough to pay for one piece more (measured, pinned memory, ms per call without / with it: 64 MiB of
    // text 2.25 / 1.96, 128 MiB 4.02 / 3.45, 64 MiB of random bytes 2.36 / 2.28 — but 48 MiB of text 1.59 / 1.80, of
    // random bytes 2.01 / 2.16: a piece costs ~0.3 ms of launches and read-backs)
    const uint64_t est_out = (cap && !alloc) ? cap : c * 4;
    uint64_t first = (est_out >= (56ull << 20) && c >= (12ull << 20)) ? std::min<uint64_t>(8ull << 20, ((c / 3) >> 16) << 16) : 0;
    if (const char* e = getenv("ZES_PIPE_FIRST_MB")) first = strtoull(e, nullptr, 10) << 20;  // (measurements)
    if (first + last + (4ull << 20) > c) first = 0;
    const uint64_t rest = c - last - first;
    const uint64_t nr = std::max<uint64_t>(1, (rest + pb - 1) / pb);
    const uint64_t each = (((rest + nr - 1) / nr + 65535) >> 16) << 16;
    B.push_back(0);
    if (first) B.push_back(first);
    for (uint64_t k = 1; k < nr; k++)
      if (k * each < rest) B.push_back(first + k * each);
    if (last && first + rest > B.back()) B.push_back(first + rest);
    B.push_back(c);
  }
  const uint32_t np = (uint32_t)B.size() - 1;
  if (np < 2) return ZES_OK;
  const uint64_t dcap = std::max<uint64_t>(alloc ? 0 : cap, std::max<uint64_t>(c * 4, 1 << 20));
  if ((rc = ensure(g.st_in, c + 64))) return rc;
  if ((rc = ensure(g.st_out, dcap + 64))) return rc;
  const uint8_t* d_in = (const uint8_t*)g.st_in.p;
  uint8_t* d_out = (uint8_t*)g.st_out.p;
  {
    uint64_t cmax = 0;
    for (uint32_t k = 0; k < np; k++) cmax = std::max<uint64_t>(cmax, B[k + 1] - B[k] + T1_PIECE_SLACK + 64);
    if ((rc = range_reserve(cmax))) return rc;
  }
  uint64_t blocks = 0, total = 0, prev_end = 16, pend_lo = 0, pend_hi = 0;
  bool final_seen = false, chain = true;
  // compressible data or not (which form of the block decoder): by the whole call, not by a piece
  const bool two = c * 10 < std::min<uint64_t>(dcap, cap ? cap : dcap) * 7;
  bool early = alloc && (flags & ZES_F_ALLOC_BOUND);  // the allocator takes an upper estimate (include/zes.h)
  RangePiece pend[2];
  uint64_t byte0s[2] = {0, 0};
  auto begin = [&](uint32_t k) -> int {  // (behind pipe.ready(k): g.stream waits for range k's upload)
    const uint64_t lo_bit = k == 0 ? 16 : B[k] * 8, own_bit = B[k + 1] * 8;
    const uint64_t byte0 = byte0s[k & 1] = t1_piece_origin(lo_bit);
    const uint64_t pc = std::min<uint64_t>(c - byte0, (own_bit >> 3) - byte0 + T1_PIECE_SLACK);
    return range_begin((int)(k & 1), pend[k & 1], d_in, byte0, pc, lo_bit - 8 * byte0, own_bit - 8 * byte0, k == 0, d_out, dcap, two, flags);
  };
  HostPipe pipe{in, (uint8_t*)g.st_in.p, c, np, [&B](uint32_t k) { return B[k] + T1_PIECE_SLACK; }, nullptr};
  if ((rc = pipe.up(0)) || (rc = pipe.ready(0, 1)) || (rc = begin(0))) return rc;
  for (uint32_t k = 0; k < np && chain && !final_seen; k++) {
    if (k + 1 < np) {  // the next piece is enqueued before this one's results are waited for
      if ((rc = pipe.ready(k + 1, k + 2)) || (rc = begin(k + 1))) return rc;  // (upload k + 2 starts, then the wait for k + 1)
    }
    RangeRes rr;
    if ((rc = range_finish((int)(k & 1), pend[k & 1], &rr))) return rc;
    const uint64_t byte0 = byte0s[k & 1];
    if (!rr.handled) {
      chain = false;
    } else if (rr.nblocks) {
      if (rr.first_bit + 8 * byte0 != prev_end || total != blocks * ZES_BLK) {
        chain = false;
      } else {
        prev_end = rr.end_bit + 8 * byte0;
        pend_lo = std::min(total, cap);
        total += rr.out_len;
        pend_hi = std::min(total, cap);
        blocks += rr.nblocks;
        final_seen = rr.final_block;
        if (early && !out) {
          // the first piece is decoded: from its blocks' ratio an upper estimate of the whole result (5 % and two blocks on
          // top), asked for now, so that every piece's bytes can go down while the ones behind it are decoded
          const uint64_t in0 = std::max<uint64_t>(1, (prev_end + 7) / 8);
          const long double ratio = (long double)total / (long double)in0;
          uint64_t est = (uint64_t)((long double)c * ratio * 1.05L) + 2 * ZES_BLK;
          est = std::min<uint64_t>(std::max<uint64_t>(est, total), dcap);
          out = alloc(user, ZES_ALLOC_EARLY, est);
          if (out) {
            cap = est;
            pend_hi = std::min(total, cap);
          } else {
            early = false;  // "not now": the exact size, once, when it is known
          }
        }
        if (out && (!alloc || early) && pend_hi > pend_lo && !(final_seen || k + 1 == np)) {  // (the last piece's bytes go down below)
          if ((rc = pipe.send(out, d_out, pend_lo, pend_hi, k))) return rc;
          pend_lo = pend_hi = 0;
        }
      }
    }
  }
  const bool dbgp = getenv("ZES_DEBUG_PIPE") != nullptr;
  auto tnow = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double tp0 = dbgp ? tnow() : 0;
  if ((rc = pipe.settle())) return rc;
  HIPCHK(hipStreamSynchronize(g.cs_in));
  HIPCHK(hipStreamSynchronize(g.stream));  // (a piece enqueued ahead of a result that ended the loop)
  if (dbgp) fprintf(stderr, "zes pipe: loop done, settle+sync %.3f ms, np %u total %llu\n", tnow() - tp0, np, (unsigned long long)total);
  // every way out from here on is pipe.drain(): what has been sent has arrived when the caller has its answer
  if (!chain || !final_seen || total > dcap) return pipe.drain();  // not this way: the one-pass path decides
  *done = true;
  g.last_tier = 1;
  *out_len = total;
  if (alloc && !(early && out && total <= cap)) {  // the caller allocates the exact result now that its size is known (or: the early estimate fell short)
    if ((rc = pipe.drain())) return rc;
    const double ta = dbgp ? tnow() : 0;
    out = alloc(user, 0, total);
    if (!out) return ZES_E_ARG;
    const double tb = dbgp ? tnow() : 0;
    rc = download(out, d_out, total, g.cs_out, true);
    if (dbgp) fprintf(stderr, "zes pipe: alloc %.3f ms, download %.3f ms\n", tb - ta, tnow() - tb);
    return rc;
  }
  if (total > cap) return (rc = pipe.drain()) ? rc : ZES_E_NOSPACE;
  return pipe.drain(out, d_out, pend_lo, pend_hi);  // what is left to go down is the last piece (with an early estimate: it held)
}

static int inflate_host(const uint8_t* in, uint64_t c, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags,
                        bool size_only, zes_alloc_fn alloc, void* user) {
  if (!out_len || (!in && c)) return ZES_E_ARG;
  *out_len = 0;
  if (c == 0 || (in[0] & 15u) != 8u) return ZES_E_NOT_DEFLATE;  // src/zlib.ts:13-16, decided before the device is touched
  LOCK_READY();
  if (c >= PIPE_IN_MIN && c < (1ull << 29) && !size_only && (out || alloc) && !(flags & (ZES_F_NO_FASTPATH | ZES_F_PIECES | ZES_F_CHECK_ADLER)) &&
      !getenv("ZES_NO_PIPELINE")) {
    bool done = false;
    rc = inflate_host_pipelined(in, c, out, cap, out_len, flags, alloc, user, &done);
    if (rc || done) return rc;
    *out_len = 0;
  }
  if ((rc = stage_in(g.st_in, in, c))) return rc;
  uint64_t n = 0, eb = 0;
  rc = grow_and_retry(g.st_out, c, (size_only || alloc) ? 0 : cap, &n, [&](uint8_t* d_out, uint64_t dcap, uint64_t* m) {
    return inflate_one((const uint8_t*)g.st_in.p, 0, c, d_out, 0, dcap, m, flags, in[0], (flags & ZES_F_CHECK_ADLER) ? &eb : nullptr);
  });
  if (rc) return rc;
  if ((flags & ZES_F_CHECK_ADLER) && (rc = check_adler_trailer(in, nullptr, c, eb, (const uint8_t*)g.st_out.p, n))) return rc;
  *out_len = n;
  if (size_only) return ZES_OK;
  if (alloc) {  // the caller allocates the exact result now that its size is known; still under the lock
    out = alloc(user, 0, n);
    if (!out) return ZES_E_ARG;
    cap = n;
  }
  if (n > cap) return ZES_E_NOSPACE;
  return download(out, (const uint8_t*)g.st_out.p, n);
}

int zes_inflate(const uint8_t* in, uint64_t c, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  UseDev ud(route_host());
  return inflate_host(in, c, out, cap, out_len, flags, false, nullptr, nullptr);
}
int zes_inflate_size(const uint8_t* in, uint64_t c, uint64_t* n, uint32_t flags) {
  UseDev ud(route_host());
  return inflate_host(in, c, nullptr, 0, n, flags, true, nullptr, nullptr);
}
int zes_inflate_alloc(const uint8_t* in, uint64_t c, zes_alloc_fn alloc, void* user, uint64_t* out_len, uint32_t flags) {
  UseDev ud(route_host());
  if (!alloc) return ZES_E_ARG;
  return inflate_host(in, c, nullptr, 0, out_len, flags, false, alloc, user);
}

// ---- batch over host pointers: one arena up, the device batch, results down ----
// The trip of every form that takes host pointers, stated once (under the lock).  place() gives a piece of input its place in
// the pool that goes up, room() gives an output its place in the pool that the batch writes: the bytes and `slack` more
// behind them, from one 16-byte boundary to the next (16 for the container forms; 64, as stage_in leaves, for the plain
// batch forms, whose streams the decoders read some way past).  up() grows the pools and sends the placed pieces.  hand_out()
// takes every item still at ZES_OK to the caller's allocator, whose null answer is the item's ZES_E_ARG, and brings it down:
// out_len[i] is its size then, and 0 for every other item.
struct HostBatch {
  DevBuf &in, &out;
  const uint64_t slack;
  uint64_t tin = 0, tout = 0;
  struct Piece { uint64_t at; const uint8_t* p; uint64_t n; };  // (p null: the place alone)
  std::vector<Piece> pieces;
  HostBatch(DevBuf& in_, DevBuf& out_, uint64_t slack_ = 16) : in(in_), out(out_), slack(slack_) {}
  uint64_t place(const uint8_t* p, uint64_t n) {
    pieces.push_back(Piece{tin, p, n});
    tin += gz_up16(n) + slack;
    return pieces.back().at;
  }
  uint64_t room(uint64_t n) {
    const uint64_t at = tout;
    tout += gz_up16(n) + slack;
    return at;
  }
  int up() {  // (a form that asked for no room lays its outputs out itself)
    int rc;
    if ((rc = ensure(in, tin + 64)) || (tout && (rc = ensure(out, tout + 64)))) return rc;
    for (const Piece& q : pieces)
      if (q.p && (rc = upload((uint8_t*)in.p + q.at, q.p, q.n))) return rc;
    return ZES_OK;
  }
  const uint8_t* d_in() const { return (const uint8_t*)in.p; }
  uint8_t* d_out() const { return (uint8_t*)out.p; }
  int hand_out(uint32_t count, zes_alloc_fn alloc, void* user, int32_t* status, uint64_t* out_len, const std::function<uint64_t(uint32_t)>& size_of,
               const std::function<uint64_t(uint32_t)>& off_of) {
    int rc;
    for (uint32_t i = 0; i < count; i++) {
      if (status[i] != ZES_OK) {
        out_len[i] = 0;
        continue;
      }
      const uint64_t n = size_of(i);
      uint8_t* to = alloc(user, i, n);
      out_len[i] = to ? n : 0;
      if (!to) {
        status[i] = ZES_E_ARG;
        continue;
      }
      // (a short result is only enqueued: one synchronisation behind the loop serves them all)
      if ((rc = download(to, d_out() + off_of(i), n, nullptr, false))) return rc;
    }
    HIPCHK(hipStreamSynchronize(g.stream));
    return ZES_OK;
  }
};

static int deflate_batch_one(const uint8_t* const* in, const uint64_t* in_len, uint8_t* const* out, const uint64_t* out_cap,
                             uint64_t* out_len, int32_t* status, uint32_t count) {
  LOCK_READY();
  HostBatch hb(g.st_in, g.st_out, 64);
  std::vector<uint64_t> in_off(count), o_off(count), o_cap(count), dl(count);
  uint64_t tout = 0;
  for (uint32_t i = 0; i < count; i++) {
    if (!in[i] && in_len[i]) return ZES_E_ARG;
    in_off[i] = hb.place(deflate_throws(in_len[i]) ? nullptr : in[i], in_len[i]);
    o_off[i] = tout;
    o_cap[i] = deflate_bound(in_len[i]);
    tout += gz_up16(o_cap[i]);
  }
  if ((rc = hb.up()) || (rc = ensure(g.st_out, tout + 64))) return rc;
  rc = deflate_batch_core((const uint8_t*)g.st_in.p, in_off.data(), in_len, (uint8_t*)g.st_out.p, o_off.data(), o_cap.data(), dl.data(), status, count);
  if (rc) return rc;
  for (uint32_t i = 0; i < count; i++) {
    out_len[i] = dl[i];
    if (status[i]) continue;
    if (dl[i] > out_cap[i] || !out[i]) {
      status[i] = out[i] ? ZES_E_NOSPACE : ZES_E_ARG;
      continue;
    }
    if ((rc = download(out[i], (const uint8_t*)g.st_out.p + o_off[i], dl[i]))) return rc;
  }
  return ZES_OK;
}

static int inflate_batch_alloc_one(const uint8_t* const* in, const uint64_t* in_len, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                                   int32_t* status, uint32_t count, uint32_t flags) {
  LOCK_READY();
  HostBatch hb(g.st_in, g.st_out, 64);
  std::vector<uint64_t> in_off(count), o_off(count), o_cap(count);
  std::vector<uint8_t> firsts(count);
  const bool check = (flags & ZES_F_CHECK_ADLER) != 0;
  for (uint32_t i = 0; i < count; i++) {
    if (!in[i] && in_len[i]) return ZES_E_ARG;
    in_off[i] = hb.place(in[i], in_len[i]);
    firsts[i] = in_len[i] ? in[i][0] : 0;
    // first guess at the result size: a reference-made stream of c bytes rarely inflates beyond 4c; the retry below has exact sizes
    o_cap[i] = std::max<uint64_t>(in_len[i] * 4, 1 << 16);
    out_len[i] = 0;
    status[i] = ZES_OK;
  }
  if ((rc = hb.up())) return rc;
  std::vector<uint32_t> todo(count);
  for (uint32_t i = 0; i < count; i++) todo[i] = i;
  for (int attempt = 0; attempt < 8 && !todo.empty(); attempt++) {
    uint64_t tout = 0;
    std::vector<InfJob> jobs(todo.size());
    std::vector<uint8_t> fb(todo.size());
    std::vector<const uint8_t*> hin(todo.size());
    for (size_t k = 0; k < todo.size(); k++) {
      const uint32_t i = todo[k];
      o_off[i] = tout;
      tout += gz_up16(o_cap[i]);
      jobs[k] = InfJob{in_off[i], in_len[i], o_off[i], o_cap[i], 0, ZES_OK, 0};
      jobs[k].want_end = check;
      fb[k] = firsts[i];
      hin[k] = in[i];
    }
    if ((rc = ensure(g.st_out, tout + 64))) return rc;
    if ((rc = inflate_jobs((const uint8_t*)g.st_in.p, (uint8_t*)g.st_out.p, jobs, fb.data(), flags & ~ZES_F_CHECK_ADLER))) return rc;
    if (check) {  // the buffers that finished in this attempt, before any of them is handed out
      if ((rc = check_adler_jobs(nullptr, hin.data(), (const uint8_t*)g.st_out.p, jobs))) return rc;
    }
    std::vector<uint32_t> again;
    for (size_t k = 0; k < todo.size(); k++) {
      const uint32_t i = todo[k];
      out_len[i] = jobs[k].out_len;
      status[i] = jobs[k].status;
      if (jobs[k].status == ZES_E_NOSPACE && jobs[k].out_len > o_cap[i]) {
        o_cap[i] = jobs[k].out_len;
        again.push_back(i);
        continue;
      }
      if (jobs[k].status) continue;
      uint8_t* dst = alloc(user, i, jobs[k].out_len);
      if (!dst) {
        status[i] = ZES_E_ARG;
        continue;
      }
      if ((rc = download(dst, (const uint8_t*)g.st_out.p + o_off[i], jobs[k].out_len))) return rc;
    }
    todo.swap(again);
  }
  for (uint32_t i : todo) status[i] = ZES_E_DEVICE;
  return ZES_OK;
}

// ---- a host batch over every device the library drives ----
// Size-balanced owner lists: the longest buffers first, each onto the lightest part so far (ties: the lower index) —
// the rule of shard.partition, so that a Node batch and a torch.distributed job cut the same work the same way.
int zes_partition(const uint64_t* sizes, uint32_t count, uint32_t parts, uint32_t* owner) {
  if ((!sizes || !owner) && count) return ZES_E_ARG;
  if (parts == 0) return ZES_E_ARG;
  std::vector<uint32_t> order(count);
  for (uint32_t i = 0; i < count; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sizes[a] > sizes[b]; });
  std::vector<uint64_t> load(parts, 0);
  for (uint32_t i : order) {
    uint32_t best = 0;
    for (uint32_t r = 1; r < parts; r++)
      if (load[r] < load[best]) best = r;
    owner[i] = best;
    load[best] += sizes[i];
  }
  return ZES_OK;
}

int zes_device_count(void) {
  return g_nctx.load();
}

}  // extern "C"
// A host batch cut into one share per context (zes_partition by in_len).  Every non-empty share runs on its own thread
// bound to its context: fn(ids, in, in_len, out_len, status, m) with the share's own arrays — its buffer k is the
// caller's buffer ids[k] — whose out_len / status go back to the caller's places.  The first non-zero return wins.
template <class F>
static int over_devices(const uint8_t* const* in, const uint64_t* in_len, uint64_t* out_len, int32_t* status, uint32_t count, F fn) {
  const int n = g_nctx.load();
  std::vector<uint32_t> owner(count);
  int rc = zes_partition(in_len, count, (uint32_t)n, owner.data());
  if (rc) return rc;
  std::vector<std::vector<uint32_t>> ids((size_t)n);
  for (uint32_t i = 0; i < count; i++) ids[owner[i]].push_back(i);
  std::vector<int> rcs((size_t)n, ZES_OK);
  auto share = [&](int d) {
    UseDev ud(d);
    const std::vector<uint32_t>& id = ids[(size_t)d];
    const uint32_t m = (uint32_t)id.size();
    std::vector<const uint8_t*> sin(m);
    std::vector<uint64_t> slen(m), sol(m);
    std::vector<int32_t> sst(m);
    for (uint32_t k = 0; k < m; k++) {
      sin[k] = in[id[k]];
      slen[k] = in_len[id[k]];
    }
    if ((rcs[(size_t)d] = fn(id, sin.data(), slen.data(), sol.data(), sst.data(), m))) return;
    for (uint32_t k = 0; k < m; k++) {
      out_len[id[k]] = sol[k];
      status[id[k]] = sst[k];
    }
  };
  std::vector<std::thread> th;
  for (int d = 1; d < n; d++)
    if (!ids[(size_t)d].empty()) th.emplace_back(share, d);
  if (!ids[0].empty()) share(0);
  for (auto& t : th) t.join();
  for (int r : rcs)
    if (r) return r;
  return ZES_OK;
}
extern "C" {

int zes_deflate_batch(const uint8_t* const* in, const uint64_t* in_len, uint8_t* const* out, const uint64_t* out_cap,
                      uint64_t* out_len, int32_t* status, uint32_t count) {
  if (!in || !in_len || !out || !out_cap || !out_len || !status) return ZES_E_ARG;
  if (g_nctx.load() <= 1 || count <= 1 || t_routed) {
    UseDev ud(route_host());
    return deflate_batch_one(in, in_len, out, out_cap, out_len, status, count);
  }
  return over_devices(in, in_len, out_len, status, count,
                      [&](const std::vector<uint32_t>& ids, const uint8_t* const* sin, const uint64_t* slen, uint64_t* sol, int32_t* sst, uint32_t m) {
                        std::vector<uint8_t*> sout(m);
                        std::vector<uint64_t> scap(m);
                        for (uint32_t k = 0; k < m; k++) {
                          sout[k] = out[ids[k]];
                          scap[k] = out_cap[ids[k]];
                        }
                        return deflate_batch_one(sin, slen, sout.data(), scap.data(), sol, sst, m);
                      });
}

struct SubAlloc {  // a share's buffer k is the caller's buffer ids[k]
  zes_alloc_fn fn;
  void* user;
  const uint32_t* ids;
};
static uint8_t* sub_alloc(void* u, uint32_t k, uint64_t n) {
  const SubAlloc* a = static_cast<const SubAlloc*>(u);
  return a->fn(a->user, a->ids[k], n);
}

int zes_inflate_batch_alloc(const uint8_t* const* in, const uint64_t* in_len, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                            int32_t* status, uint32_t count, uint32_t flags) {
  if (!in || !in_len || !alloc || !out_len || !status) return ZES_E_ARG;
  if (g_nctx.load() <= 1 || count <= 1 || t_routed) {
    UseDev ud(route_host());
    return inflate_batch_alloc_one(in, in_len, alloc, user, out_len, status, count, flags);
  }
  return over_devices(in, in_len, out_len, status, count,
                      [&](const std::vector<uint32_t>& ids, const uint8_t* const* sin, const uint64_t* slen, uint64_t* sol, int32_t* sst, uint32_t m) {
                        SubAlloc sa{alloc, user, ids.data()};
                        return inflate_batch_alloc_one(sin, slen, sub_alloc, &sa, sol, sst, m, flags);
                      });
}

namespace {
int adler32_locked(const uint8_t* d_in, uint64_t n, uint32_t* adler_out) {
  int rc;
  if ((rc = ensure(g.adler, 16))) return rc;
  unsigned long long* acc = (unsigned long long*)g.adler.p;
  HIPCHK(hipMemsetAsync(acc, 0, 16, g.stream));
  if (n) {
    Timed t("k_adler");
    const uint32_t nch = (uint32_t)((n + ADLER_CHUNK - 1) / ADLER_CHUNK);
    hipLaunchKernelGGL(k_adler, dim3(nch), dim3(ADLER_THREADS), 0, g.stream, d_in, (uint64_t)0, n, acc);
  }
  HIPCHK(hipMemcpyAsync(g.pinned->adler, acc, 16, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  collect_times();
  const unsigned long long* h = g.pinned->adler;
  const uint32_t s1 = (uint32_t)((1ull + h[0]) % 65521ull);
  const uint32_t s2 = (uint32_t)((n % 65521ull + h[1]) % 65521ull);
  *adler_out = (s2 << 16) | s1;
  return ZES_OK;
}
}  // namespace

// ---- one buffer over several GPUs: block ranges and their join ----
int zes_deflate_range_dev(const uint8_t* d_in, uint64_t n, uint64_t n_readable, int final_range, uint8_t* d_out, uint64_t cap,
                          uint64_t* out_bits, uint32_t* adler) {
  ROUTE_DEV(d_in, d_out);
  if (!out_bits || !d_in || !d_out || n == 0 || n_readable < n) return ZES_E_ARG;
  if (!final_range && (n % ZES_BLK)) return ZES_E_ARG;  // only the input's last range may end inside a block
  if ((n % ZES_BLK) == 1) return ZES_E_CORRUPT;         // the reference throws on a 1-byte last block
  if ((((uintptr_t)d_in) & 15u) || (((uintptr_t)d_out) & 15u)) return ZES_E_ARG;
  LOCK_READY();
  uint64_t bits = 0;
  DeflateRange range{n_readable, ZES_BUF_RANGE | (final_range ? 0u : ZES_BUF_NOTFINAL)};
  rc = deflate_one(d_in, 0, n, d_out, 0, cap, &bits, &range);
  if (rc == ZES_OK || rc == ZES_E_NOSPACE) *out_bits = bits;  // (NOSPACE: the capacity needed, in bytes)
  if (rc) return rc;
  if (adler) *adler = range.adler;
  return ZES_OK;
}

int zes_deflate_join_dev(const uint8_t* const* d_piece, const uint64_t* piece_bits, const uint32_t* piece_adler, const uint64_t* piece_len,
                         uint32_t count, uint8_t* d_out, uint64_t cap, uint64_t* out_len) {
  ROUTE_DEV(d_out, (d_piece && count) ? d_piece[0] : nullptr);
  if (!d_piece || !piece_bits || !piece_adler || !piece_len || !d_out || !out_len || count == 0) return ZES_E_ARG;
  if (((uintptr_t)d_out) & 15u) return ZES_E_ARG;
  uint64_t bits = 0;
  AdlerJoin adler;
  for (uint32_t i = 0; i < count; i++) {
    if (piece_bits[i] && (!d_piece[i] || (((uintptr_t)d_piece[i]) & 3u))) return ZES_E_ARG;
    bits += piece_bits[i];
    adler.add(piece_adler[i], piece_len[i]);
  }
  const uint64_t raw_end = 2 + (bits + 7) / 8, total = raw_end + 4;
  *out_len = total;
  // the pieces are placed dword by dword: the kernel writes (and the memset clears) up to the dword that holds the
  // result's last byte, so the buffer must reach that far (include/zes.h says so; zes_deflate_bound always does)
  if (((total + 3) & ~3ull) > cap) return ZES_E_NOSPACE;
  LOCK_READY();
  HIPCHK(hipMemsetAsync(d_out, 0, (total + 3) & ~3ull, g.stream));
  uint64_t pos = 16;  // behind 78 9C
  for (uint32_t i = 0; i < count; i++) {
    if (!piece_bits[i]) continue;
    Timed t("k_bits_place");
    const uint64_t dwords = (piece_bits[i] + 63) / 32;
    const uint32_t nwg = (uint32_t)std::min<uint64_t>((dwords + 255) / 256, 4096);
    hipLaunchKernelGGL(k_bits_place, dim3(nwg), dim3(256), 0, g.stream, (uint32_t*)d_out, pos, (const uint32_t*)d_piece[i], piece_bits[i]);
    pos += piece_bits[i];
  }
  HIPCHK(hipGetLastError());
  uint8_t *head = g.pinned->head, *tail = g.pinned->tail;
  head[0] = 0x78;  // src/zlib.ts:29-34
  head[1] = 0x9C;
  put_be32(tail, adler.value());
  HIPCHK(hipMemcpyAsync(d_out, head, 2, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemcpyAsync(d_out + raw_end, tail, 4, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  collect_times();
  return ZES_OK;
}

int zes_inflate_range_dev(const uint8_t* d_in, uint64_t c, uint64_t lo_bit, uint64_t own_bit, int exact_start, uint8_t* d_out, uint64_t cap,
                          uint64_t* out_len, uint64_t* first_bit, uint64_t* end_bit, uint32_t* nblocks, int* final_block) {
  ROUTE_DEV(d_in, d_out);
  if (!d_in || !out_len || !first_bit || !end_bit || !nblocks || !final_block || lo_bit < 16 || own_bit <= lo_bit) return ZES_E_ARG;
  if ((((uintptr_t)d_in) & 15u) || (((uintptr_t)d_out) & 15u) || c >= (1ull << 29)) return ZES_E_ARG;
  LOCK_READY();
  RangeRes rr;
  if ((rc = inflate_t1_range(d_in, 0, c, lo_bit, own_bit, exact_start != 0, d_out, 0, cap, ZES_F_DEFAULT, &rr))) return rc;
  collect_times();
  if (!rr.handled) return ZES_E_NOTRANGE;
  *out_len = rr.out_len;
  *first_bit = rr.first_bit;
  *end_bit = rr.end_bit;
  *nblocks = rr.nblocks;
  *final_block = rr.final_block ? 1 : 0;
  return rr.out_len > cap ? ZES_E_NOSPACE : ZES_OK;
}

int zes_adler32_dev(const uint8_t* d_in, uint64_t n, uint32_t* adler_out) {
  ROUTE_DEV(d_in);
  if (!adler_out) return ZES_E_ARG;
  LOCK_READY();
  return adler32_locked(d_in, n, adler_out);
}

// ---- raw DEFLATE (src/deflate.ts:14, src/inflate.ts:16): thin forms over the wrapped pipeline ----
// The raw stream is decoded as the body of a zlib stream whose two header bytes are supplied here; it is
// copied device-to-device behind them so that the kernels keep their aligned dword view of the input.
// in_used (optional): on ZES_OK, the stream's bytes up to and including the one that holds its last bit
static int inflate_raw_staged(uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint32_t flags, uint64_t* in_used = nullptr) {
  HIPCHK(hipMemsetAsync(g.st_in.p, 0x78, 1, g.stream));
  HIPCHK(hipMemsetAsync((uint8_t*)g.st_in.p + 1, 0x9C, 1, g.stream));
  uint64_t eb = 0;
  const int rc = inflate_one((const uint8_t*)g.st_in.p, 0, n + 2, d_out, 0, cap, out_len, flags & ~ZES_F_CHECK_ADLER, 0x78, in_used ? &eb : nullptr);
  if (rc == ZES_OK && in_used) *in_used = eb >= 16 ? std::min<uint64_t>((eb - 16 + 7) / 8, n) : 0;
  return rc;
}

static int inflate_raw_dev_locked(const uint8_t* d_in, uint64_t c, uint64_t offset, uint8_t* d_out, uint64_t cap, uint64_t* out_len,
                                  uint64_t* in_used, uint32_t flags) {
  int rc;
  const uint64_t n = offset < c ? c - offset : 0;
  if ((rc = ensure(g.st_in, n + 2 + 64))) return rc;
  if (n) HIPCHK(hipMemcpyAsync((uint8_t*)g.st_in.p + 2, d_in + offset, n, hipMemcpyDeviceToDevice, g.stream));
  return inflate_raw_staged(n, d_out, cap, out_len, flags, in_used);
}

int zes_inflate_raw_used_dev(const uint8_t* d_in, uint64_t c, uint64_t offset, uint8_t* d_out, uint64_t cap, uint64_t* out_len,
                             uint64_t* in_used, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (!out_len || (!d_in && c)) return ZES_E_ARG;
  if ((((uintptr_t)d_out) & 15u)) return ZES_E_ARG;
  LOCK_READY();
  return inflate_raw_dev_locked(d_in, c, offset, d_out, cap, out_len, in_used, flags);
}

int zes_inflate_raw_dev(const uint8_t* d_in, uint64_t c, uint64_t offset, uint8_t* d_out, uint64_t cap, uint64_t* out_len,
                        uint32_t flags) {
  return zes_inflate_raw_used_dev(d_in, c, offset, d_out, cap, out_len, nullptr, flags);
}

int zes_inflate_raw(const uint8_t* in, uint64_t c, uint64_t offset, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  return zes_inflate_raw_used(in, c, offset, out, cap, out_len, nullptr, flags);
}

int zes_inflate_raw_used(const uint8_t* in, uint64_t c, uint64_t offset, uint8_t* out, uint64_t cap, uint64_t* out_len, uint64_t* in_used,
                         uint32_t flags) {
  UseDev ud(route_host());
  if (!out_len || (!in && c)) return ZES_E_ARG;
  *out_len = 0;
  LOCK_READY();
  const uint64_t n = offset < c ? c - offset : 0;
  if ((rc = stage_in(g.st_in, in + offset, n, 2))) return rc;
  uint64_t m = 0;
  rc = grow_and_retry(g.st_out, n, cap, &m, [&](uint8_t* d_out, uint64_t dcap, uint64_t* got) {
    return inflate_raw_staged(n, d_out, dcap, got, flags, in_used);
  });
  if (rc) return rc;
  *out_len = m;
  if (m > cap) return ZES_E_NOSPACE;
  return download(out, (const uint8_t*)g.st_out.p, m);
}

static int deflate_raw_common(const uint8_t* d_in, uint64_t n, uint64_t* raw_len) {
  const uint64_t bound = deflate_bound(n);
  int rc;
  if ((rc = ensure(g.st_out, bound + 64))) return rc;
  uint64_t dl = 0;
  if ((rc = deflate_one(d_in, 0, n, (uint8_t*)g.st_out.p, 0, bound, &dl))) return rc;
  *raw_len = dl - 6;  // without 78 9C and the Adler-32 trailer (src/zlib.ts:28-46)
  return ZES_OK;
}

int zes_deflate_raw_dev(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len) {
  ROUTE_DEV(d_in, d_out);
  if (!out_len || !d_out) return ZES_E_ARG;
  *out_len = 0;
  if (deflate_throws(n)) return ZES_E_CORRUPT;
  LOCK_READY();
  uint64_t rl = 0;
  if ((rc = deflate_raw_common(d_in, n, &rl))) return rc;
  *out_len = rl;
  if (rl > cap) return ZES_E_NOSPACE;
  HIPCHK(hipMemcpyAsync(d_out, (const uint8_t*)g.st_out.p + 2, rl, hipMemcpyDeviceToDevice, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return ZES_OK;
}

int zes_deflate_raw(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  UseDev ud(route_host());
  if (!out_len || (!in && n) || !out) return ZES_E_ARG;
  *out_len = 0;
  if (deflate_throws(n)) return ZES_E_CORRUPT;
  LOCK_READY();
  if ((rc = stage_in(g.st_in, in, n))) return rc;
  uint64_t rl = 0;
  if ((rc = deflate_raw_common((const uint8_t*)g.st_in.p, n, &rl))) return rc;
  *out_len = rl;
  if (rl > cap) return ZES_E_NOSPACE;
  return download(out, (const uint8_t*)g.st_out.p + 2, rl);
}

int zes_adler32(const uint8_t* in, uint64_t n, uint32_t* adler_out) {
  UseDev ud(route_host());
  if (!adler_out || (!in && n)) return ZES_E_ARG;
  LOCK_READY();  // staging and kernel under one lock: nobody else's call can replace st_in in between
  if ((rc = stage_in(g.st_in, in, n))) return rc;
  return adler32_locked((const uint8_t*)g.st_in.p, n, adler_out);
}

// ---- CRC-32 (zes_crc.hip) ----
// the kernel's table, holding the chunk powers an n-byte input needs
static int crc_ready(uint64_t n) {
  const uint64_t nch = (n + CRC_CHUNK - 1) / CRC_CHUNK;
  if (nch >= (1ull << 31)) return ZES_E_ARG;
  const uint32_t need = (uint32_t)std::max<uint64_t>(nch, 2) - 1;
  if (g.crctab.p && g.crc_npow >= need) return ZES_OK;
  uint32_t npow = std::max<uint32_t>(1024, g.crctab.p ? g.crc_npow : 0);
  while (npow < need) npow *= 2;
  std::vector<uint32_t> tab(CRC_TAB_POW + npow);
  zes_crc_tables(tab.data(), npow);
  HIPCHK(hipStreamSynchronize(g.stream));  // (a launch may still read the table being replaced)
  HIPCHK(hipStreamSynchronize(g.s_adler));
  int rc;
  if ((rc = ensure(g.crctab, tab.size() * 4))) return rc;
  HIPCHK(hipMemcpy(g.crctab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  g.crc_npow = npow;
  return ZES_OK;
}

// k_crc32 over d[0, n) on `st`, the two accumulator words on their way to the area's crc; crc_finish() once st is synchronised
static int crc_enqueue(const uint8_t* d, uint64_t n, hipStream_t st) {
  int rc;
  if ((rc = crc_ready(n))) return rc;
  if ((rc = ensure(g.crcacc, 16))) return rc;
  HIPCHK(hipMemsetAsync(g.crcacc.p, 0, 8, st));
  if (n) {
    Timed t("k_crc32", st);
    hipLaunchKernelGGL(k_crc32, dim3((uint32_t)((n + CRC_CHUNK - 1) / CRC_CHUNK)), dim3(CRC_THREADS), 0, st, d, n, (const uint32_t*)g.crctab.p,
                       (unsigned int*)g.crcacc.p);
  }
  HIPCHK(hipMemcpyAsync(g.pinned->crc, g.crcacc.p, 8, hipMemcpyDeviceToHost, st));
  return ZES_OK;
}

// word 0 holds the chunks before the last one, shifted to the last chunk's start; word 1 the last chunk
static uint32_t crc_finish(uint64_t n) {
  const uint32_t* a = g.pinned->crc;
  const uint64_t last = n ? n - ((n - 1) / CRC_CHUNK) * CRC_CHUNK : 0;
  const uint32_t raw = zes_crc_shift(a[0], last) ^ a[1];
  return raw ^ zes_crc_shift(0xFFFFFFFFu, n) ^ 0xFFFFFFFFu;
}

static int crc32_locked(const uint8_t* d, uint64_t n, uint32_t* crc) {
  int rc;
  if ((rc = crc_enqueue(d, n, g.stream))) return rc;
  HIPCHK(hipStreamSynchronize(g.stream));
  *crc = crc_finish(n);
  return ZES_OK;
}

int zes_crc32_dev(const uint8_t* d_in, uint64_t n, uint32_t* crc) {
  ROUTE_DEV(d_in);
  if (!crc || (!d_in && n)) return ZES_E_ARG;
  LOCK_READY();
  rc = crc32_locked(d_in, n, crc);
  collect_times();
  return rc;
}

int zes_crc32(const uint8_t* in, uint64_t n, uint32_t* crc) {
  UseDev ud(route_host());
  if (!crc || (!in && n)) return ZES_E_ARG;
  LOCK_READY();
  if ((rc = stage_in(g.st_in, in, n))) return rc;
  rc = crc32_locked((const uint8_t*)g.st_in.p, n, crc);
  collect_times();
  return rc;
}

}  // extern "C" (a template has C++ linkage)
// ---- segmented checksums (k_crc32_seg, k_adler_seg) ----
// out[i] = the checksum of d[segs[i].off, + segs[i].len) for all i, in one launch and one read-back.  The work items are
// (buffer, 64 KiB chunk of memory) pairs, listed here from the lengths exactly as the kernel cuts a buffer; the kernel leaves
// two accumulator words per buffer, finished here.  The pool holds segs | work | acc.  What differs between the checksums
// is in the description S:
//   Word, EMPTY, NAME  an accumulator word, the checksum of no bytes, the launch's name in the times
//   pool()             the pool
//   chunks(a, end)     the work items of a buffer at the addresses [a, end), a < end
//   ready(maxlen)      what the launch needs beside the pool, for buffers of up to maxlen bytes
//   launch(...)        the kernel over `items` work items
//   finish(a, end, w)  the buffer's checksum from its two words
namespace {
// The front half: the work list, the pool, the uploads and the launch.  *d_acc: the accumulator words on the device, two per
// buffer, or null when no buffer has bytes (no launch).  `work` is read by an upload: it lives until the stream has passed it.
template <class S>
int seg_checksum_enqueue(S& ck, const uint8_t* d, const ZesCrcSeg* segs, uint32_t count, std::vector<uint2>& work, typename S::Word** d_acc) {
  using Word = typename S::Word;
  int rc;
  *d_acc = nullptr;
  work.clear();  // (buffer, chunk)
  work.reserve(count);
  uint64_t maxlen = 0;
  for (uint32_t i = 0; i < count; i++) {
    if (!segs[i].len) continue;
    const uint64_t a = (uint64_t)(uintptr_t)d + segs[i].off, nch = S::chunks(a, a + segs[i].len);
    if (work.size() + nch >= (1ull << 31)) return ZES_E_ARG;
    for (uint64_t j = 0; j < nch; j++) work.push_back(make_uint2(i, (uint32_t)j));
    maxlen = std::max(maxlen, segs[i].len);
  }
  if (work.empty()) return ZES_OK;
  if ((rc = ck.ready(maxlen))) return rc;
  const size_t o_work = sizeof(ZesCrcSeg) * (size_t)count, o_acc = o_work + sizeof(uint2) * work.size(), n_acc = 2 * sizeof(Word) * (size_t)count;
  if ((rc = ensure(S::pool(), o_acc + n_acc))) return rc;
  uint8_t* base = (uint8_t*)S::pool().p;
  HIPCHK(hipMemcpyAsync(base, segs, o_work, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemcpyAsync(base + o_work, work.data(), sizeof(uint2) * work.size(), hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemsetAsync(base + o_acc, 0, n_acc, g.stream));
  {
    Timed t(S::NAME);
    ck.launch((uint32_t)work.size(), d, (const ZesCrcSeg*)base, (const uint2*)(base + o_work), (Word*)(base + o_acc));
  }
  HIPCHK(hipGetLastError());
  *d_acc = (Word*)(base + o_acc);
  return ZES_OK;
}

template <class S>
int seg_checksum_locked(S ck, const uint8_t* d, const ZesCrcSeg* segs, uint32_t count, uint32_t* out) {
  using Word = typename S::Word;
  int rc;
  for (uint32_t i = 0; i < count; i++) out[i] = S::EMPTY;
  std::vector<uint2> work;
  Word* d_acc = nullptr;
  if ((rc = seg_checksum_enqueue(ck, d, segs, count, work, &d_acc))) return rc;
  if (!d_acc) return ZES_OK;
  std::vector<Word> acc(2 * (size_t)count);
  HIPCHK(hipMemcpyAsync(acc.data(), d_acc, sizeof(Word) * acc.size(), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  for (uint32_t i = 0; i < count; i++) {
    if (!segs[i].len) continue;
    const uint64_t a = (uint64_t)(uintptr_t)d + segs[i].off;
    out[i] = ck.finish(a, a + segs[i].len, &acc[2 * (size_t)i]);
  }
  return ZES_OK;
}

// CRC-32: chunk j of a buffer holds [max(a, A + 64Ki * j), min(E, A + 64Ki * (j + 1))), A = a rounded down to 16, E = the end
// rounded down to 16 (a, when that lies in front of a), the last one also [E, end): at least one item.  Word 0 is shifted
// by the last item's bytes (two GF(2) multiplies per buffer; the powers are kept per length, a batch of BGZF members has
// two or three different ones).
struct CrcSeg {
  using Word = unsigned int;
  static constexpr uint32_t EMPTY = 0;
  static constexpr const char* NAME = "k_crc32_seg";
  static DevBuf& pool() { return g.crcseg; }
  static uint64_t chunks(uint64_t a, uint64_t end) {
    const uint64_t A = a & ~(uint64_t)15, E = std::max<uint64_t>(end & ~(uint64_t)15, a);
    return E > a ? (E - A + CRC_CHUNK - 1) / CRC_CHUNK : 1;
  }
  int ready(uint64_t maxlen) { return crc_ready(maxlen + 2 * CRC_CHUNK); }
  void launch(uint32_t items, const uint8_t* d, const ZesCrcSeg* segs, const uint2* work, Word* acc) {
    hipLaunchKernelGGL(k_crc32_seg, dim3(items), dim3(CRC_THREADS), 0, g.stream, d, segs, work, (const uint32_t*)g.crctab.p, acc);
  }
  std::map<uint64_t, uint32_t> pw;  // x^(8k)
  uint32_t shift(uint32_t v, uint64_t k) {
    auto it = pw.find(k);
    if (it == pw.end()) it = pw.emplace(k, zes_crc_shift(0x80000000u, k)).first;
    return zes_crc_mul(it->second, v);
  }
  uint32_t finish(uint64_t a, uint64_t end, const Word* w) {
    const ZesCrcPut p = put(a, end, 0);
    return zes_crc_mul(p.mul, w[0]) ^ w[1] ^ p.add;
  }
  // finish() for the device (k_crc32_put): the two constants, which depend on where the buffer lies and on its length alone
  ZesCrcPut put(uint64_t a, uint64_t end, uint64_t dst) {
    const uint64_t last = end - std::max<uint64_t>(a, (a & ~(uint64_t)15) + (chunks(a, end) - 1) * CRC_CHUNK);
    return ZesCrcPut{dst, shift(0x80000000u, last), shift(0xFFFFFFFFu, end - a) ^ 0xFFFFFFFFu};
  }
};

// Adler-32: chunk j holds the bytes of [a, end) inside [G + 64Ki * j, G + 64Ki * (j + 1)), G = a rounded down to 16; the two
// sums are finished as k_layout finishes k_adler's.
struct AdlerSeg {
  using Word = unsigned long long;
  static constexpr uint32_t EMPTY = 1;
  static constexpr const char* NAME = "k_adler_seg";
  static DevBuf& pool() { return g.adlerseg; }
  static uint64_t chunks(uint64_t a, uint64_t end) { return (((end + 15) & ~(uint64_t)15) - (a & ~(uint64_t)15) + ADLER_CHUNK - 1) / ADLER_CHUNK; }
  int ready(uint64_t) { return ZES_OK; }
  void launch(uint32_t items, const uint8_t* d, const ZesCrcSeg* segs, const uint2* work, Word* acc) {
    hipLaunchKernelGGL(k_adler_seg, dim3(items), dim3(ADLER_THREADS), 0, g.stream, d, segs, work, acc);
  }
  uint32_t finish(uint64_t a, uint64_t end, const Word* w) {
    const uint32_t s1 = (uint32_t)((1ull + w[0]) % 65521ull), s2 = (uint32_t)(((end - a) % 65521ull + w[1]) % 65521ull);
    return (s2 << 16) | s1;
  }
};

int crc32_batch_locked(const uint8_t* d, const ZesCrcSeg* segs, uint32_t count, uint32_t* crc) {
  return seg_checksum_locked(CrcSeg(), d, segs, count, crc);
}

int adler32_batch_locked(const uint8_t* d, const ZesCrcSeg* segs, uint32_t count, uint32_t* adler) {
  return seg_checksum_locked(AdlerSeg(), d, segs, count, adler);
}
}  // namespace
extern "C" {

// zes_crc32_batch_dev, zes_adler32_batch_dev: the argument checks, the buffers as ZesCrcSeg, the call's times
static int checksum_batch_dev(int (*batch)(const uint8_t*, const ZesCrcSeg*, uint32_t, uint32_t*), const uint8_t* d_in, const uint64_t* off,
                              const uint64_t* len, uint32_t* out, uint32_t count) {
  ROUTE_DEV(d_in);
  if (count && (!off || !len || !out)) return ZES_E_ARG;
  LOCK_READY();
  std::vector<ZesCrcSeg> segs(count);
  for (uint32_t i = 0; i < count; i++) {
    if (len[i] && !d_in) return ZES_E_ARG;
    segs[i] = ZesCrcSeg{off[i], len[i]};
  }
  rc = batch(d_in, segs.data(), count, out);
  collect_times();
  return rc;
}

int zes_crc32_batch_dev(const uint8_t* d_in, const uint64_t* off, const uint64_t* len, uint32_t* crc, uint32_t count) {
  return checksum_batch_dev(crc32_batch_locked, d_in, off, len, crc, count);
}

int zes_adler32_batch_dev(const uint8_t* d_in, const uint64_t* off, const uint64_t* len, uint32_t* adler, uint32_t count) {
  return checksum_batch_dev(adler32_batch_locked, d_in, off, len, adler, count);
}

// ---- gzip writer (RFC 1952): fixed header | zes_deflate_raw's bytes | CRC-32, ISIZE ----
static const uint8_t kGzHeader[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};  // FLG 0, MTIME 0, XFL 0, OS 255
static uint64_t gzip_bound(uint64_t n) { return deflate_bound(n) - 6 + 18; }

// the body into g.st_out + 2 (as zes_deflate_raw does); the input's CRC-32 runs on the second stream beside the deflate
// kernels, as the Adler-32 pass does
static int gzip_core(const uint8_t* d_in, uint64_t n, uint64_t* raw_len, uint32_t* crc) {
  int rc;
  HIPCHK(hipEventRecord(g.ev_a0, g.stream));  // (behind the upload of a host call)
  HIPCHK(hipStreamWaitEvent(g.s_adler, g.ev_a0, 0));
  if ((rc = crc_enqueue(d_in, n, g.s_adler))) return rc;
  rc = deflate_raw_common(d_in, n, raw_len);
  HIPCHK(hipStreamSynchronize(g.s_adler));
  if (rc) return rc;
  *crc = crc_finish(n);
  return ZES_OK;
}

int zes_gzip_bound(uint64_t n, uint64_t* cap) {
  if (!cap) return ZES_E_ARG;
  *cap = gzip_bound(n);
  return ZES_OK;
}

int zes_gzip_dev(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len) {
  ROUTE_DEV(d_in, d_out);
  if (!out_len || !d_out || (!d_in && n)) return ZES_E_ARG;
  *out_len = 0;
  if (deflate_throws(n)) return ZES_E_CORRUPT;
  if (((uintptr_t)d_out) & 15u) return ZES_E_ARG;
  LOCK_READY();
  uint64_t rl = 0;
  uint32_t crc = 0;
  if ((rc = gzip_core(d_in, n, &rl, &crc))) return rc;
  *out_len = rl + 18;
  if (rl + 18 > cap) return ZES_E_NOSPACE;
  memcpy(g.pinned->head, kGzHeader, 10);
  put_le32(g.pinned->tail, crc);
  put_le32(g.pinned->tail + 4, (uint32_t)n);
  HIPCHK(hipMemcpyAsync(d_out + 10, (const uint8_t*)g.st_out.p + 2, rl, hipMemcpyDeviceToDevice, g.stream));
  HIPCHK(hipMemcpyAsync(d_out, g.pinned->head, 10, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemcpyAsync(d_out + 10 + rl, g.pinned->tail, 8, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return ZES_OK;
}

int zes_gzip(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  UseDev ud(route_host());
  if (!out_len || (!in && n) || !out) return ZES_E_ARG;
  *out_len = 0;
  if (deflate_throws(n)) return ZES_E_CORRUPT;
  LOCK_READY();
  if ((rc = stage_in(g.st_in, in, n))) return rc;
  uint64_t rl = 0;
  uint32_t crc = 0;
  if ((rc = gzip_core((const uint8_t*)g.st_in.p, n, &rl, &crc))) return rc;
  *out_len = rl + 18;
  if (rl + 18 > cap) return ZES_E_NOSPACE;
  memcpy(out, kGzHeader, 10);
  if ((rc = download(out + 10, (const uint8_t*)g.st_out.p + 2, rl))) return rc;
  put_le32(out + 10 + rl, crc);
  put_le32(out + 14 + rl, (uint32_t)n);
  return ZES_OK;
}

// The end of a container call's device work (zes_bgzip*, zes_bgzf_read*, zes_zip_read*, zes_zipwrite*): with `clear`, a call
// that failed leaves no HIP error behind for the next one; the call's times are collected either way.
static int call_done(int rc, bool clear) {
  if (rc && clear) (void)hipGetLastError();
  collect_times();
  return rc;
}

// ---- A group of buffers encoded for a container: the step that bgzip_core (members), zipwrite_core (entries) and
// pngwrite_core (images) share ----
// Buffer k of a group is d_in[in_off[k], + in_len[k]) and has the 16-byte aligned slot [o_off[k], + o_cap[k]) of g.gz_bodies,
// o_cap[k] == 0 for a buffer that the encoder is spared; the slots take `slots` bytes.  form() lays a group out by the
// writers' rule; bgzip_core, whose chunks have one fixed slot, fills the three itself.  encode() gives every buffer its
// CRC-32 by one segmented launch (unless the caller has no use for them: crcs) and encodes the group by one deflate_batch_core call (none when the slots take no bytes: no
// times of its own to keep); raw[k] is then the length of buffer k's raw stream, which starts at o_off[k] + 2 (78 9C in
// front, the Adler-32 behind), and 0 for a spared buffer.
// A result beyond the caller's capacity, by room(): every group is still encoded (the size needed is the answer), and from
// the first group that does not fit whole nothing more is written.
constexpr uint32_t ENC_GROUP = 1024;                     // buffers encoded at once: a block's scratch each, what zes_deflate_dev pools for 128 MiB ...
constexpr uint32_t ENC_GROUP_PIECES = 4;                 // ... under ZES_F_PIECES
constexpr uint64_t ENC_GROUP_SLOTS = 256ull << 20;       // ... and the bytes of their encoder slots (1024 buffers of up to 64 KiB take half of it)
constexpr uint64_t ENC_GROUP_SLOTS_PIECES = 1ull << 20;  // ... under ZES_F_PIECES: two buffers of 300000 bytes do not share a group
static_assert(ENC_GROUP <= DEFLATE_TABLE_BUFS && ENC_GROUP <= DEFLATE_DIRECT_BUFS, "a group's buffer table and results go through the page-locked area");
struct EncGroup {
  const uint32_t group;
  const uint64_t group_slots;
  std::vector<uint64_t> o_off, o_cap, o_len, raw;
  std::vector<int32_t> status;
  std::vector<ZesCrcSeg> csegs;
  std::vector<uint32_t> crc;
  bool fits = true;
  // for a call of `items` buffers in all
  EncGroup(uint32_t flags, uint64_t items)
      : group((flags & ZES_F_PIECES) ? ENC_GROUP_PIECES : ENC_GROUP), group_slots((flags & ZES_F_PIECES) ? ENC_GROUP_SLOTS_PIECES : ENC_GROUP_SLOTS),
        o_off((size_t)std::min<uint64_t>(group, items)), o_cap(o_off.size()), o_len(o_off.size()), raw(o_off.size()), status(o_off.size()),
        csegs(o_off.size()), crc(o_off.size()) {}
  // The next group of the buffers whose lengths are len[0, left): up to `group` of them whose encoder slots take up to
  // group_slots bytes, and one at least; a length that the encoder refuses has no slot.  Returns how many it takes, and
  // *slots: the bytes of their slots, for encode().
  uint32_t form(const uint64_t* len, uint64_t left, uint64_t* slots) {
    uint32_t cnt = 0;
    for (*slots = 0; cnt < left && cnt < group; cnt++) {
      const uint64_t slot = deflate_throws(len[cnt]) ? 0 : gz_up16(deflate_bound(len[cnt]));
      if (cnt && *slots + slot > group_slots) break;
      o_off[cnt] = *slots;
      *slots += o_cap[cnt] = slot;
    }
    return cnt;
  }
  int encode(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t cnt, uint64_t slots, bool crcs = true) {
    int rc;
    for (uint32_t k = 0; k < cnt; k++) csegs[k] = ZesCrcSeg{in_off[k], in_len[k]};
    if ((rc = ensure(g.gz_bodies, slots + 64))) return rc;
    if (crcs && (rc = crc32_batch_locked(d_in, csegs.data(), cnt, crc.data()))) return rc;
    if (slots) {
      if ((rc = deflate_batch_core(d_in, in_off, in_len, (uint8_t*)g.gz_bodies.p, o_off.data(), o_cap.data(), o_len.data(), status.data(), cnt))) return rc;
      keep_times();
    }
    for (uint32_t k = 0; k < cnt; k++) {
      if (o_cap[k] && (status[k] != ZES_OK || o_len[k] < 6)) return status[k] ? status[k] : ZES_E_DEVICE;
      raw[k] = o_cap[k] ? o_len[k] - 6 : 0;  // without 78 9C and the Adler-32
    }
    return ZES_OK;
  }
  bool room(uint64_t total, uint64_t cap, const uint8_t* d_out) { return fits = fits && total <= cap && d_out != nullptr; }
};

// ---- BGZF writer: the input in chunks of ZES_BGZF_CHUNK bytes, a gzip member each, and the end-of-file marker ----
static const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
constexpr uint64_t BGZF_MEMBER_MAX = ZES_BGZF_HLEN + 5 + ZES_BGZF_CHUNK + 8;  // a full chunk as a stored block: 65311
constexpr uint64_t BGZF_N_MAX = 1ull << 62;  // (the bound of a longer input does not fit 64 bits)
static_assert(BGZF_MEMBER_MAX <= 65536, "BSIZE has 16 bits");
static uint64_t bgzip_members(uint64_t n) { return (n + ZES_BGZF_CHUNK - 1) / ZES_BGZF_CHUNK + 1; }
static uint64_t bgzip_bound(uint64_t n) {
  const uint64_t tail = n % ZES_BGZF_CHUNK;
  return n / ZES_BGZF_CHUNK * BGZF_MEMBER_MAX + (tail ? tail + ZES_BGZF_HLEN + 5 + 8 : 0) + sizeof kBgzfEof;
}

// The members of d_in[0, n) and the marker into d_out[0, cap), group by group (EncGroup, ENC_GROUP members or ENC_GROUP_PIECES):
// every chunk has a slot of its own size class, a chunk of one byte, which the encoder refuses, is spared, and the call is made whenever the group has members.
// The sizes come back, the host chooses stream or stored block per member and k_bgzf_pack puts the members in their places.
// The marker is the last launch's last record.  A result beyond cap: EncGroup's rule.  member_off: null, or where every
// member starts, the marker's last.
static int bgzip_core(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint64_t* member_off, uint32_t flags) {
  int rc;
  g.carry.clear();
  const uint64_t nm = bgzip_members(n) - 1;  // (without the marker)
  const uint64_t slot = gz_up16(deflate_bound(ZES_BGZF_CHUNK));
  std::vector<ZesBgzfRec> recs((size_t)nm + 1);  // (of the whole call: uploads read it until the last synchronisation)
  EncGroup eg(flags, nm);
  const uint64_t group = eg.group;
  std::vector<uint64_t> in_off(eg.o_off.size()), in_len(eg.o_off.size());
  Drain drain;  // (behind recs, eg and the group's tables)
  uint64_t total = 0;
  for (uint64_t m0 = 0;; m0 += group) {
    const uint32_t cnt = (uint32_t)std::min(group, nm - m0);
    const bool last = m0 + cnt == nm;
    for (uint32_t k = 0; k < cnt; k++) {
      in_off[k] = (m0 + k) * ZES_BGZF_CHUNK;
      in_len[k] = std::min<uint64_t>(ZES_BGZF_CHUNK, n - in_off[k]);
      eg.o_off[k] = k * slot;
      eg.o_cap[k] = in_len[k] == 1 ? 0 : slot;
    }
    if (cnt && (rc = eg.encode(d_in, in_off.data(), in_len.data(), cnt, cnt * slot))) return rc;
    for (uint32_t k = 0; k < cnt; k++) {
      const uint32_t len = (uint32_t)in_len[k];
      const bool stored = len == 1 || eg.raw[k] > (uint64_t)len + 5;
      ZesBgzfRec& r = recs[(size_t)(m0 + k)];
      r.src_off = stored ? in_off[k] : eg.o_off[k] + 2;
      r.dst_off = total;
      r.body_len = stored ? len + 5 : (uint32_t)eg.raw[k];
      r.len = len;
      r.crc = eg.crc[k];
      r.kind = stored ? ZES_BGZF_STORED : ZES_BGZF_STREAM;
      total += ZES_BGZF_HLEN + r.body_len + 8;
    }
    if (last) {
      recs[(size_t)nm] = ZesBgzfRec{0, total, 2, 0, 0, ZES_BGZF_EOF};
      total += sizeof kBgzfEof;
    }
    const uint32_t nrec = cnt + (last ? 1u : 0u);
    if (eg.room(total, cap, d_out)) {
      if ((rc = ensure(g.gz_tab, sizeof(ZesBgzfRec) * (size_t)nrec))) return rc;
      HIPCHK(hipMemcpyAsync(g.gz_tab.p, &recs[(size_t)m0], sizeof(ZesBgzfRec) * (size_t)nrec, hipMemcpyHostToDevice, g.stream));
      Timed t("k_bgzf_pack");
      hipLaunchKernelGGL(k_bgzf_pack, dim3(nrec), dim3(GZ_GATHER_THREADS), 0, g.stream, d_in, (const uint8_t*)g.gz_bodies.p, d_out,
                         (const ZesBgzfRec*)g.gz_tab.p);
    }
    HIPCHK(hipGetLastError());
    if (last) break;
  }
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  if (member_off)
    for (uint64_t k = 0; k <= nm; k++) member_off[k] = recs[(size_t)k].dst_off;
  *out_len = total;
  return eg.fits ? ZES_OK : ZES_E_NOSPACE;
}

int zes_bgzip_members(uint64_t n, uint64_t* members) {
  if (!members) return ZES_E_ARG;
  *members = bgzip_members(n);
  return ZES_OK;
}

int zes_bgzip_bound(uint64_t n, uint64_t* cap) {
  if (!cap || n > BGZF_N_MAX) return ZES_E_ARG;
  *cap = bgzip_bound(n);
  return ZES_OK;
}

int zes_bgzip_dev(const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint64_t* member_off, uint32_t flags) {
  ROUTE_DEV(d_out, d_in);
  if (!out_len || (n && (!d_in || !d_out)) || (!d_out && cap) || (flags & ~ZES_F_PIECES) || n > BGZF_N_MAX) return ZES_E_ARG;
  *out_len = 0;
  LOCK_READY();
  return call_done(bgzip_core(d_in, n, d_out, cap, out_len, member_off, flags), false);
}

int zes_bgzip(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len, uint64_t* member_off, uint32_t flags) {
  UseDev ud(route_host());
  if (!out_len || (n && (!in || !out)) || (!out && cap) || (flags & ~ZES_F_PIECES) || n > BGZF_N_MAX) return ZES_E_ARG;
  *out_len = 0;
  if (n == 0) {  // the marker alone: nothing to compute
    *out_len = sizeof kBgzfEof;
    if (member_off) member_off[0] = 0;
    if (cap < sizeof kBgzfEof) return ZES_E_NOSPACE;
    memcpy(out, kBgzfEof, sizeof kBgzfEof);
    return ZES_OK;
  }
  LOCK_READY();
  if ((rc = stage_in(g.gz_in, in, n))) return rc;
  const uint64_t bound = bgzip_bound(n);
  if ((rc = ensure(g.gz_acc, bound + 64))) return rc;
  uint64_t total = 0;
  if ((rc = call_done(bgzip_core((const uint8_t*)g.gz_in.p, n, (uint8_t*)g.gz_acc.p, bound, &total, member_off, flags), false))) return rc;
  *out_len = total;
  if (total > cap) return ZES_E_NOSPACE;
  return download(out, (const uint8_t*)g.gz_acc.p, total);
}

// ---- gzip reader (RFC 1952; CPython's gzip.decompress) ----
// One member's header in h[0, avail) (left = input bytes from its start): ZES_OK and *hlen, ZES_E_GZIP / ZES_E_CHECKSUM,
// or 1: the header goes on behind `avail` (bring more bytes)
static int gz_header(const uint8_t* h, uint64_t avail, uint64_t left, uint64_t* hlen) {
  auto need = [&](uint64_t k) { return k <= avail ? 0 : (avail < left ? 1 : (int)ZES_E_GZIP); };
  int r;
  if ((r = need(10))) return r;
  if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0xE0u)) return ZES_E_GZIP;  // (reserved FLG bits: rejected, as zlib does)
  const uint8_t flg = h[3];
  uint64_t p = 10;
  if (flg & 4u) {  // FEXTRA
    if ((r = need(p + 2))) return r;
    p += 2 + ((uint64_t)h[p] | (uint64_t)h[p + 1] << 8);
    if ((r = need(p))) return r;
  }
  for (uint32_t f = 8; f <= 16; f <<= 1)  // FNAME, FCOMMENT: zero-terminated
    if (flg & f)
      for (;;) {
        if ((r = need(p + 1))) return r;
        if (h[p++] == 0) break;
      }
  if (flg & 2u) {  // FHCRC: the low 16 bits of the header's CRC-32
    if ((r = need(p + 2))) return r;
    if ((zes_crc_host(h, p) & 0xFFFFu) != ((uint32_t)h[p] | (uint32_t)h[p + 1] << 8)) return ZES_E_CHECKSUM;
    p += 2;
  }
  *hlen = p;
  return ZES_OK;
}

// the input as the host sees it: the caller's memory (host forms), or pieces copied down from the device
struct GzSrc {
  const uint8_t* h;
  const uint8_t* d;  // the input on the device
  uint64_t c;
  std::vector<uint8_t> win;
  uint64_t win_pos = 0;
  int get(uint64_t pos, uint64_t k, const uint8_t** out) {  // bytes [pos, pos + k), k <= c - pos
    if (h) {
      *out = h + pos;
      return ZES_OK;
    }
    if (pos < win_pos || pos + k > win_pos + win.size()) {
      const uint64_t len = std::min<uint64_t>(c - pos, std::max<uint64_t>(k, 4096));
      win.resize(len);
      if (len) HIPCHK(hipMemcpy(win.data(), d + pos, len, hipMemcpyDeviceToHost));
      win_pos = pos;
    }
    *out = win.data() + (pos - win_pos);
    return ZES_OK;
  }
  int header(uint64_t pos, uint64_t* hlen) {
    for (uint64_t k = std::min<uint64_t>(c - pos, 4096);; k = std::min<uint64_t>(c - pos, k * 4)) {
      const uint8_t* p = nullptr;
      int rc = get(pos, k, &p);
      if (rc) return rc;
      rc = gz_header(p, k, c - pos, hlen);
      if (rc != 1) return rc;
    }
  }
};

// grows b to hold `bytes`, keeping its first `keep` bytes
static int grow_keep(DevBuf& b, size_t bytes, size_t keep) {
  if (bytes <= b.cap) return ZES_OK;
  void* p = nullptr;
  const size_t want = bytes + bytes / 8 + 4096;
  HIPCHK(hipMalloc(&p, want));
  if (keep) HIPCHK(hipMemcpyAsync(p, b.p, keep, hipMemcpyDeviceToDevice, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  HIPCHK(release(b));
  b.p = p;
  b.cap = want;
  return ZES_OK;
}

// Members one after the other, the first one's header already read (hlen).  dev: the result goes to d_dst (capacity cap;
// NOSPACE once it does not fit, the members behind are still measured); else it collects in g.gz_acc.  A member is
// decoded straight to its place when that is 16-byte aligned and has room, else into g.gz_stage and copied.
static int gunzip_locked(GzSrc& S, uint64_t hlen, bool dev, uint8_t* d_dst, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  int rc;
  uint64_t pos = 0, total = 0;
  flags &= ~(ZES_F_CHECK_ADLER | ZES_F_GZIP_SERIAL);
  for (bool first = true;; first = false) {
    if (!first && (rc = S.header(pos, &hlen))) return rc;
    const uint64_t body = pos + hlen;
    uint8_t* base = dev ? d_dst : (uint8_t*)g.gz_acc.p;
    const uint64_t room = dev ? (cap > total ? cap - total : 0) : (g.gz_acc.cap > total + 64 ? g.gz_acc.cap - total - 64 : 0);
    bool direct = base && room && (((uintptr_t)(base + total)) & 15u) == 0;
    uint64_t m = 0, used = 0;
    if (direct) {
      rc = inflate_raw_dev_locked(S.d, S.c, body, base + total, room, &m, &used, flags);
      if (rc == ZES_E_NOSPACE) direct = false;
      else if (rc) return rc;
    }
    const uint8_t* res = base + total;
    if (!direct) {
      rc = grow_and_retry(g.gz_stage, S.c - body, m, &m, [&](uint8_t* d_stage, uint64_t scap, uint64_t* got) {
        return inflate_raw_dev_locked(S.d, S.c, body, d_stage, scap, got, &used, flags);
      });
      if (rc) return rc;
      res = (const uint8_t*)g.gz_stage.p;
    }
    const uint64_t tpos = body + used;  // the trailer: CRC-32 and ISIZE of this member's output
    if (tpos + 8 > S.c) return ZES_E_GZIP;
    const uint8_t* tp = nullptr;
    if ((rc = S.get(tpos, 8, &tp))) return rc;
    const uint32_t want_crc = get_le32(tp), want_size = get_le32(tp + 4);
    uint32_t crc = 0;
    if ((rc = crc32_locked(res, m, &crc))) return rc;
    if (crc != want_crc || (uint32_t)m != want_size) return ZES_E_CHECKSUM;
    if (!direct && m) {
      if (dev) {
        if (total + m <= cap) HIPCHK(hipMemcpyAsync(d_dst + total, res, m, hipMemcpyDeviceToDevice, g.stream));
      } else {
        if ((rc = grow_keep(g.gz_acc, total + m + 64, total))) return rc;
        HIPCHK(hipMemcpyAsync((uint8_t*)g.gz_acc.p + total, res, m, hipMemcpyDeviceToDevice, g.stream));
      }
      HIPCHK(hipStreamSynchronize(g.stream));  // (the staging buffer is the next member's)
    }
    total += m;
    pos = tpos + 8;
    while (pos < S.c) {  // zero bytes between and after members
      const uint64_t k = std::min<uint64_t>(S.c - pos, 4096);
      const uint8_t* p = nullptr;
      if ((rc = S.get(pos, k, &p))) return rc;
      uint64_t i = 0;
      while (i < k && p[i] == 0) i++;
      pos += i;
      if (i < k) break;
    }
    if (pos >= S.c) break;
  }
  *out_len = total;
  return (dev && total > cap) ? ZES_E_NOSPACE : ZES_OK;
}

// ---- the member-parallel reader (include/zes.h: "Member-parallel reading") ----
// the members of the input when it is such a file from its first byte to its last (*ok), else nothing
static int gz_walk(GzSrc& S, std::vector<ZesGzMember>& tab, bool* ok) {
  *ok = false;
  tab.clear();
  if (S.h) {  // the caller's memory
    const bool whole = gz_walk_host(S.h, S.c, [&](uint64_t pos, ZesGzMember m) {
      m.crc = get_le32(S.h + pos + m.size - 8);
      m.isize = get_le32(S.h + pos + m.size - 4);
      tab.push_back(m);
    });
    *ok = whole && tab.size() >= 2;
    return ZES_OK;
  }
  int rc;
  const uint8_t* p = nullptr;
  const uint64_t k = std::min<uint64_t>(S.c, 4096);  // (the bytes the header check has brought down already)
  if ((rc = S.get(0, k, &p))) return rc;
  ZesGzMember m0;
  if (!gz_member(p, k, S.c, &m0) || m0.size >= S.c) return ZES_OK;  // an ordinary gzip file: no launch, no table
  // the table's size: members as long as the first one, four times over (a file of shorter ones goes member by member)
  const uint32_t cap = (uint32_t)std::min<uint64_t>({S.c / 28 + 1, 4 * (S.c / m0.size) + 1024, (uint64_t)1 << 28});
  if (gz_walk_room(cap)) return ZES_OK;
  if ((rc = gz_walk_dev(S.d, S.c, cap, [&](const ZesGzWalk& w) { return w.ok && w.count >= 2 && w.count <= cap; }, tab))) return rc;
  *ok = !tab.empty();
  return ZES_OK;
}

// One member of a batch of gz_decode_batch: where it lies in the source, what its header and trailer say, and the part of its
// output that is wanted: bytes [skip, skip + take) of it go to dst + dst_off (a whole member: skip 0, take = its ISIZE)
struct GzPart {
  uint64_t pos;
  ZesGzMember m;
  uint64_t dst_off;
  uint32_t skip, take;
};

// ---- DEFLATE bodies as one batch: the plan of gz_decode_batch (gzip members) and zip_read_core (ZIP entries), stated once ----
// body_plan gives every part its places, the caller puts the bodies there (the staging is what differs: k_gz_gather for
// members, k_zip_stage for entries, which also judges the local headers), body_run decodes and checks them.
// A body of `len` bytes stands in gz_bodies behind a 78 9C, in a slot of gz_slot_in(len) bytes (the decoders read whole 16-byte
// groups, and some way past a stream's end); an output of m bytes that cannot be decoded in place gets gz_slot_out(m) bytes of
// gz_outs, of which the job may write gz_slot_cap(m).
static uint64_t gz_slot_in(uint64_t len) { return gz_up16(2 + len) + 64; }
static uint64_t gz_slot_cap(uint64_t m) { return std::max<uint64_t>(gz_up16(m), 16); }
static uint64_t gz_slot_out(uint64_t m) { return gz_slot_cap(m) + 16; }

// One part of a batch: what its container says, and the part of its output that is wanted: bytes [skip, skip + take) of it go
// to dst + dst_off (a whole part: skip 0, take = isize)
struct BodyPart {
  uint64_t len;         // the body's bytes
  uint32_t isize, crc;  // the output's length and CRC-32
  uint64_t dst_off;
  uint32_t skip, take;
  bool deflate;         // a DEFLATE body; else the staging puts the bytes in place itself (a stored entry)
  int status;           // so far: a part that is not at ZES_OK is neither decoded nor checked
  // body_plan's: the slot in gz_bodies, and either decoded in place (direct) or into a slot of gz_outs
  uint64_t islot = 0, oslot = 0;
  bool direct = false;
  bool whole() const { return skip == 0 && take == isize; }
};

// A part is decoded in place when the 16-byte groups the decoders write stay inside its own part of dst: whole, at a 16-byte
// boundary, a multiple of 16 long.  The others get a slot of their own (the parts run side by side: a group that reaches into
// a neighbour's range would race with it).  exact: no byte of dst outside the parts is written; else the last part with
// output may also be decoded in place up to the next 16-byte boundary below dst_cap.
static int body_plan(std::vector<BodyPart>& ps, uint8_t* dst, uint64_t dst_cap, bool exact) {
  int rc;
  const BodyPart* last_out = nullptr;
  for (const BodyPart& p : ps)
    if (!exact && p.isize) last_out = &p;
  uint64_t ipos = 0, opos = 0;
  for (BodyPart& p : ps) {
    if (!p.deflate) continue;
    const uint64_t m = p.isize;
    p.islot = ipos;
    ipos += gz_slot_in(p.len);
    p.direct = dst && m && p.whole() && ((uintptr_t)(dst + p.dst_off) & 15u) == 0 &&
               ((m & 15u) == 0 || (&p == last_out && gz_up16(p.dst_off + m) <= dst_cap));
    if (!p.direct) {
      p.oslot = opos;
      opos += gz_slot_out(m);
    }
  }
  if ((rc = ensure(g.gz_bodies, ipos + 64)) || (rc = ensure(g.gz_outs, opos + 64))) return rc;
  return ZES_OK;
}

// A body's job behind inflate_jobs (want_end set) against what its container says: the body's inflate status when it does not
// decode; ZES_E_CHECKSUM when the output is not `want` bytes long (one that outgrew its capacity included) or the stream does
// not end in the last of the body's `len` bytes; else ZES_OK (the CRC-32 is the caller's next step).
static int gz_job_verdict(const InfJob& j, uint64_t want, uint64_t len) {
  if (j.status != ZES_OK && j.status != ZES_E_NOSPACE) return j.status;
  if (j.status != ZES_OK || j.out_len != want || j.end_bit < 16 || (j.end_bit - 16 + 7) / 8 != len) return ZES_E_CHECKSUM;
  return ZES_OK;
}

// The staged parts decoded and checked: one inflate_jobs call for the DEFLATE bodies at ZES_OK (none when there is no such
// body), one gather of the outputs that were not decoded in place, one segmented CRC-32 launch with a segment per part (of
// no bytes for a part with a status).  A part's status becomes what it is guilty of: its body's inflate status, or
// ZES_E_CHECKSUM — an output that is not isize bytes long (one that would outgrow its slot included), a stream that does not
// end in the body's last byte, a CRC-32 mismatch.  stop: the first part in order with a status ends the call, and that status
// is returned (a job's verdict comes before the gather and the CRC launch); else every part gets its own and the call goes
// on.  With a status a part's memory may have been written to.  stamps: null, or the time in front of and behind inflate_jobs.
static int body_run(std::vector<BodyPart>& ps, uint8_t* dst, uint32_t flags, bool stop, std::chrono::steady_clock::time_point* stamps) {
  int rc;
  const uint32_t n = (uint32_t)ps.size();
  // one base for both kinds of destination (inflate_jobs takes one pointer and an offset per job): the lower of the two
  uint8_t* outs = (uint8_t*)g.gz_outs.p;
  uint8_t* base = dst && dst < outs ? dst : outs;
  std::vector<InfJob> jobs;
  std::vector<uint32_t> jp;  // job -> part
  bool any = false;
  for (uint32_t k = 0; k < n; k++) {
    const BodyPart& p = ps[k];
    if (!p.deflate) continue;
    uint8_t* to = p.direct ? dst + p.dst_off : outs + p.oslot;
    InfJob j{p.islot, 2 + p.len, (uint64_t)(to - base), p.direct ? p.isize : gz_slot_cap(p.isize), 0, p.status, 0};
    j.want_end = true;
    jobs.push_back(j);
    jp.push_back(k);
    any = any || p.status == ZES_OK;
  }
  if (any) {  // (inflate_jobs leaves a job with a status alone)
    const std::vector<uint8_t> firsts(jobs.size(), 0x78);
    if (stamps) stamps[0] = std::chrono::steady_clock::now();
    if ((rc = inflate_jobs((const uint8_t*)g.gz_bodies.p, base, jobs, firsts.data(), flags))) return rc;
    keep_times();
    if (stamps) stamps[1] = std::chrono::steady_clock::now();
  }
  for (size_t i = 0; i < jobs.size(); i++) {
    BodyPart& p = ps[jp[i]];
    if (p.status == ZES_OK) p.status = gz_job_verdict(jobs[i], p.isize, p.len);
    if (p.status && stop) return p.status;
  }
  // a whole part's output is checked where it ends up, a trimmed one's in its slot, over all its bytes
  std::vector<ZesGzSeg> segs;
  std::vector<ZesCrcSeg> csegs(n);
  for (uint32_t k = 0; k < n; k++) {
    const BodyPart& p = ps[k];
    const bool ok = p.status == ZES_OK && p.isize;
    if (ok && p.deflate && !p.direct && p.take) segs.push_back(ZesGzSeg{p.oslot + p.skip, p.dst_off, p.take, 0u, 0u});
    csegs[k] = ok ? ZesCrcSeg{(uint64_t)((p.whole() ? dst + p.dst_off : outs + p.oslot) - base), p.isize} : ZesCrcSeg{0, 0};
  }
  if ((rc = gz_gather(outs, dst, segs))) return rc;
  std::vector<uint32_t> crc(n);
  if ((rc = crc32_batch_locked(base, csegs.data(), n, crc.data()))) return rc;
  for (uint32_t k = 0; k < n; k++)
    if (ps[k].status == ZES_OK && crc[k] != ps[k].crc) {
      ps[k].status = ZES_E_CHECKSUM;
      if (stop) return ZES_E_CHECKSUM;
    }
  return ZES_OK;
}

// Members as one batch (gunzip_parallel: a whole file; bgzf_read_core: the members a range touches): one gather of the
// bodies into body_plan's slots, then body_run.  Every member is decoded whole and must check out: ZES_OK when all do, else
// what the first member in file order that does not is guilty of (body_run, stop), or the status of a scratch buffer that
// could not grow.  exact, stamps: body_plan's and body_run's.
static int gz_decode_batch(const uint8_t* d_src, const std::vector<GzPart>& ps, uint8_t* dst, uint64_t dst_cap, bool exact, uint32_t flags,
                           std::chrono::steady_clock::time_point* stamps) {
  int rc;
  std::vector<BodyPart> bs;
  for (const GzPart& p : ps) bs.push_back(BodyPart{p.m.size - p.m.hlen - 8, p.m.isize, p.m.crc, p.dst_off, p.skip, p.take, true, ZES_OK});
  if ((rc = body_plan(bs, dst, dst_cap, exact))) return rc;
  std::vector<ZesGzSeg> segs;
  for (size_t k = 0; k < ps.size(); k++) segs.push_back(ZesGzSeg{ps[k].pos + ps[k].m.hlen, bs[k].islot + 2, bs[k].len, 1u, 0u});
  if ((rc = gz_gather(d_src, (uint8_t*)g.gz_bodies.p, segs))) return rc;
  return body_run(bs, dst, flags & ~(ZES_F_CHECK_ADLER | ZES_F_GZIP_SERIAL), true, stamps);
}

// All members of a file as one batch (gz_decode_batch).  *done only when every member checks out; in every other case
// nothing has been decided (the result's memory may have been written to) and the serial path runs.
// dev: the result goes to d_dst (capacity cap), else to g.gz_acc.
static int gunzip_parallel(GzSrc& S, bool dev, uint8_t* d_dst, uint64_t cap, uint64_t* out_len, uint32_t flags, bool* done) {
  *done = false;
  int rc;
  std::vector<ZesGzMember> tab;
  bool ok = false;
  // ZES_DEBUG: where the call's wall time goes
  static const bool dbg = getenv("ZES_DEBUG") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const auto t0 = now();
  if ((rc = gz_walk(S, tab, &ok))) return rc;
  const auto t1 = now();
  if (!ok || tab.size() >= (1u << 28)) return ZES_OK;
  const uint32_t n = (uint32_t)tab.size();
  std::vector<GzPart> ps(n);
  uint64_t total = 0, at = 0;
  for (uint32_t k = 0; k < n; k++) {
    ps[k] = GzPart{at, tab[k], total, 0u, tab[k].isize};
    at += tab[k].size;
    total += tab[k].isize;
  }
  if (dev && total > cap) return ZES_OK;
  if (!dev && ensure(g.gz_acc, total + 64)) return ZES_OK;
  std::chrono::steady_clock::time_point st[2];
  if ((rc = gz_decode_batch(S.d, ps, dev ? d_dst : (uint8_t*)g.gz_acc.p, dev ? cap : g.gz_acc.cap, false, flags, st))) return rc;
  if (dbg)
    fprintf(stderr, "zes gunzip, %u members as one batch: walk %.3f ms, plan + gather %.3f, inflate_jobs %.3f, gather + CRC-32 %.3f\n", n, ms(t0, t1),
            ms(t1, st[0]), ms(st[0], st[1]), ms(st[1], now()));
  *out_len = total;
  g.last_members = (int)n;
  *done = true;
  return ZES_OK;
}

// the parallel path where it applies and succeeds, else the members one after the other
static int gunzip_any(GzSrc& S, uint64_t hlen, bool dev, uint8_t* d_dst, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  g.last_members = 0;
  if (!(flags & ZES_F_GZIP_SERIAL)) {
    bool done = false;
    uint64_t n = 0;
    if (gunzip_parallel(S, dev, d_dst, cap, &n, flags, &done) == ZES_OK && done) {
      *out_len = n;
      return ZES_OK;
    }
    (void)hipGetLastError();
    g.carry.clear();
  }
  return gunzip_locked(S, hlen, dev, d_dst, cap, out_len, flags);
}

int zes_gunzip_dev(const uint8_t* d_in, uint64_t c, uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (!out_len || (!d_in && c)) return ZES_E_ARG;
  *out_len = 0;
  if (((uintptr_t)d_out) & 15u) return ZES_E_ARG;
  if (c == 0) return ZES_E_GZIP;
  LOCK_READY();
  GzSrc S{nullptr, d_in, c};
  uint64_t hlen = 0;
  if ((rc = S.header(0, &hlen))) return rc;
  rc = gunzip_any(S, hlen, true, d_out, cap, out_len, flags);
  collect_times();
  return rc;
}

static int gunzip_host(const uint8_t* in, uint64_t c, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags, zes_alloc_fn alloc,
                       void* user) {
  if (!out_len || (!in && c)) return ZES_E_ARG;
  *out_len = 0;
  if (c == 0) return ZES_E_GZIP;
  uint64_t hlen = 0;
  if (const int hrc = gz_header(in, c, c, &hlen)) return hrc;  // (decided before the device is touched)
  LOCK_READY();
  if ((rc = stage_in(g.gz_in, in, c))) return rc;
  if (g.gz_acc.cap < std::max<uint64_t>(c * 4, 1 << 20) && (rc = ensure(g.gz_acc, std::max<uint64_t>(c * 4, 1 << 20) + 64))) return rc;
  GzSrc S{in, (const uint8_t*)g.gz_in.p, c};
  uint64_t n = 0;
  rc = gunzip_any(S, hlen, false, nullptr, 0, &n, flags);
  collect_times();
  if (rc) return rc;
  *out_len = n;
  if (alloc) {
    out = alloc(user, 0, n);
    if (!out) return ZES_E_ARG;
    cap = n;
  }
  if (n > cap) return ZES_E_NOSPACE;
  return download(out, (const uint8_t*)g.gz_acc.p, n);
}

int zes_gunzip(const uint8_t* in, uint64_t c, uint8_t* out, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  UseDev ud(route_host());
  return gunzip_host(in, c, out, cap, out_len, flags, nullptr, nullptr);
}

int zes_gunzip_alloc(const uint8_t* in, uint64_t c, zes_alloc_fn alloc, void* user, uint64_t* out_len, uint32_t flags) {
  UseDev ud(route_host());
  if (!alloc) return ZES_E_ARG;
  return gunzip_host(in, c, nullptr, 0, out_len, flags, alloc, user);
}

// ---- BGZF random access (include/zes.h: "BGZF random access"): the member index and range reads through it ----
struct BgzfEntry {  // a member of the chain from byte 0: where it starts, how long its output is
  uint64_t pos;
  uint32_t isize;
};

static int bgzf_index_args(const uint8_t* in, uint64_t c, const uint64_t* coff, const uint64_t* uoff, uint64_t cap, uint64_t* members, uint32_t flags) {
  if (!members || (!in && c) || (flags & ~ZES_F_INDEX_WALK) || (!coff) != (!uoff) || (!coff && cap)) return ZES_E_ARG;
  *members = 0;
  return c ? ZES_OK : ZES_E_GZIP;
}

// the index of a chain: members + 1 entries, the last one the file's end and the total of the ISIZE fields
static int bgzf_index_out(const std::vector<BgzfEntry>& ch, uint64_t c, uint64_t* coff, uint64_t* uoff, uint64_t cap, uint64_t* members) {
  *members = ch.size();
  if (cap < ch.size() + 1) return ZES_E_NOSPACE;
  uint64_t u = 0;
  for (size_t k = 0; k < ch.size(); k++) {
    coff[k] = ch[k].pos;
    uoff[k] = u;
    u += ch[k].isize;
  }
  coff[ch.size()] = c;
  uoff[ch.size()] = u;
  return ZES_OK;
}

int zes_bgzf_index(const uint8_t* in, uint64_t c, uint64_t* coff, uint64_t* uoff, uint64_t cap, uint64_t* members, uint32_t flags) {
  if (const int arc = bgzf_index_args(in, c, coff, uoff, cap, members, flags)) return arc;
  std::vector<BgzfEntry> ch;
  if (!gz_walk_host(in, c, [&](uint64_t pos, const ZesGzMember& m) { ch.push_back(BgzfEntry{pos, get_le32(in + pos + m.size - 4)}); })) return ZES_E_GZIP;
  return bgzf_index_out(ch, c, coff, uoff, cap, members);
}

constexpr uint64_t BGZF_MARK_FIRST = 4096;  // candidates that come down together with the counter

// The chain of members of the device-resident file d_in[0, c), c != 0 (*ok: it is BGZF from its first byte to its last).
// The parallel finder: k_bgzf_mark lists every position whose member qualifies, one read-back brings the counter and the
// first BGZF_MARK_FIRST records down (a second one the rest, when a file has more), and the chain from 0 is followed through
// the list sorted by position; candidates the chain does not reach (headers inside stored payloads) play no part.
// With more candidates than the list holds (c / 256 + 1024), or with `walk`, k_gz_walk answers, its table sized for the
// worst case: as many members as there were candidates, or c / 28 + 1 when nothing has been counted.
static int bgzf_find_dev(const uint8_t* d_in, uint64_t c, bool walk, std::vector<BgzfEntry>& ch, bool* ok) {
  *ok = false;
  ch.clear();
  int rc;
  uint64_t counted = 0;
  if (!walk) {
    const uint64_t lcap = c / 256 + 1024;
    const uint64_t tiles = (((uintptr_t)d_in & 15u) + c + ZES_BGZF_MARK_TILE - 1) / ZES_BGZF_MARK_TILE;
    if (lcap >= (1ull << 31) || tiles >= (1ull << 31)) return ZES_E_ARG;
    if ((rc = ensure(g.gz_tab, sizeof(ZesBgzfMark) + sizeof(ZesBgzfCand) * (size_t)lcap))) return rc;
    ZesBgzfMark* d_head = (ZesBgzfMark*)g.gz_tab.p;
    const ZesBgzfCand* d_list = (const ZesBgzfCand*)(d_head + 1);
    HIPCHK(hipMemsetAsync(d_head, 0, sizeof *d_head, g.stream));
    {
      Timed t("k_bgzf_mark");
      hipLaunchKernelGGL(k_bgzf_mark, dim3((uint32_t)tiles), dim3(ZES_BGZF_MARK_THREADS), 0, g.stream, d_in, c, d_head, (ZesBgzfCand*)(d_head + 1),
                         (uint32_t)lcap);
    }
    HIPCHK(hipGetLastError());
    const size_t first = (size_t)std::min<uint64_t>(lcap, BGZF_MARK_FIRST);
    std::vector<uint8_t> down(sizeof(ZesBgzfMark) + sizeof(ZesBgzfCand) * first);
    HIPCHK(hipMemcpyAsync(down.data(), d_head, down.size(), hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    ZesBgzfMark head;
    memcpy(&head, down.data(), sizeof head);
    counted = head.count;
    if (counted <= lcap) {
      std::vector<ZesBgzfCand> list((size_t)counted);
      const size_t got = std::min<size_t>(first, list.size());
      if (got) memcpy(list.data(), down.data() + sizeof head, sizeof(ZesBgzfCand) * got);
      if (list.size() > got) {
        HIPCHK(hipMemcpyAsync(list.data() + got, d_list + got, sizeof(ZesBgzfCand) * (list.size() - got), hipMemcpyDeviceToHost, g.stream));
        HIPCHK(hipStreamSynchronize(g.stream));
      }
      std::sort(list.begin(), list.end(), [](const ZesBgzfCand& a, const ZesBgzfCand& b) { return a.pos < b.pos; });
      uint64_t pos = 0;
      while (pos < c) {  // (a candidate's size keeps it inside the file: pos never passes c)
        auto it = std::lower_bound(list.begin(), list.end(), pos, [](const ZesBgzfCand& a, uint64_t p) { return a.pos < p; });
        if (it == list.end() || it->pos != pos) return ZES_OK;
        ch.push_back(BgzfEntry{pos, it->isize});
        pos += it->size;
      }
      *ok = true;
      return ZES_OK;
    }
  }
  const uint64_t cap = std::min<uint64_t>(counted ? counted : c / 28 + 1, 0xFFFFFFFFull);
  if ((rc = gz_walk_room(cap))) return rc;
  std::vector<ZesGzMember> tab;
  // (head.ok asks for two members, as zes_gunzip's batch does; one is enough here: the walk got to the file's end)
  if ((rc = gz_walk_dev(d_in, c, (uint32_t)cap, [&](const ZesGzWalk& w) { return w.count && w.count <= cap && w.end == c; }, tab))) return rc;
  if (tab.empty()) return ZES_OK;
  uint64_t pos = 0;
  for (const ZesGzMember& m : tab) {
    ch.push_back(BgzfEntry{pos, m.isize});
    pos += m.size;
  }
  *ok = true;
  return ZES_OK;
}

int zes_bgzf_index_dev(const uint8_t* d_in, uint64_t c, uint64_t* coff, uint64_t* uoff, uint64_t cap, uint64_t* members, uint32_t flags) {
  ROUTE_DEV(d_in);
  if (const int arc = bgzf_index_args(d_in, c, coff, uoff, cap, members, flags)) return arc;
  LOCK_READY();
  std::vector<BgzfEntry> ch;
  bool ok = false;
  rc = bgzf_find_dev(d_in, c, (flags & ZES_F_INDEX_WALK) != 0, ch, &ok);
  collect_times();
  if (rc) return rc;
  if (!ok) return ZES_E_GZIP;
  return bgzf_index_out(ch, c, coff, uoff, cap, members);
}

// What the index says about a read of [pos, pos + len): *out_len = n, the bytes it yields, and the members with output in
// that range (`touched`; none when n == 0).  Only their entries are looked at: O(log members + members in the range).
static int bgzf_read_plan(uint64_t c, const uint64_t* coff, const uint64_t* uoff, uint64_t members, uint64_t pos, uint64_t len, uint64_t cap,
                          uint64_t* out_len, std::vector<uint64_t>& touched) {
  const uint64_t total = uoff[members];
  if (pos > total) return ZES_E_ARG;
  const uint64_t n = std::min(len, total - pos);
  *out_len = n;
  if (n > cap) return ZES_E_NOSPACE;
  if (!n) return ZES_OK;
  const uint64_t end = pos + n;
  const uint64_t* ue = uoff + members + 1;
  const uint64_t a = (uint64_t)(std::upper_bound(uoff, ue, pos) - uoff), b = (uint64_t)(std::lower_bound(uoff, ue, end) - uoff);
  // member k0 holds byte pos, member k1 byte end - 1 (an index whose entries are out of order can send the searches anywhere)
  if (!a || !b || b > members || a > b) return ZES_E_GZIP;
  const uint64_t k0 = a - 1, k1 = b - 1;
  if (uoff[k0] > pos || uoff[k0 + 1] <= pos || uoff[k1] >= end || uoff[k1 + 1] < end) return ZES_E_GZIP;
  for (uint64_t k = k0; k <= k1; k++) {
    if (uoff[k + 1] < uoff[k]) return ZES_E_GZIP;
    if (uoff[k + 1] == uoff[k]) continue;  // no output: skipped
    if (coff[k] >= coff[k + 1] || coff[k + 1] > c || coff[k + 1] - coff[k] > 65536 || coff[k + 1] - coff[k] < 20) return ZES_E_GZIP;
    touched.push_back(k);
  }
  return ZES_OK;
}

constexpr uint64_t BGZF_PEEK = ZES_GZ_HLEN_MAX + 16;  // a touched member's first 256 bytes and its trailer, as the device form brings them down

// The touched members decoded and the range's bytes put at dst[0, n).  d_src holds the file from byte `src_at` on; h: the
// file in the caller's memory (host form), or null: the members' headers and trailers come down from d_src in one gather.
// A member that is not what the index says (a stale or foreign index) is ZES_E_GZIP; the rest is gz_decode_batch's verdict.
static int bgzf_read_core(const uint8_t* h, const uint8_t* d_src, uint64_t src_at, uint64_t c, const uint64_t* coff, const uint64_t* uoff, uint64_t pos,
                          uint64_t n, const std::vector<uint64_t>& touched, uint8_t* dst, uint32_t flags) {
  int rc;
  const size_t nt = touched.size();
  std::vector<uint8_t> peek;
  if (!h) {
    std::vector<ZesGzSeg> segs;
    for (size_t i = 0; i < nt; i++) {
      const uint64_t at = coff[touched[i]], size = coff[touched[i] + 1] - at;
      segs.push_back(ZesGzSeg{at - src_at, i * BGZF_PEEK, std::min<uint64_t>(size, ZES_GZ_HLEN_MAX), 0u, 0u});
      segs.push_back(ZesGzSeg{at - src_at + size - 8, i * BGZF_PEEK + ZES_GZ_HLEN_MAX, 8, 0u, 0u});
    }
    peek.resize(nt * BGZF_PEEK);
    if ((rc = gather_down(g.gz_stage, d_src, segs, peek.data(), peek.size()))) return rc;
  }
  std::vector<GzPart> ps(nt);
  for (size_t i = 0; i < nt; i++) {
    const uint64_t k = touched[i], at = coff[k], size = coff[k + 1] - at, u0 = uoff[k], u1 = uoff[k + 1];
    const uint8_t* hd = h ? h + at : peek.data() + i * BGZF_PEEK;
    const uint8_t* tr = h ? h + at + size - 8 : hd + ZES_GZ_HLEN_MAX;
    ZesGzMember m;
    if (!gz_member(hd, std::min<uint64_t>(size, ZES_GZ_HLEN_MAX), c - at, &m) || m.size != size) return ZES_E_GZIP;
    m.crc = get_le32(tr);
    m.isize = get_le32(tr + 4);
    if (m.isize != u1 - u0) return ZES_E_GZIP;
    const uint64_t lo = std::max(pos, u0), hi = std::min(pos + n, u1);
    ps[i] = GzPart{at - src_at, m, lo - pos, (uint32_t)(lo - u0), (uint32_t)(hi - lo)};
  }
  if ((rc = gz_decode_batch(d_src, ps, dst, n, true, flags, nullptr))) return rc;
  g.last_members = (int)nt;
  return ZES_OK;
}

static int bgzf_read_args(const uint8_t* in, const uint64_t* coff, const uint64_t* uoff, uint64_t members, const uint8_t* out, uint64_t* out_len,
                          uint32_t flags) {
  if (!in || !coff || !uoff || !out || !out_len || !members || (flags & ~ZES_F_PIECES)) return ZES_E_ARG;
  *out_len = 0;
  return ZES_OK;
}

// a call that decodes nothing: zes_last_gunzip_members reports 0 after it.  (Not one helper with call_none: this one is
// also the way out of a call whose plan failed, and leaves the times alone as every call does that ends in its checks.)
static void bgzf_read_none() {
  std::lock_guard<std::mutex> lk(g_mu);
  g.last_members = 0;
}

int zes_bgzf_read_dev(const uint8_t* d_in, uint64_t c, const uint64_t* coff, const uint64_t* uoff, uint64_t members, uint64_t pos, uint64_t len,
                      uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (const int arc = bgzf_read_args(d_in, coff, uoff, members, d_out, out_len, flags)) return arc;
  std::vector<uint64_t> touched;
  if (const int prc = bgzf_read_plan(c, coff, uoff, members, pos, len, cap, out_len, touched); prc || touched.empty()) {
    bgzf_read_none();
    return prc;
  }
  LOCK_READY();
  g.last_members = 0;
  return call_done(bgzf_read_core(nullptr, d_in, 0, c, coff, uoff, pos, *out_len, touched, d_out, flags), true);
}

int zes_bgzf_read(const uint8_t* in, uint64_t c, const uint64_t* coff, const uint64_t* uoff, uint64_t members, uint64_t pos, uint64_t len, uint8_t* out,
                  uint64_t cap, uint64_t* out_len, uint32_t flags) {
  UseDev ud(route_host());
  if (const int arc = bgzf_read_args(in, coff, uoff, members, out, out_len, flags)) return arc;
  std::vector<uint64_t> touched;
  if (const int prc = bgzf_read_plan(c, coff, uoff, members, pos, len, cap, out_len, touched); prc || touched.empty()) {
    bgzf_read_none();
    return prc;
  }
  LOCK_READY();
  g.last_members = 0;
  // only the file bytes of the touched members cross to the device
  const uint64_t lo = coff[touched.front()], hi = coff[touched.back() + 1], n = *out_len;
  if ((rc = stage_in(g.gz_in, in + lo, hi - lo))) return rc;
  if ((rc = ensure(g.gz_acc, n + 64))) return rc;
  if ((rc = call_done(bgzf_read_core(in, (const uint8_t*)g.gz_in.p, lo, c, coff, uoff, pos, n, touched, (uint8_t*)g.gz_acc.p, flags), true))) return rc;
  return download(out, (const uint8_t*)g.gz_acc.p, n);
}

// ---- ZIP archives (include/zes.h: "ZIP archives"): the entry index and batch extraction through it ----
constexpr uint64_t ZIP_END = 22, ZIP_TAIL = ZIP_END + 65535;  // the end record without its comment; with the longest one

// The index rule, once, for both forms: fetch(pos, len) answers with the file's bytes [pos, pos + len) (null: they could not
// be had, *frc says why), and is called twice at most — for the last min(c, ZIP_TAIL) bytes, then for the directory (from 20
// bytes in front of the end record on, when a comment of more than 65515 bytes has pushed those out of the first piece).
static int zip_index_core(uint64_t c, const std::function<const uint8_t*(uint64_t, uint64_t)>& fetch, int* frc, std::vector<zes_zip_entry>& ent,
                          std::vector<uint8_t>& names) {
  ent.clear();
  names.clear();
  if (c < ZIP_END) return ZES_E_ZIP;
  const uint64_t tail_at = c - std::min(c, ZIP_TAIL);
  const uint8_t* tail = fetch(tail_at, c - tail_at);
  if (!tail) return *frc;
  uint64_t p = c - ZIP_END;
  for (;; p--) {
    const uint8_t* e = tail + (p - tail_at);
    if (e[0] == 0x50 && e[1] == 0x4b && e[2] == 5 && e[3] == 6 && p + ZIP_END + get_le16(e + 20) == c) break;
    if (p == tail_at) return ZES_E_ZIP;
  }
  const uint8_t* e = tail + (p - tail_at);
  const uint32_t count = get_le16(e + 10);
  const uint64_t cd_size = get_le32(e + 12), cd_off = get_le32(e + 16);
  if (get_le16(e + 4) || get_le16(e + 6) || get_le16(e + 8) != count || count == 0xFFFF || cd_size == 0xFFFFFFFFull || cd_off == 0xFFFFFFFFull)
    return ZES_E_UNSUPPORTED;
  const bool bounds = cd_size + cd_off <= p;
  const bool loc_in_tail = p < 20 || p - 20 >= tail_at;
  auto locator = [](const uint8_t* q) { return q[0] == 0x50 && q[1] == 0x4b && q[2] == 6 && q[3] == 7; };
  if (loc_in_tail) {
    if (p >= 20 && locator(e - 20)) return ZES_E_UNSUPPORTED;
    if (!bounds) return ZES_E_ZIP;
  }
  const uint64_t dir_at = bounds ? p - cd_size : p, got_at = loc_in_tail ? dir_at : std::min(dir_at, p - 20);
  const uint8_t* got = fetch(got_at, p - got_at);
  if (!got && p != got_at) return *frc;
  if (!loc_in_tail) {
    if (locator(got + (p - 20 - got_at))) return ZES_E_UNSUPPORTED;
    if (!bounds) return ZES_E_ZIP;
  }
  const uint8_t* dir = got + (dir_at - got_at);
  const uint64_t base = p - cd_size - cd_off;
  uint64_t at = 0;
  while (at < cd_size) {
    const uint8_t* r = dir + at;
    if (cd_size - at < 46 || r[0] != 0x50 || r[1] != 0x4b || r[2] != 1 || r[3] != 2) return ZES_E_ZIP;
    const uint64_t nlen = get_le16(r + 28), len = 46 + nlen + get_le16(r + 30) + get_le16(r + 32);
    if (len > cd_size - at) return ZES_E_ZIP;
    const uint64_t csize = get_le32(r + 20), usize = get_le32(r + 24), off = get_le32(r + 42);
    if (csize == 0xFFFFFFFFull || usize == 0xFFFFFFFFull || off == 0xFFFFFFFFull || get_le16(r + 34)) return ZES_E_UNSUPPORTED;
    if (off + 30 > cd_off) return ZES_E_ZIP;
    zes_zip_entry z;
    z.hdr_off = base + off;
    z.name_pos = dir_at + at + 46;
    z.csize = (uint32_t)csize;
    z.usize = (uint32_t)usize;
    z.crc = get_le32(r + 16);
    z.name_off = (uint32_t)names.size();
    z.name_len = (uint16_t)nlen;
    z.method = (uint16_t)get_le16(r + 10);
    z.flags = (uint16_t)get_le16(r + 8);
    z.pad = 0;
    ent.push_back(z);
    names.insert(names.end(), r + 46, r + 46 + nlen);
    at += len;
  }
  return ent.size() == count ? ZES_OK : ZES_E_ZIP;
}

static int zip_index_args(const uint8_t* in, uint64_t c, const zes_zip_entry* ent, uint64_t cap, uint64_t* entries, const uint8_t* names,
                          uint64_t names_cap, uint64_t* names_len, uint32_t flags) {
  if (!entries || !names_len || (!in && c) || flags || (!ent && cap) || (!names && names_cap)) return ZES_E_ARG;
  *entries = 0;
  *names_len = 0;
  return ZES_OK;
}

static int zip_index_out(const std::vector<zes_zip_entry>& e, const std::vector<uint8_t>& nm, zes_zip_entry* ent, uint64_t cap, uint64_t* entries,
                         uint8_t* names, uint64_t names_cap, uint64_t* names_len) {
  *entries = e.size();
  *names_len = nm.size();
  if (cap < e.size() || names_cap < nm.size() || (!ent && !names)) return ZES_E_NOSPACE;
  if (!e.empty()) memcpy(ent, e.data(), sizeof(zes_zip_entry) * e.size());
  if (!nm.empty()) memcpy(names, nm.data(), nm.size());
  return ZES_OK;
}

int zes_zip_index(const uint8_t* in, uint64_t c, zes_zip_entry* ent, uint64_t cap, uint64_t* entries, uint8_t* names, uint64_t names_cap,
                  uint64_t* names_len, uint32_t flags) {
  if (const int arc = zip_index_args(in, c, ent, cap, entries, names, names_cap, names_len, flags)) return arc;
  std::vector<zes_zip_entry> e;
  std::vector<uint8_t> nm;
  int frc = ZES_OK;
  if (const int irc = zip_index_core(c, [&](uint64_t pos, uint64_t) { return in + pos; }, &frc, e, nm)) return irc;
  return zip_index_out(e, nm, ent, cap, entries, names, names_cap, names_len);
}

int zes_zip_index_dev(const uint8_t* d_in, uint64_t c, zes_zip_entry* ent, uint64_t cap, uint64_t* entries, uint8_t* names, uint64_t names_cap,
                      uint64_t* names_len, uint32_t flags) {
  ROUTE_DEV(d_in);
  if (const int arc = zip_index_args(d_in, c, ent, cap, entries, names, names_cap, names_len, flags)) return arc;
  if (c < ZIP_END) return ZES_E_ZIP;
  LOCK_READY();
  std::vector<zes_zip_entry> e;
  std::vector<uint8_t> nm;
  std::vector<uint8_t> piece[2];
  int k = 0, frc = ZES_OK;
  auto fetch = [&](uint64_t pos, uint64_t len) -> const uint8_t* {
    std::vector<uint8_t>& b = piece[k++ & 1];
    b.resize(len + 1);
    if (len && (hipMemcpyAsync(b.data(), d_in + pos, len, hipMemcpyDeviceToHost, g.stream) != hipSuccess || hipStreamSynchronize(g.stream) != hipSuccess)) {
      (void)hipGetLastError();
      frc = ZES_E_DEVICE;
      return nullptr;
    }
    return b.data();
  };
  if (const int irc = zip_index_core(c, fetch, &frc, e, nm)) return irc;
  return zip_index_out(e, nm, ent, cap, entries, names, names_cap, names_len);
}

// An entry's status as far as its index record alone decides it (include/zes.h, zes_zip_read*: step 1)
static int zip_entry_alone(const zes_zip_entry& z, uint64_t c) {
  if ((z.flags & 0x61u) || (z.method != 0 && z.method != 8)) return ZES_E_UNSUPPORTED;
  if (z.method == 0 && z.csize != z.usize) return ZES_E_ZIP;
  if (z.hdr_off > c || c - z.hdr_off < 30 || z.name_pos > c || c - z.name_pos < z.name_len) return ZES_E_ZIP;
  // (step 2's last test with an extra field of no bytes: a csize no file has gets its status here, not a scratch slot first)
  if (30ull + z.name_len + z.csize > c - z.hdr_off) return ZES_E_ZIP;
  return ZES_OK;
}

static int zip_read_args(const uint8_t* in, uint64_t c, const zes_zip_entry* ent, uint64_t nent, const uint32_t* sel, uint32_t count,
                         const uint64_t* out_len, const int32_t* status, uint32_t flags) {
  if ((flags & ~ZES_F_PIECES) || (!in && c)) return ZES_E_ARG;
  if (count && (!ent || !out_len || !status)) return ZES_E_ARG;
  if (!sel && count > nent) return ZES_E_ARG;
  for (uint32_t i = 0; sel && i < count; i++)
    if (sel[i] >= nent) return ZES_E_ARG;
  return ZES_OK;
}

// a ZIP or PNG call with nothing to do: no device work; the times and the tier of the call before do not stay (a successful
// call that launches nothing reports no launch; bgzf_read_none says why the two differ)
static void call_none() {
  std::lock_guard<std::mutex> lk(g_mu);
  g.last_tier = 0;
  collect_times();
}

// One entry of a zip_read_core batch: its index record, where its header and the directory's name lie in d_src and how many
// bytes of the file follow the header's first byte, and where its usize bytes go in dst
struct ZipPart {
  zes_zip_entry z;
  uint64_t hdr_at, name_at, limit, dst_off;
};

// The entries of ps whose status[k] is ZES_OK on entry (zip_entry_alone has passed them), as one batch on the plan of the gzip
// members (body_plan, body_run): every entry is whole and the mode is `exact`, no byte of dst outside the parts is written.
// The staging is k_zip_stage, which judges the local headers and puts the DEFLATE bodies into their slots and the stored
// entries in place; one read-back brings its verdicts down and they become the parts' statuses.  body_run goes on per
// entry: status[k] becomes the entry's status (include/zes.h, steps 2 to 4).
static int zip_read_core(const uint8_t* d_src, const std::vector<ZipPart>& ps, uint8_t* dst, int32_t* status, uint32_t flags) {
  int rc;
  g.last_tier = 0;
  std::vector<uint32_t> st;  // the staged entries
  std::vector<BodyPart> bs;
  for (uint32_t k = 0; k < ps.size(); k++)
    if (status[k] == ZES_OK) {
      st.push_back(k);
      bs.push_back(BodyPart{ps[k].z.csize, ps[k].z.usize, ps[k].z.crc, ps[k].dst_off, 0u, ps[k].z.usize, ps[k].z.method == 8, ZES_OK});
    }
  const uint32_t n = (uint32_t)st.size();
  if (!n) return ZES_OK;
  if ((rc = body_plan(bs, dst, 0, true))) return rc;
  std::vector<ZesZipRec> recs(n);
  std::vector<ZesZipVerdict> verd(n);
  Drain drain;  // (behind recs, which an upload reads, and verd, which the read-back writes)
  uint64_t longest = 0;
  for (uint32_t q = 0; q < n; q++) {
    const ZipPart& p = ps[st[q]];
    ZesZipRec& r = recs[q];
    memset(&r, 0, sizeof r);
    r.hdr_at = p.hdr_at;
    r.name_at = p.name_at;
    r.limit = p.limit;
    r.csize = p.z.csize;
    r.name_len = p.z.name_len;
    r.method = p.z.method;
    r.flag0 = p.z.flags & 1u;
    r.dst_off = bs[q].deflate ? bs[q].islot + 2 : p.dst_off;
    longest = std::max<uint64_t>(longest, p.z.csize);
  }
  const size_t o_verd = sizeof(ZesZipRec) * (size_t)n;
  if ((rc = ensure(g.gz_tab, o_verd + sizeof(ZesZipVerdict) * (size_t)n))) return rc;
  ZesZipVerdict* d_verd = (ZesZipVerdict*)((uint8_t*)g.gz_tab.p + o_verd);
  HIPCHK(hipMemcpyAsync(g.gz_tab.p, recs.data(), o_verd, hipMemcpyHostToDevice, g.stream));
  {
    const uint32_t ny = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((longest + GZ_GATHER_PIECE - 1) / GZ_GATHER_PIECE, 1), 256);
    Timed t("k_zip_stage");
    hipLaunchKernelGGL(k_zip_stage, dim3(n, ny), dim3(GZ_GATHER_THREADS), 0, g.stream, d_src, (uint8_t*)g.gz_bodies.p, dst, (const ZesZipRec*)g.gz_tab.p,
                       d_verd);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(verd.data(), d_verd, sizeof(ZesZipVerdict) * (size_t)n, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  for (uint32_t q = 0; q < n; q++) bs[q].status = verd[q].status;
  rc = body_run(bs, dst, flags & ZES_F_PIECES, false, nullptr);
  for (uint32_t q = 0; q < n; q++) status[st[q]] = bs[q].status;
  return rc;
}

int zes_zip_read_dev(const uint8_t* d_in, uint64_t c, const zes_zip_entry* ent, uint64_t nent, const uint32_t* sel, uint32_t count, uint8_t* d_out,
                     const uint64_t* out_off, uint64_t* out_len, int32_t* status, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (const int arc = zip_read_args(d_in, c, ent, nent, sel, count, out_len, status, flags)) return arc;
  if (count && !out_off) return ZES_E_ARG;
  if (!count) {
    call_none();
    return ZES_OK;
  }
  std::vector<ZipPart> ps(count);
  for (uint32_t i = 0; i < count; i++) {
    const zes_zip_entry& z = ent[sel ? sel[i] : i];
    out_len[i] = 0;
    status[i] = zip_entry_alone(z, c);
    ps[i] = ZipPart{z, z.hdr_off, z.name_pos, c - std::min(c, z.hdr_off), out_off[i]};
    if (status[i] == ZES_OK && z.usize && !d_out) return ZES_E_ARG;
  }
  LOCK_READY();
  if ((rc = call_done(zip_read_core(d_in, ps, d_out, status, flags), true))) return rc;
  for (uint32_t i = 0; i < count; i++)
    if (status[i] == ZES_OK) out_len[i] = ps[i].z.usize;
  return ZES_OK;
}

int zes_zip_read_alloc(const uint8_t* in, uint64_t c, const zes_zip_entry* ent, uint64_t nent, const uint32_t* sel, uint32_t count, zes_alloc_fn alloc,
                       void* user, uint64_t* out_len, int32_t* status, uint32_t flags) {
  UseDev ud(route_host());
  if (const int arc = zip_read_args(in, c, ent, nent, sel, count, out_len, status, flags)) return arc;
  if (!alloc) return ZES_E_ARG;
  if (!count) {
    call_none();
    return ZES_OK;
  }
  LOCK_READY();
  // only the selected entries' bytes cross to the device: header, name, extra field and body in one piece, the directory's
  // copy of the name in another
  HostBatch hb(g.gz_in, g.gz_acc);
  std::vector<ZipPart> ps(count);
  for (uint32_t i = 0; i < count; i++) {
    const zes_zip_entry& z = ent[sel ? sel[i] : i];
    out_len[i] = 0;
    status[i] = zip_entry_alone(z, c);
    ps[i] = ZipPart{z, 0, 0, 0, 0};
    if (status[i]) continue;
    ps[i].limit = c - z.hdr_off;
    ps[i].hdr_at = hb.place(in + z.hdr_off, std::min<uint64_t>(ps[i].limit, 30ull + z.name_len + get_le16(in + z.hdr_off + 28) + z.csize));
    ps[i].name_at = hb.place(in + z.name_pos, z.name_len);
    ps[i].dst_off = hb.room(z.usize);
  }
  if ((rc = hb.up())) return rc;
  if ((rc = call_done(zip_read_core(hb.d_in(), ps, hb.d_out(), status, flags), true))) return rc;
  return hb.hand_out(count, alloc, user, status, out_len, [&](uint32_t i) { return (uint64_t)ps[i].z.usize; }, [&](uint32_t i) { return ps[i].dst_off; });
}

// ---- ZIP writer (include/zes.h: "zes_zipwrite*"): local headers, names and bodies by k_zip_pack, the directory by the host ----
constexpr uint32_t ZIPW_COUNT_MAX = 65534;        // (65535 is ZIP64's mark)
constexpr uint64_t ZIPW_LEN_MAX = 0xFFFFFFFEull;  // (as is 0xFFFFFFFF in a size or an offset)

static uint64_t zipwrite_bound(const uint64_t* in_len, const uint16_t* name_len, uint32_t count) {
  uint64_t b = ZIP_END;
  for (uint32_t i = 0; i < count; i++) b += 30 + 46 + 2 * (uint64_t)name_len[i] + in_len[i];
  return b;
}

// the end record of an archive of `count` entries whose directory is [cd_off, cd_off + cd_size)
static void zip_end_record(uint8_t* e, uint32_t count, uint64_t cd_size, uint64_t cd_off) {
  memset(e, 0, ZIP_END);
  put_le32(e, 0x06054b50u);
  put_le16(e + 8, count);
  put_le16(e + 10, count);
  put_le32(e + 12, (uint32_t)cd_size);
  put_le32(e + 16, (uint32_t)cd_off);
}

// What both forms decide from the arguments alone (`data(i)`: entry i's bytes are there): ZES_E_ARG, then ZES_E_UNSUPPORTED
static int zipwrite_args(const std::function<bool(uint32_t)>& data, const uint64_t* in_len, const uint8_t* names, const uint16_t* name_len, uint32_t count, const uint8_t* out, uint64_t cap,
                         uint64_t* out_len, uint32_t flags) {
  if (!out_len || (flags & ~ZES_F_PIECES) || (!out && cap)) return ZES_E_ARG;
  *out_len = 0;
  if (count && (!in_len || !name_len)) return ZES_E_ARG;
  uint64_t nbytes = 0;
  for (uint32_t i = 0; i < count; i++) {
    if (in_len[i] && !data(i)) return ZES_E_ARG;
    nbytes += name_len[i];
  }
  if (nbytes && !names) return ZES_E_ARG;
  if (count > ZIPW_COUNT_MAX) return ZES_E_UNSUPPORTED;
  for (uint32_t i = 0; i < count; i++)
    if (in_len[i] > ZIPW_LEN_MAX) return ZES_E_UNSUPPORTED;
  return ZES_OK;
}

// The archive of the entries d_in[in_off[i], + in_len[i]) into d_out[0, cap), group by group as bgzip_core goes: a group is
// what EncGroup::form takes (an entry that the encoder refuses is spared and has no slot, so
// a group of such entries makes no encoder call); the sizes come back, the host chooses the method (8 when the raw stream
// is shorter than the entry, else 0) and the places, and one k_zip_pack launch writes the group's headers, names and bodies.
// The directory and the end record are made here and go up in one copy behind the last group.  g.gz_tab holds the names
// (uploaded once, padded to whole 16-byte groups) and behind them the group's records.  A result beyond cap: EncGroup's
// rule, with the directory as one more group.  ent: null, or the records zes_zip_index lists for the result.
// The host memory that the call's asynchronous uploads read (the padded names, every group's records, the directory, the
// encoder's tables) is declared in front of a Drain.  ZES_OK and ZES_E_NOSPACE come from behind the last synchronisation.
static int zipwrite_core(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, const uint8_t* names, const uint16_t* name_len, uint32_t count,
                         uint8_t* d_out, uint64_t cap, uint64_t* out_len, zes_zip_entry* ent, uint32_t flags) {
  int rc;
  g.carry.clear();
  std::vector<uint8_t> hnames, cd;
  // (of the whole call: uploads read it until the last synchronisation.  A group has one entry at least and a closing record:
  // at most `count` groups, whichever bound ends them)
  std::vector<ZesZipPackRec> recs(2 * (size_t)count + 1);
  EncGroup eg(flags, count);
  Drain drain;  // (behind hnames, cd, recs and eg)
  std::vector<uint32_t> name_off((size_t)count + 1, 0);
  for (uint32_t i = 0; i < count; i++) name_off[i + 1] = name_off[i] + name_len[i];  // (65534 names of 65535 bytes fit 32 bits)
  const size_t names_pad = (size_t)gz_up16(name_off[count]);
  hnames.assign(names_pad, 0);
  if (name_off[count]) memcpy(hnames.data(), names, name_off[count]);
  if ((rc = ensure(g.gz_tab, names_pad + sizeof(ZesZipPackRec) * (eg.o_off.size() + 1)))) return rc;
  if (names_pad) HIPCHK(hipMemcpyAsync(g.gz_tab.p, hnames.data(), names_pad, hipMemcpyHostToDevice, g.stream));
  ZesZipPackRec* d_recs = (ZesZipPackRec*)((uint8_t*)g.gz_tab.p + names_pad);
  std::vector<zes_zip_entry> z(count);
  size_t rpos = 0;
  uint64_t total = 0;
  for (uint32_t e0 = 0; e0 < count;) {
    uint64_t slots;
    const uint32_t cnt = eg.form(in_len + e0, count - e0, &slots);
    if ((rc = eg.encode(d_in, in_off + e0, in_len + e0, cnt, slots))) return rc;
    ZesZipPackRec* gr = &recs[rpos];
    uint32_t wgs = 0;
    for (uint32_t k = 0; k < cnt; k++) {
      const uint32_t i = e0 + k;
      const uint64_t len = in_len[i], raw = eg.raw[k];
      const bool deflated = eg.o_cap[k] && raw < len;
      if (total >= 0xFFFFFFFFull) return ZES_E_UNSUPPORTED;
      bool utf8 = false;
      for (uint32_t b = 0; b < name_len[i]; b++) utf8 = utf8 || names[name_off[i] + b] >= 0x80;
      zes_zip_entry& t = z[i];
      t.hdr_off = total;
      t.name_pos = 0;  // (known with the directory's place)
      t.csize = (uint32_t)(deflated ? raw : len);
      t.usize = (uint32_t)len;
      t.crc = eg.crc[k];
      t.name_off = name_off[i];
      t.name_len = name_len[i];
      t.method = deflated ? 8 : 0;
      t.flags = utf8 ? 0x0800 : 0;
      t.pad = 0;
      ZesZipPackRec& r = gr[k];
      memset(&r, 0, sizeof r);
      r.src_off = deflated ? eg.o_off[k] + 2 : in_off[i];
      r.dst_off = total;
      r.csize = t.csize;
      r.usize = t.usize;
      r.crc = t.crc;
      r.name_off = t.name_off;
      r.first_wg = wgs;
      r.name_len = t.name_len;
      r.method = t.method;
      r.flags = t.flags;
      wgs += (uint32_t)std::min<uint64_t>(std::max<uint64_t>(((uint64_t)t.csize + GZ_GATHER_PIECE - 1) / GZ_GATHER_PIECE, 1), ZES_ZIP_PACK_SHARES);
      total += 30ull + t.name_len + t.csize;
    }
    memset(&gr[cnt], 0, sizeof(ZesZipPackRec));
    gr[cnt].first_wg = wgs;
    if (eg.room(total, cap, d_out)) {
      HIPCHK(hipMemcpyAsync(d_recs, gr, sizeof(ZesZipPackRec) * ((size_t)cnt + 1), hipMemcpyHostToDevice, g.stream));
      Timed t("k_zip_pack");
      hipLaunchKernelGGL(k_zip_pack, dim3(wgs), dim3(GZ_GATHER_THREADS), 0, g.stream, d_in, (const uint8_t*)g.gz_bodies.p, (const uint8_t*)g.gz_tab.p, d_out,
                         (const ZesZipPackRec*)d_recs, cnt);
    }
    HIPCHK(hipGetLastError());
    rpos += (size_t)cnt + 1;
    e0 += cnt;
  }
  // the directory and the end record
  const uint64_t cd_off = total;
  cd.reserve((size_t)count * 46 + name_off[count] + ZIP_END);
  for (uint32_t i = 0; i < count; i++) {
    zes_zip_entry& t = z[i];
    const size_t at = cd.size();
    cd.resize(at + 46 + t.name_len, 0);
    uint8_t* r = &cd[at];
    put_le32(r, 0x02014b50u);
    put_le16(r + 4, 20);
    put_le16(r + 6, 20);
    put_le16(r + 8, t.flags);
    put_le16(r + 10, t.method);
    put_le16(r + 14, 33);  // 1980-01-01, time 0
    put_le32(r + 16, t.crc);
    put_le32(r + 20, t.csize);
    put_le32(r + 24, t.usize);
    put_le16(r + 28, t.name_len);
    put_le32(r + 42, (uint32_t)t.hdr_off);
    if (t.name_len) memcpy(r + 46, names + t.name_off, t.name_len);
    t.name_pos = cd_off + at + 46;
  }
  const uint64_t cd_size = cd.size();
  if (cd_off >= 0xFFFFFFFFull || cd_size >= 0xFFFFFFFFull) return ZES_E_UNSUPPORTED;
  cd.resize((size_t)cd_size + ZIP_END);
  zip_end_record(&cd[(size_t)cd_size], count, cd_size, cd_off);
  total += cd.size();
  if (eg.room(total, cap, d_out)) HIPCHK(hipMemcpyAsync(d_out + cd_off, cd.data(), cd.size(), hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  *out_len = total;
  if (!eg.fits) return ZES_E_NOSPACE;
  if (ent && count) memcpy(ent, z.data(), sizeof(zes_zip_entry) * (size_t)count);
  return ZES_OK;
}

int zes_zipwrite_bound(const uint64_t* in_len, const uint16_t* name_len, uint32_t count, uint64_t* cap) {
  if (!cap || (count && (!in_len || !name_len))) return ZES_E_ARG;
  *cap = zipwrite_bound(in_len, name_len, count);
  return ZES_OK;
}

int zes_zipwrite_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, const uint8_t* names, const uint16_t* name_len, uint32_t count,
                     uint8_t* d_out, uint64_t cap, uint64_t* out_len, zes_zip_entry* ent, uint32_t flags) {
  ROUTE_DEV(d_out, d_in);
  if (count && !in_off) return ZES_E_ARG;
  if (const int arc = zipwrite_args([&](uint32_t) { return d_in != nullptr; }, in_len, names, name_len, count, d_out, cap, out_len, flags)) return arc;
  LOCK_READY();
  rc = zipwrite_core(d_in, in_off, in_len, names, name_len, count, d_out, cap, out_len, ent, flags);
  return call_done(rc, rc != ZES_E_NOSPACE);  // (ZES_E_NOSPACE is an answer, not a failure)
}

int zes_zipwrite(const uint8_t* const* in, const uint64_t* in_len, const uint8_t* names, const uint16_t* name_len, uint32_t count, uint8_t* out, uint64_t cap,
                 uint64_t* out_len, zes_zip_entry* ent, uint32_t flags) {
  UseDev ud(route_host());
  if (count && !in) return ZES_E_ARG;
  if (const int arc = zipwrite_args([&](uint32_t i) { return in[i] != nullptr; }, in_len, names, name_len, count, out, cap, out_len, flags)) return arc;
  if (count == 0) {  // the end record alone: nothing to compute
    *out_len = ZIP_END;
    if (cap < ZIP_END) return ZES_E_NOSPACE;
    zip_end_record(out, 0, 0, 0);
    return ZES_OK;
  }
  LOCK_READY();
  HostBatch hb(g.gz_in, g.gz_acc);
  std::vector<uint64_t> in_off(count);
  for (uint32_t i = 0; i < count; i++) in_off[i] = hb.place(in[i], in_len[i]);
  const uint64_t bound = zipwrite_bound(in_len, name_len, count);
  hb.room(bound);  // (the archive: one place)
  if ((rc = hb.up())) return rc;
  uint64_t total = 0;
  std::vector<zes_zip_entry> z(ent ? count : 0);
  rc = zipwrite_core(hb.d_in(), in_off.data(), in_len, names, name_len, count, hb.d_out(), bound, &total, ent ? z.data() : nullptr, flags);
  if ((rc = call_done(rc, true))) return rc;
  *out_len = total;
  if (total > cap) return ZES_E_NOSPACE;
  if ((rc = download(out, hb.d_out(), total))) return rc;
  if (ent) memcpy(ent, z.data(), sizeof(zes_zip_entry) * (size_t)count);
  return ZES_OK;
}

// ---- PNG images (include/zes.h: "PNG images"): the file rule, and batch decoding through it ----
constexpr uint32_t PNG_IHDR = 0x49484452u, PNG_IDAT = 0x49444154u, PNG_PLTE = 0x504c5445u, PNG_IEND = 0x49454e44u, PNG_TRNS = 0x74524e53u;

static uint32_t png_channels(uint32_t colour) { return colour == 2 ? 3u : colour == 4 ? 2u : colour == 6 ? 4u : 1u; }
static uint64_t png_rowbytes(uint32_t width, uint32_t colour, uint32_t depth) { return ((uint64_t)width * (png_channels(colour) * depth) + 7) / 8; }
static uint64_t png_rowbytes(const ZesPngHead& h) { return png_rowbytes(h.width, h.colour, h.depth); }

// The file rule on p[0, c), stated once for the host forms (k_png_walk restates it for files in device memory): the verdict,
// h filled as far as the walk got, and every chunk that passes the chain's tests handed to each().
static int png_rule(const uint8_t* p, uint64_t c, ZesPngHead& h, const std::function<void(const ZesPngChunk&)>& each) {
  memset(&h, 0, sizeof h);
  static const uint8_t sig[8] = {0x89, 0x50, 0x4e, 0x47, 0x0d, 0x0a, 0x1a, 0x0a};
  if (c < 8 || memcmp(p, sig, 8)) return ZES_E_PNG;
  uint64_t pos = 8;
  bool idat = false, closed = false, plte = false, trns = false;
  const uint64_t steps = c / 12;  // a chunk takes 12 bytes at least
  for (uint64_t s = 0; s < steps; s++) {
    if (c - pos < 12) return ZES_E_PNG;  // (pos == c: the chain ends without IEND)
    const uint32_t L = get_be32(p + pos), type = get_be32(p + pos + 4);
    if (L > 0x7fffffffu) return ZES_E_PNG;
    for (uint32_t b = 0; b < 4; b++) {
      const uint32_t ch = (type >> (8 * b)) & 255u;
      if (!((ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'))) return ZES_E_PNG;
    }
    if (L > c - pos - 12) return ZES_E_PNG;
    const uint8_t* d = p + pos + 8;
    each(ZesPngChunk{pos, L | (type == PNG_IDAT ? ZES_PNG_IDAT : 0u), get_be32(d + L)});
    if (++h.nchunks == 1) {
      if (type != PNG_IHDR || L != 13) return ZES_E_PNG;
      h.width = get_be32(d);
      h.height = get_be32(d + 4);
      h.depth = d[8];
      h.colour = d[9];
      h.interlace = d[12];
      if (h.width < 1 || h.width > 0x7fffffffu || h.height < 1 || h.height > 0x7fffffffu) return ZES_E_PNG;
      const uint32_t dp = h.depth;
      bool ok = false;
      if (h.colour == 0) ok = dp == 1 || dp == 2 || dp == 4 || dp == 8 || dp == 16;
      else if (h.colour == 3) ok = dp == 1 || dp == 2 || dp == 4 || dp == 8;
      else if (h.colour == 2 || h.colour == 4 || h.colour == 6) ok = dp == 8 || dp == 16;
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
        return 1 + png_rowbytes(h) > 0xFFFFFFFFull / h.height ? ZES_E_UNSUPPORTED : ZES_OK;
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

// the caller's record of a file that passed the rule (h.status == ZES_OK); zeros for any other
static void png_info_of(const ZesPngHead& h, zes_png_info* o) {
  memset(o, 0, sizeof *o);
  if (h.status != ZES_OK) return;
  o->width = h.width, o->height = h.height;
  o->depth = h.depth, o->colour = h.colour, o->interlace = h.interlace;
  o->channels = (uint8_t)png_channels(h.colour);
  o->bpp = (uint8_t)std::max<uint32_t>(1, o->channels * h.depth / 8);
  o->rowbytes = png_rowbytes(h);
  o->out_size = h.height * o->rowbytes;
  o->idat_count = h.idat_count, o->idat_bytes = h.idat_bytes;
  o->plte_pos = h.plte_pos, o->plte_len = h.plte_len;
  o->trns_pos = h.trns_pos, o->trns_len = h.trns_len;
}

int zes_png_info_get(const uint8_t* in, uint64_t c, zes_png_info* info, uint32_t flags) {
  if (!info || flags || (!in && c)) return ZES_E_ARG;
  ZesPngHead h;
  h.status = png_rule(in, c, h, [](const ZesPngChunk&) {});
  png_info_of(h, info);
  return h.status;
}

// An Adam7 image's seven passes (include/zes.h: "Interlaced images"): pass p + 1 has ph[p] rows of prb[p] bytes behind a filter
// byte each (both 0 for a pass without pixels, which has no byte in the stream); Fi is what the stream inflates to.  Where
// the unfiltered passes stand in the image's slot of g.png_passes: off[p], each on a 16-byte boundary; the slot is padded
struct PngPasses {
  uint32_t ph[7];
  uint64_t prb[7], off[7];
  uint64_t Fi, slot;
};
static PngPasses png_passes_of(const ZesPngHead& h) {
  static const uint8_t x0[7] = {0, 4, 0, 2, 0, 1, 0}, y0[7] = {0, 0, 4, 0, 2, 0, 1}, sx[7] = {3, 3, 2, 2, 1, 1, 0}, sy[7] = {3, 3, 3, 2, 2, 1, 1};
  const uint64_t bits = png_channels(h.colour) * h.depth;
  PngPasses a;
  a.Fi = a.slot = 0;
  for (int p = 0; p < 7; p++) {
    uint64_t pw = h.width > x0[p] ? ((uint64_t)(h.width - x0[p]) + (1u << sx[p]) - 1) >> sx[p] : 0;
    uint64_t ph = h.height > y0[p] ? ((uint64_t)(h.height - y0[p]) + (1u << sy[p]) - 1) >> sy[p] : 0;
    if (!pw || !ph) pw = ph = 0;
    a.ph[p] = (uint32_t)ph;
    a.prb[p] = (pw * bits + 7) / 8;
    a.off[p] = a.slot;
    a.Fi += ph * (1 + a.prb[p]);  // (at most the file rule's F a pass: no overflow)
    a.slot += gz_up16(ph * a.prb[p]);
  }
  a.slot += 16;
  return a;
}

// One file of a png_decode_core batch: what the walk says about it, its chunks (when it passed the rule), where its first
// byte lies in d_src and where its out_size bytes go in dst
struct PngImg {
  ZesPngHead h;
  std::vector<ZesPngChunk> ch;
  uint64_t src_at = 0, dst_off = 0;
};

// The share of the chunk table the first walk gives a file of n bytes: sized from the arguments alone
static uint32_t png_tab_share(uint64_t n) { return (uint32_t)std::min<uint64_t>(n / 12, 16 + n / 4096); }

// k_png_walk over the files d_src[in_off[i], + in_len[i]): heads and chunks of all of them into im.  The table goes through
// g.gz_tab as files | heads | chunks; one launch and one read-back, and both once more with exact shares when a file that
// passed the rule had more chunks than its share.
static int png_walk_dev(const uint8_t* d_src, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, std::vector<PngImg>& im) {
  int rc;
  std::vector<ZesPngFile> files(count);
  std::vector<uint8_t> back;
  Drain drain;  // (behind files, which an upload reads, and back, which the read-back writes)
  for (uint32_t i = 0; i < count; i++) files[i] = ZesPngFile{in_off[i], in_len[i], 0u, png_tab_share(in_len[i])};
  for (int round = 0; round < 2; round++) {
    uint64_t total = 0;
    for (ZesPngFile& f : files) {
      if (total + f.tab_cap > 0xFFFFFFFFull) return ZES_E_ARG;
      f.tab_base = (uint32_t)total;
      total += f.tab_cap;
    }
    const size_t o_head = sizeof(ZesPngFile) * (size_t)count, o_tab = o_head + sizeof(ZesPngHead) * (size_t)count;
    const size_t bytes = o_tab + sizeof(ZesPngChunk) * (size_t)total;
    if ((rc = ensure(g.gz_tab, bytes))) return rc;
    uint8_t* base = (uint8_t*)g.gz_tab.p;
    HIPCHK(hipMemcpyAsync(base, files.data(), o_head, hipMemcpyHostToDevice, g.stream));
    {
      Timed t("k_png_walk");
      hipLaunchKernelGGL(k_png_walk, dim3((count + 63) / 64), dim3(64), 0, g.stream, d_src, (const ZesPngFile*)base, count, (ZesPngHead*)(base + o_head),
                         (ZesPngChunk*)(base + o_tab));
    }
    HIPCHK(hipGetLastError());
    back.resize(bytes - o_head);
    HIPCHK(hipMemcpyAsync(back.data(), base + o_head, bytes - o_head, hipMemcpyDeviceToHost, g.stream));
    HIPCHK(hipStreamSynchronize(g.stream));
    const ZesPngHead* heads = (const ZesPngHead*)back.data();
    bool again = false;
    for (uint32_t i = 0; i < count; i++) {
      again = again || (heads[i].status == ZES_OK && heads[i].nchunks > files[i].tab_cap);
      files[i].tab_cap = heads[i].status == ZES_OK ? heads[i].nchunks : 0u;
    }
    if (!again) {
      const ZesPngChunk* tab = (const ZesPngChunk*)(back.data() + (o_tab - o_head));
      for (uint32_t i = 0; i < count; i++) {
        im[i].h = heads[i];
        if (heads[i].status == ZES_OK) im[i].ch.assign(tab + files[i].tab_base, tab + files[i].tab_base + heads[i].nchunks);
      }
      drain.done();  // (behind the round's synchronisation)
      return ZES_OK;
    }
  }
  return ZES_E_DEVICE;  // (the second launch counts what the first one counted)
}

// The images of im whose status[k] is ZES_OK on entry (rule, interlace and capacity have passed them): steps 2 to 4 of
// include/zes.h, every step one launch sequence for the batch.  status[k] becomes the image's status.  An interlaced image
// (it is here only under ZES_F_PNG_INTERLACED) takes the same steps with its seven passes as seven images of step 4, which go
// to a slot of g.png_passes, and step 4b behind it: k_png_deinterlace from there to the image's place.  `more`: the caller
// launches on g.stream behind this and synchronises there (pngpix_core), so step 4b, which brings nothing back, does not.
static int png_decode_core(const uint8_t* d_src, const std::vector<PngImg>& im, uint8_t* dst, int32_t* status, uint32_t flags, bool more = false) {
  int rc;
  g.last_tier = 0;
  const uint32_t n = (uint32_t)im.size();
  // what copies queued on the stream read (step 2's segments through the checksum's upload, step 3's through gz_gather's,
  // step 4's jobs) or write (step 4's read-back), and the guard behind them
  std::vector<ZesCrcSeg> csegs;
  std::vector<ZesGzSeg> segs;
  std::vector<ZesPngJob> uj;
  std::vector<ZesPngDeintJob> dj;
  std::vector<uint8_t> table;
  std::vector<uint32_t> bad;
  Drain drain;
  // 2. chunk CRCs: type and data of every chunk
  {
    for (uint32_t k = 0; k < n; k++)
      if (status[k] == ZES_OK)
        for (const ZesPngChunk& c : im[k].ch) csegs.push_back(ZesCrcSeg{im[k].src_at + c.pos + 4, 4ull + (c.len & ~ZES_PNG_IDAT)});
    if (csegs.size() > 0x7fffffffull) return ZES_E_ARG;
    std::vector<uint32_t> crc(csegs.size());
    if (!csegs.empty() && (rc = crc32_batch_locked(d_src, csegs.data(), (uint32_t)csegs.size(), crc.data()))) return rc;
    size_t q = 0;
    for (uint32_t k = 0; k < n; k++)
      if (status[k] == ZES_OK)
        for (const ZesPngChunk& c : im[k].ch)
          if (crc[q++] != c.crc) status[k] = ZES_E_CHECKSUM;
  }
  // 3. the zlib streams: gathered, decoded, their lengths and trailers checked
  std::vector<uint32_t> who;
  std::vector<InfJob> jobs;
  std::vector<uint64_t> filtered;
  uint64_t ipos = 0, opos = 0;
  for (uint32_t k = 0; k < n; k++) {
    if (status[k] != ZES_OK) continue;
    const ZesPngHead& h = im[k].h;
    const uint64_t F = h.interlace ? png_passes_of(h).Fi : h.height * (1 + png_rowbytes(h));
    uint64_t at = ipos;
    for (const ZesPngChunk& c : im[k].ch)
      if ((c.len & ZES_PNG_IDAT) && (c.len & ~ZES_PNG_IDAT)) {
        segs.push_back(ZesGzSeg{im[k].src_at + c.pos + 8, at, c.len & ~ZES_PNG_IDAT, 0u, 0u});
        at += c.len & ~ZES_PNG_IDAT;
      }
    InfJob j{ipos, h.idat_bytes, opos, gz_slot_cap(F), 0, ZES_OK, 0};
    j.want_end = true;
    jobs.push_back(j);
    who.push_back(k);
    filtered.push_back(F);
    ipos += gz_slot_in(h.idat_bytes);
    opos += gz_slot_out(F);
  }
  if (jobs.empty()) {
    drain.done();  // (step 2 ends in its read-back)
    return ZES_OK;
  }
  if ((rc = ensure(g.gz_bodies, ipos + 64)) || (rc = ensure(g.gz_outs, opos + 64))) return rc;
  if ((rc = gz_gather(d_src, (uint8_t*)g.gz_bodies.p, segs))) return rc;
  if ((rc = inflate_jobs((const uint8_t*)g.gz_bodies.p, (uint8_t*)g.gz_outs.p, jobs, nullptr, flags & ZES_F_PIECES))) return rc;
  for (size_t q = 0; q < jobs.size(); q++)
    if (jobs[q].status == ZES_E_NOSPACE || (jobs[q].status == ZES_OK && jobs[q].out_len != filtered[q])) jobs[q].status = ZES_E_PNG;
  if ((rc = check_adler_jobs((const uint8_t*)g.gz_bodies.p, nullptr, (const uint8_t*)g.gz_outs.p, jobs))) return rc;
  keep_times();
  // 4. the filters
  std::vector<uint32_t> uw, dw;
  uint64_t bands = 0, tiles = 0, pass_at = 0;
  for (size_t q = 0; q < jobs.size(); q++) {
    const uint32_t k = who[q];
    status[k] = jobs[q].status;
    if (status[k] != ZES_OK) continue;
    const ZesPngHead& h = im[k].h;
    const uint32_t depth_bits = png_channels(h.colour) * h.depth, bpp = std::max<uint32_t>(1, depth_bits / 8);
    if (!h.interlace) {
      uj.push_back(ZesPngJob{jobs[q].out_off, im[k].dst_off, h.height, (uint32_t)png_rowbytes(h), bpp, (uint32_t)bands});
      uw.push_back(k);
      bands += (h.height + ZES_PNG_BAND - 1) / ZES_PNG_BAND;
    } else {  // a job per pass that has pixels, and the record of step 4b
      const PngPasses a = png_passes_of(h);
      ZesPngDeintJob d;
      memset(&d, 0, sizeof d);
      d.src_off = pass_at, d.dst_off = im[k].dst_off;
      d.width = h.width, d.height = h.height, d.rowbytes = (uint32_t)png_rowbytes(h), d.bits = depth_bits;
      d.tile_rows = std::min(h.height, std::max(1u, ZES_PNGD_TILE_BYTES / d.rowbytes));
      d.first_tile = (uint32_t)tiles;
      d.ujob0 = (uint32_t)uj.size();
      uint64_t from = jobs[q].out_off;
      for (int p = 0; p < 7; p++) {
        d.pass_off16[p] = (uint32_t)(a.off[p] / 16);
        if (!a.ph[p]) continue;
        uj.push_back(ZesPngJob{from, pass_at + a.off[p], a.ph[p], (uint32_t)a.prb[p], bpp | ZES_PNG_TO_PASSES, (uint32_t)bands});
        uw.push_back(k);
        bands += (a.ph[p] + ZES_PNG_BAND - 1) / ZES_PNG_BAND;
        from += a.ph[p] * (1 + a.prb[p]);
      }
      d.ujobs = (uint32_t)uj.size() - d.ujob0;
      dj.push_back(d);
      dw.push_back(k);
      tiles += (h.height + d.tile_rows - 1) / d.tile_rows;
      pass_at += a.slot;
    }
    if (bands > 0x7fffffffull || tiles > 0x7fffffffull || uj.size() > 0x7fffffffull) return ZES_E_ARG;
  }
  if (uj.empty()) {
    drain.done();  // (inflate_jobs has brought the jobs' results down: the stream is past segs)
    return ZES_OK;
  }
  // one table, one upload: the unfilter jobs, the deinterlace jobs behind them, then the jobs' `bad` words
  const size_t o_dj = sizeof(ZesPngJob) * uj.size(), o_bad = o_dj + sizeof(ZesPngDeintJob) * dj.size();
  table.resize(o_bad);
  memcpy(table.data(), uj.data(), o_dj);
  if (!dj.empty()) memcpy(table.data() + o_dj, dj.data(), o_bad - o_dj);
  if ((rc = ensure(g.gz_tab, o_bad + 4 * uj.size()))) return rc;
  if (pass_at && (rc = ensure(g.png_passes, pass_at + 64))) return rc;
  uint32_t* d_bad = (uint32_t*)((uint8_t*)g.gz_tab.p + o_bad);
  HIPCHK(hipMemcpyAsync(g.gz_tab.p, table.data(), o_bad, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemsetAsync(d_bad, 0, 4 * uj.size(), g.stream));
  {
    Timed t("k_png_unfilter");
    constexpr uint32_t per = ZES_PNG_UNF_THREADS / 64u;
    hipLaunchKernelGGL(k_png_unfilter, dim3((uint32_t)((bands + per - 1) / per)), dim3(ZES_PNG_UNF_THREADS), 0, g.stream, (const uint8_t*)g.gz_outs.p, dst,
                       (uint8_t*)g.png_passes.p, (const ZesPngJob*)g.gz_tab.p, (uint32_t)uj.size(), (uint32_t)bands, d_bad);
  }
  HIPCHK(hipGetLastError());
  bad.resize(uj.size());
  HIPCHK(hipMemcpyAsync(bad.data(), d_bad, 4 * uj.size(), hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();  // (the table has gone up and the words have come down: nothing queued reads or writes host memory now)
  for (size_t q = 0; q < uj.size(); q++)
    if (bad[q]) status[uw[q]] = ZES_E_PNG;
  // 4b. the passes of the interlaced images gathered into scanlines: the table is already there, and the tiles of an image
  // that has a `bad` word set are launched with the others and exit on reading it
  bool gather = false;
  for (const uint32_t k : dw) gather = gather || status[k] == ZES_OK;
  if (gather) {
    {
      Timed t("k_png_deinterlace");
      hipLaunchKernelGGL(k_png_deinterlace, dim3((uint32_t)tiles), dim3(ZES_PNGD_THREADS), 0, g.stream, (const uint8_t*)g.png_passes.p, dst,
                         (const ZesPngDeintJob*)((const uint8_t*)g.gz_tab.p + o_dj), (uint32_t)dj.size(), (const uint32_t*)d_bad);
    }
    HIPCHK(hipGetLastError());
    if (!more) HIPCHK(hipStreamSynchronize(g.stream));
  }
  return ZES_OK;
}
static_assert(sizeof(ZesPngJob) == 32 && sizeof(ZesPngDeintJob) == 80, "the step-4 table: 8-byte aligned records back to back");

// zes_png_decode*: what both forms check before anything else
static int png_decode_args(bool arrays, const uint64_t* out_len, const int32_t* status, uint32_t count, uint32_t flags) {
  if (flags & ~(ZES_F_PIECES | ZES_F_PNG_INTERLACED)) return ZES_E_ARG;
  if (count && (!arrays || !out_len || !status)) return ZES_E_ARG;
  return ZES_OK;
}

// Step 1 behind the walk, for image i: the rule's verdict, then interlace (refused without ZES_F_PNG_INTERLACED; with it, the
// seven passes' filtered size has the bound the rule sets for a plain image's); the caller's records filled
static void png_judge(const PngImg& m, uint32_t i, uint64_t* out_len, int32_t* status, zes_png_info* info, zes_png_info* mine, uint32_t flags) {
  png_info_of(m.h, mine);
  if (info) info[i] = *mine;
  out_len[i] = 0;
  status[i] = m.h.status;
  if (status[i] == ZES_OK && m.h.interlace && (!(flags & ZES_F_PNG_INTERLACED) || png_passes_of(m.h).Fi > 0xFFFFFFFFull)) status[i] = ZES_E_UNSUPPORTED;
}

// ---- step 5 of zes_pngpix* (include/zes.h: "The conversion rule"), which zes_pngpix_expand_dev runs alone ----
// What k_png_expand is told about one image, and the tiles it takes behind *tiles.  The rule's reading of tRNS: a length that
// does not fit the colour type counts as none
static ZesPngxJob pngx_job(uint32_t width, uint32_t height, uint32_t colour, uint32_t depth, uint32_t plte_len, uint64_t trns_len, uint64_t* tiles) {
  ZesPngxJob j;
  memset(&j, 0, sizeof j);
  j.width = width, j.height = height, j.rowbytes = (uint32_t)png_rowbytes(width, colour, depth);
  j.depth = (uint8_t)depth, j.colour = (uint8_t)colour;
  j.plte_len = colour == 3 ? (uint16_t)std::min<uint32_t>(plte_len, 768) : 0;
  const bool fits = colour == 0 ? trns_len == 2 : colour == 2 ? trns_len == 6 : colour == 3 && trns_len <= plte_len / 3;
  j.trns_len = fits ? (uint16_t)trns_len : 0;
  j.tile_rows = std::min(height, std::max(1u, ZES_PNGX_TILE_PIXELS / width));
  j.first_tile = (uint32_t)*tiles;
  *tiles += (height + j.tile_rows - 1) / j.tile_rows;
  return j;
}
static_assert(sizeof(ZesPngxJob) == 64, "ZesPngxJob is 64 bytes");
static uint64_t png_pix_size(uint32_t width, uint32_t height) { return 4ull * width * height; }

// One k_png_expand launch over `table`: njobs records and, behind them, the PLTE and tRNS bytes that came from the host (none
// when d_aux is given: the jobs then point into those bytes, the files).  One upload into g.gz_tab, one launch; the
// synchronisation ends the call's device work.  `table` is the caller's and outlives this function.
static int pngx_run(const uint8_t* d_lines, const uint8_t* d_aux, uint8_t* d_out, const std::vector<uint8_t>& table, uint32_t njobs, uint64_t tiles) {
  int rc;
  if (tiles > 0x7fffffffull) return ZES_E_ARG;
  if ((rc = ensure(g.gz_tab, table.size() + 16))) return rc;
  Drain drain;
  HIPCHK(hipMemcpyAsync(g.gz_tab.p, table.data(), table.size(), hipMemcpyHostToDevice, g.stream));
  {
    Timed t("k_png_expand");
    hipLaunchKernelGGL(k_png_expand, dim3((uint32_t)tiles), dim3(ZES_PNGX_THREADS), 0, g.stream, d_lines,
                       d_aux ? d_aux : (const uint8_t*)g.gz_tab.p + sizeof(ZesPngxJob) * (size_t)njobs, d_out, (const ZesPngxJob*)g.gz_tab.p, njobs);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  return ZES_OK;
}

// Steps 2 to 5 of zes_pngpix* for the images whose status[k] is ZES_OK on entry, im[k].dst_off the place of their pixels in
// dst: png_decode_core with a padded slot of g.png_lines as every image's place, then the pixels of those that came through
static int pngpix_core(const uint8_t* d_src, std::vector<PngImg>& im, uint8_t* dst, int32_t* status, uint32_t flags) {
  int rc;
  const uint32_t n = (uint32_t)im.size();
  std::vector<uint64_t> pix_off(n);
  uint64_t at = 0;
  for (uint32_t k = 0; k < n; k++) {
    pix_off[k] = im[k].dst_off;
    if (status[k] != ZES_OK) continue;
    im[k].dst_off = at;
    at += gz_up16(im[k].h.height * png_rowbytes(im[k].h)) + 16;
  }
  if (at && (rc = ensure(g.png_lines, at + 64))) return rc;
  // The pixel forms launch the same kernels for one image as for many: a single stream's block chain is followed by
  // k_inf_chain as a batch's is, not on the host (a kernel of about 11 us; the design point is a batch)
  g.device_chain = true;
  rc = png_decode_core(d_src, im, (uint8_t*)g.png_lines.p, status, flags, true);  // (an image at ZES_OK behind it: pngx_run synchronises)
  g.device_chain = false;
  if (rc) return rc;
  std::vector<uint8_t> table;
  uint64_t tiles = 0;
  uint32_t njobs = 0;
  for (uint32_t k = 0; k < n; k++) {
    if (status[k] != ZES_OK) continue;
    const ZesPngHead& h = im[k].h;
    ZesPngxJob j = pngx_job(h.width, h.height, h.colour, h.depth, h.plte_len, h.trns_len, &tiles);
    j.src_off = im[k].dst_off, j.dst_off = pix_off[k];
    j.plte_off = im[k].src_at + h.plte_pos, j.trns_off = im[k].src_at + h.trns_pos;
    table.insert(table.end(), (const uint8_t*)&j, (const uint8_t*)&j + sizeof j);
    njobs++;
  }
  return njobs ? pngx_run((const uint8_t*)g.png_lines.p, d_src, dst, table, njobs, tiles) : ZES_OK;
}

// The device forms: zes_png_decode_dev, and with `pix` zes_pngpix_dev — the same steps and statuses, the size an image needs
// and the core behind step 1 apart
static int png_dev_form(bool pix, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out,
                        const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, zes_png_info* info, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (const int arc = png_decode_args(in_off && in_len && out_off && out_cap, out_len, status, count, flags)) return arc;
  for (uint32_t i = 0; i < count; i++)
    if (in_len[i] && !d_in) return ZES_E_ARG;
  if (!count) {
    call_none();
    return ZES_OK;
  }
  LOCK_READY();
  std::vector<PngImg> im(count);
  if ((rc = png_walk_dev(d_in, in_off, in_len, count, im))) return call_done(rc, true);
  bool null_out = false;
  for (uint32_t i = 0; i < count; i++) {
    zes_png_info mine;
    png_judge(im[i], i, out_len, status, info, &mine, flags);
    im[i].src_at = in_off[i];
    im[i].dst_off = out_off[i];
    if (status[i] != ZES_OK) continue;
    out_len[i] = pix ? png_pix_size(mine.width, mine.height) : mine.out_size;
    if (out_cap[i] < out_len[i]) status[i] = ZES_E_NOSPACE;
    else null_out = null_out || !d_out;
  }
  if (null_out) return call_done(ZES_E_ARG, true);
  if ((rc = call_done(pix ? pngpix_core(d_in, im, d_out, status, flags) : png_decode_core(d_in, im, d_out, status, flags), true))) return rc;
  for (uint32_t i = 0; i < count; i++)
    if (status[i] != ZES_OK && status[i] != ZES_E_NOSPACE) out_len[i] = 0;
  return ZES_OK;
}

// The alloc forms: zes_png_decode_alloc, and with `pix` zes_pngpix_alloc
static int png_alloc_form(bool pix, const uint8_t* const* in, const uint64_t* in_len, uint32_t count, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                          int32_t* status, zes_png_info* info, uint32_t flags) {
  UseDev ud(route_host());
  if (const int arc = png_decode_args(in && in_len, out_len, status, count, flags)) return arc;
  if (!alloc) return ZES_E_ARG;
  for (uint32_t i = 0; i < count; i++)
    if (in_len[i] && !in[i]) return ZES_E_ARG;
  if (!count) {
    call_none();
    return ZES_OK;
  }
  // the rule on the caller's memory: a batch in which no file passes touches no device
  std::vector<PngImg> im(count);
  std::vector<uint64_t> size(count, 0);
  bool any = false;
  for (uint32_t i = 0; i < count; i++) {
    PngImg& m = im[i];
    m.h.status = png_rule(in[i], in_len[i], m.h, [&](const ZesPngChunk& c) { m.ch.push_back(c); });
    zes_png_info mine;
    png_judge(m, i, out_len, status, info, &mine, flags);
    if (status[i] != ZES_OK) continue;
    any = true;
    size[i] = pix ? png_pix_size(mine.width, mine.height) : mine.out_size;
  }
  if (!any) {
    call_none();
    return ZES_OK;
  }
  LOCK_READY();
  HostBatch hb(g.gz_in, g.gz_acc);
  std::vector<uint64_t> place(count, 0);
  for (uint32_t i = 0; i < count; i++)
    if (status[i] == ZES_OK) {
      im[i].src_at = hb.place(in[i], in_len[i]);
      im[i].dst_off = place[i] = hb.room(size[i]);
    }
  if ((rc = hb.up())) return rc;
  if ((rc = call_done(pix ? pngpix_core(hb.d_in(), im, hb.d_out(), status, flags) : png_decode_core(hb.d_in(), im, hb.d_out(), status, flags), true))) return rc;
  return hb.hand_out(count, alloc, user, status, out_len, [&](uint32_t i) { return size[i]; }, [&](uint32_t i) { return place[i]; });
}

int zes_png_decode_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out, const uint64_t* out_off,
                       const uint64_t* out_cap, uint64_t* out_len, int32_t* status, zes_png_info* info, uint32_t flags) {
  return png_dev_form(false, d_in, in_off, in_len, count, d_out, out_off, out_cap, out_len, status, info, flags);
}
int zes_png_decode_alloc(const uint8_t* const* in, const uint64_t* in_len, uint32_t count, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                         int32_t* status, zes_png_info* info, uint32_t flags) {
  return png_alloc_form(false, in, in_len, count, alloc, user, out_len, status, info, flags);
}
int zes_pngpix_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out, const uint64_t* out_off,
                   const uint64_t* out_cap, uint64_t* out_len, int32_t* status, zes_png_info* info, uint32_t flags) {
  return png_dev_form(true, d_in, in_off, in_len, count, d_out, out_off, out_cap, out_len, status, info, flags);
}
int zes_pngpix_alloc(const uint8_t* const* in, const uint64_t* in_len, uint32_t count, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                     int32_t* status, zes_png_info* info, uint32_t flags) {
  return png_alloc_form(true, in, in_len, count, alloc, user, out_len, status, info, flags);
}

// ---- TIFF reader (include/zes.h: "zes_tiff_*"): the file rule on the host, the touched segments through inflate_jobs as one
// batch, the pixels by k_tiff_place ----
// What the rule says about one directory of a file: the record, the segment arrays, the chain's length
struct TiffIndex {
  zes_tiff_image im;
  std::vector<uint64_t> off, len;
  uint32_t dirs = 0;
};
// fetch(pos, len): the file's bytes [pos, pos + len), which the rule has checked to lie inside the file, valid until the rule
// returns; null when they cannot be had (the device form's copy failed: *frc says how)
using TiffFetch = std::function<const uint8_t*(uint64_t, uint64_t)>;

static uint64_t tiff_ps(const zes_tiff_image& m) { return (uint64_t)m.spp * (m.bits / 8u); }
static uint64_t tiff_ceil(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
// the rows of the segments of segment row sy, and the decoded size of one of them (step 2 of include/zes.h)
static uint32_t tiff_seg_rows(const zes_tiff_image& m, uint32_t sy) {
  return m.tiled ? m.seg_h : (uint32_t)std::min<uint64_t>(m.seg_h, m.height - (uint64_t)sy * m.seg_h);
}
static uint64_t tiff_seg_size(const zes_tiff_image& m, uint32_t sy) { return (uint64_t)m.seg_w * tiff_seg_rows(m, sy) * tiff_ps(m); }

// The file rule of include/zes.h on a file of c bytes, directory `dir`: the verdict; x.dirs is filled once the chain has been
// walked, the rest of x with ZES_OK only
static int tiff_rule(uint64_t c, uint32_t dir, const TiffFetch& fetch, const int* frc, TiffIndex& x) {
  memset(&x.im, 0, sizeof x.im);
  x.off.clear();
  x.len.clear();
  x.dirs = 0;
  // header
  if (c < 8) return ZES_E_TIFF;
  const uint8_t* h = fetch(0, 8);
  if (!h) return *frc;
  if (!((h[0] == 0x49 && h[1] == 0x49) || (h[0] == 0x4d && h[1] == 0x4d))) return ZES_E_TIFF;
  const bool be = h[0] == 0x4d;
  auto u16 = [be](const uint8_t* p) { return be ? (uint32_t)p[0] << 8 | p[1] : (uint32_t)p[1] << 8 | p[0]; };
  auto u32 = [be](const uint8_t* p) {
    return be ? (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3] : (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0];
  };
  if (u16(h + 2) == 43) return ZES_E_UNSUPPORTED;
  if (u16(h + 2) != 42) return ZES_E_TIFF;
  // chain
  uint64_t o = u32(h + 4), at = 0;
  uint32_t n_at = 0, dirs = 0;
  while (o) {
    if (dirs >= 65536 || o < 8 || o + 2 > c) return ZES_E_TIFF;
    const uint8_t* p = fetch(o, 2);
    if (!p) return *frc;
    const uint32_t n = u16(p);
    if (o + 2 + 12ull * n + 4 > c) return ZES_E_TIFF;
    if (dirs == dir) at = o, n_at = n;
    if (!(p = fetch(o + 2 + 12ull * n, 4))) return *frc;
    o = u32(p);
    dirs++;
  }
  x.dirs = dirs;
  if (dir >= dirs) return ZES_E_ARG;
  // entries
  struct Tag {
    uint32_t id;
    bool have = false;
    uint32_t type = 0, count = 0;
    uint64_t pos = 0;
    explicit Tag(uint32_t i) : id(i) {}
  };
  Tag t_w(256), t_h(257), t_bits(258), t_comp(259), t_photo(262), t_fill(266), t_soff(273), t_spp(277), t_rps(278), t_slen(279), t_planar(284), t_pred(317),
      t_tw(322), t_tl(323), t_toff(324), t_tlen(325), t_extra(338), t_fmt(339);
  Tag* const used[] = {&t_w, &t_h, &t_bits, &t_comp, &t_photo, &t_fill, &t_soff, &t_spp, &t_rps, &t_slen, &t_planar, &t_pred, &t_tw, &t_tl, &t_toff, &t_tlen,
                       &t_extra, &t_fmt};
  const uint8_t* ents = n_at ? fetch(at + 2, 12ull * n_at) : h;
  if (!ents) return *frc;
  for (uint32_t i = 0; i < n_at; i++) {
    const uint8_t* e = ents + 12ull * i;
    const uint32_t id = u16(e);
    for (Tag* t : used) {
      if (t->id != id || t->have) continue;
      t->type = u16(e + 2), t->count = u32(e + 4);
      if ((t->type != 3 && t->type != 4) || !t->count) return ZES_E_TIFF;
      const uint64_t bytes = (uint64_t)t->count * (t->type == 3 ? 2 : 4);
      t->pos = at + 2 + 12ull * i + 8;
      if (bytes > 4) {
        t->pos = u32(e + 8);
        if (t->pos + bytes > c) return ZES_E_TIFF;
      }
      t->have = true;
    }
  }
  // values k0 .. k0 + n - 1 of a tag that is there (inline ones out of the entries, the others by one fetch)
  bool lost = false;
  auto values = [&](const Tag& t, uint64_t k0, uint64_t n, std::vector<uint64_t>& v) {
    const uint32_t size = t.type == 3 ? 2 : 4;
    const bool inl = (uint64_t)t.count * size <= 4;
    const uint8_t* p = inl ? ents + (t.pos - (at + 2)) + k0 * size : fetch(t.pos + k0 * size, n * size);
    if (!p) {
      lost = true;
      return;
    }
    v.resize(n);
    for (uint64_t k = 0; k < n; k++) v[k] = size == 2 ? u16(p + 2 * k) : u32(p + 4 * k);
  };
  auto first = [&](const Tag& t, uint64_t absent) -> uint64_t {
    if (!t.have) return absent;
    std::vector<uint64_t> v;
    values(t, 0, 1, v);
    return lost ? 0 : v[0];
  };
  // geometry
  if (!t_w.have || !t_h.have) return ZES_E_TIFF;
  const uint64_t W = first(t_w, 0), H = first(t_h, 0);
  if (lost) return *frc;
  if (!W || !H) return ZES_E_TIFF;
  const bool strips = t_soff.have || t_slen.have, tiles = t_tw.have || t_tl.have || t_toff.have || t_tlen.have;
  if (strips == tiles) return ZES_E_TIFF;
  if (strips ? !(t_soff.have && t_slen.have) : !(t_tw.have && t_tl.have && t_toff.have && t_tlen.have)) return ZES_E_TIFF;
  uint64_t sw, sh;
  if (tiles) {
    sw = first(t_tw, 0), sh = first(t_tl, 0);
    if (lost) return *frc;
    if (!sw || !sh || sw % 16 || sh % 16) return ZES_E_TIFF;
  } else {
    sw = W, sh = first(t_rps, H);
    if (lost) return *frc;
    if (!sh) return ZES_E_TIFF;
    sh = std::min(sh, H);
  }
  const uint64_t across = tiff_ceil(W, sw), down = tiff_ceil(H, sh), nseg = across * down;
  const Tag &t_off = tiles ? t_toff : t_soff, &t_len = tiles ? t_tlen : t_slen;
  if (t_off.count != nseg || t_len.count != nseg) return ZES_E_TIFF;
  values(t_off, 0, nseg, x.off);
  if (!lost) values(t_len, 0, nseg, x.len);
  if (lost) return *frc;
  for (uint64_t k = 0; k < nseg; k++)
    if (x.off[k] + x.len[k] > c) return ZES_E_TIFF;
  // defaults and kinds
  const uint64_t spp = first(t_spp, 1), comp = first(t_comp, 1), pred = first(t_pred, 1), planar = first(t_planar, 1), fill = first(t_fill, 1);
  const uint64_t fmt = first(t_fmt, 1), photo = first(t_photo, 0), extra = first(t_extra, 0);
  if (lost) return *frc;
  if (!spp || (t_bits.have ? t_bits.count : 1u) != spp) return ZES_E_TIFF;
  std::vector<uint64_t> bits(1, 1);
  if (t_bits.have) values(t_bits, 0, spp, bits);
  if (lost) return *frc;
  for (uint64_t b : bits)
    if (b != bits[0]) return ZES_E_UNSUPPORTED;
  if (bits[0] != 8 && bits[0] != 16 && bits[0] != 32) return ZES_E_UNSUPPORTED;
  if (spp > 4) return ZES_E_UNSUPPORTED;
  if (planar != 1 && spp > 1) return ZES_E_UNSUPPORTED;
  if (fill != 1) return ZES_E_UNSUPPORTED;
  if (comp != 1 && comp != 8 && comp != 32946) return ZES_E_UNSUPPORTED;
  if (pred == 3) return ZES_E_UNSUPPORTED;
  if (pred == 2 && comp == 1) return ZES_E_UNSUPPORTED;
  if (sw * sh > 0xFFFFFFFFull / (spp * (bits[0] / 8))) return ZES_E_UNSUPPORTED;  // (sw, sh < 2^32: the product fits; times the pixel's bytes it might not)
  if (nseg > 0x7fffffffull) return ZES_E_UNSUPPORTED;
  if (pred != 1 && pred != 2) return ZES_E_TIFF;
  zes_tiff_image& m = x.im;
  m.width = (uint32_t)W, m.height = (uint32_t)H, m.seg_w = (uint32_t)sw, m.seg_h = (uint32_t)sh, m.across = (uint32_t)across, m.down = (uint32_t)down;
  m.bits = (uint16_t)bits[0], m.spp = (uint16_t)spp, m.compression = (uint16_t)comp, m.predictor = (uint16_t)pred, m.photometric = (uint16_t)photo;
  m.sample_format = (uint16_t)fmt, m.extra_samples = (uint16_t)extra;
  m.big_endian = be, m.tiled = tiles;
  m.out_size = W * H * spp * (bits[0] / 8);
  return ZES_OK;
}
static_assert(sizeof(zes_tiff_image) == 48 && offsetof(zes_tiff_image, out_size) == 40, "zes_tiff_image is 48 bytes without pad fields");

static int tiff_index_args(const uint8_t* in, uint64_t c, zes_tiff_image* img, const uint64_t* seg_off, const uint64_t* seg_len, uint64_t cap,
                           uint64_t* segments, uint32_t* dirs, uint32_t flags) {
  if (!img || !segments || !dirs || (!in && c) || flags || (cap && (!seg_off || !seg_len))) return ZES_E_ARG;
  memset(img, 0, sizeof *img);
  *segments = 0;
  *dirs = 0;
  return ZES_OK;
}

static int tiff_index_out(int rrc, const TiffIndex& x, zes_tiff_image* img, uint64_t* seg_off, uint64_t* seg_len, uint64_t cap, uint64_t* segments,
                          uint32_t* dirs) {
  *dirs = x.dirs;
  if (rrc) return rrc;
  *img = x.im;
  *segments = x.off.size();
  if (cap < x.off.size()) return ZES_E_NOSPACE;
  memcpy(seg_off, x.off.data(), 8 * x.off.size());
  memcpy(seg_len, x.len.data(), 8 * x.len.size());
  return ZES_OK;
}

int zes_tiff_index(const uint8_t* in, uint64_t c, uint32_t dir, zes_tiff_image* img, uint64_t* seg_off, uint64_t* seg_len, uint64_t cap,
                   uint64_t* segments, uint32_t* dirs, uint32_t flags) {
  if (const int arc = tiff_index_args(in, c, img, seg_off, seg_len, cap, segments, dirs, flags)) return arc;
  TiffIndex x;
  const int frc = ZES_OK;
  const int rrc = tiff_rule(c, dir, [&](uint64_t pos, uint64_t) { return in + pos; }, &frc, x);
  return tiff_index_out(rrc, x, img, seg_off, seg_len, cap, segments, dirs);
}

int zes_tiff_index_dev(const uint8_t* d_in, uint64_t c, uint32_t dir, zes_tiff_image* img, uint64_t* seg_off, uint64_t* seg_len, uint64_t cap,
                       uint64_t* segments, uint32_t* dirs, uint32_t flags) {
  ROUTE_DEV(d_in);
  if (const int arc = tiff_index_args(d_in, c, img, seg_off, seg_len, cap, segments, dirs, flags)) return arc;
  if (c < 8) return ZES_E_TIFF;
  LOCK_READY();
  std::deque<std::vector<uint8_t>> kept;  // (every piece stays until the rule returns)
  int frc = ZES_OK;
  auto fetch = [&](uint64_t pos, uint64_t len) -> const uint8_t* {
    kept.emplace_back(len + 1);
    if (len && (hipMemcpyAsync(kept.back().data(), d_in + pos, len, hipMemcpyDeviceToHost, g.stream) != hipSuccess || hipStreamSynchronize(g.stream) != hipSuccess)) {
      (void)hipGetLastError();
      frc = ZES_E_DEVICE;
      return nullptr;
    }
    return kept.back().data();
  };
  TiffIndex x;
  const int rrc = tiff_rule(c, dir, fetch, &frc, x);
  return tiff_index_out(rrc, x, img, seg_off, seg_len, cap, segments, dirs);
}

// One segment that the rectangle touches: its place in the arrays, where its bytes lie in d_src, its decoded size, its first
// pixel's place in the image and its rows; then its status, and where its decoded bytes lie in k_tiff_place's source
struct TiffSeg {
  uint32_t idx;
  uint64_t at, len, E;
  uint32_t x0, y0, rows;
  int32_t status = ZES_OK;
  uint64_t src_off = 0;
};

// A record the rule could have produced (step 1 of include/zes.h): ZES_OK, or what is wrong with it - ZES_E_ARG for values no
// file gives the record, then ZES_E_UNSUPPORTED for the kinds the rule refuses.  The reader turns both down alike
// (tiff_record_ok); the writer answers them as they are.
static int tiff_record_status(const zes_tiff_image& m) {
  if (!m.width || !m.height || !m.seg_w || !m.seg_h || m.big_endian > 1 || m.tiled > 1) return ZES_E_ARG;
  if ((m.bits != 8 && m.bits != 16 && m.bits != 32) || m.spp < 1 || m.spp > 4) return ZES_E_ARG;
  if ((m.compression != 1 && m.compression != 8 && m.compression != 32946) || (m.predictor != 1 && m.predictor != 2)) return ZES_E_ARG;
  if (m.tiled ? (m.seg_w % 16 || m.seg_h % 16) : (m.seg_w != m.width || m.seg_h > m.height)) return ZES_E_ARG;
  if (m.across != tiff_ceil(m.width, m.seg_w) || m.down != tiff_ceil(m.height, m.seg_h)) return ZES_E_ARG;
  if ((unsigned __int128)m.out_size != (unsigned __int128)m.width * m.height * tiff_ps(m)) return ZES_E_ARG;
  if (m.predictor == 2 && m.compression == 1) return ZES_E_UNSUPPORTED;
  if ((uint64_t)m.across * m.down > 0x7fffffffull || (uint64_t)m.seg_w * m.seg_h > 0xFFFFFFFFull / tiff_ps(m)) return ZES_E_UNSUPPORTED;
  return ZES_OK;
}
static bool tiff_record_ok(const zes_tiff_image& m) { return tiff_record_status(m) == ZES_OK; }

// the rectangle of a call (null: the whole image), or false for an empty one or one that leaves the image
static bool tiff_rect_of(const zes_tiff_image& m, const zes_tiff_rect* rect, zes_tiff_rect* r) {
  *r = rect ? *rect : zes_tiff_rect{0, 0, m.width, m.height};
  return r->w && r->h && (uint64_t)r->x + r->w <= m.width && (uint64_t)r->y + r->h <= m.height;
}

// the segments under the rectangle, in segment order; seg(k) = (file position, length) of segment k
static void tiff_touched(const zes_tiff_image& m, const zes_tiff_rect& r, const std::function<std::pair<uint64_t, uint64_t>(uint32_t)>& seg,
                         std::vector<TiffSeg>& ts) {
  const uint32_t sx0 = r.x / m.seg_w, sx1 = (r.x + r.w - 1) / m.seg_w, sy0 = r.y / m.seg_h, sy1 = (r.y + r.h - 1) / m.seg_h;
  for (uint32_t sy = sy0; sy <= sy1; sy++)
    for (uint32_t sx = sx0; sx <= sx1; sx++) {
      TiffSeg t;
      t.idx = sy * m.across + sx;
      const std::pair<uint64_t, uint64_t> ol = seg(t.idx);
      t.at = ol.first, t.len = ol.second;
      t.E = tiff_seg_size(m, sy);
      t.x0 = sx * m.seg_w, t.y0 = sy * m.seg_h, t.rows = tiff_seg_rows(m, sy);
      ts.push_back(t);
    }
}

// Steps 3 to 5 of include/zes.h for the touched segments ts, whose bytes lie at d_src + at: the rectangle r of image m to dst.
// Every segment's status is left in ts; the return value is the call's own (a device error, scratch that could not grow).
static int tiff_read_core(const uint8_t* d_src, const zes_tiff_image& m, std::vector<TiffSeg>& ts, const zes_tiff_rect& r, uint8_t* dst, uint32_t flags) {
  int rc;
  g.last_tier = 0;
  // what copies queued on the stream read (the gather's segments, the kernel's jobs), and the guard behind them
  std::vector<ZesGzSeg> segs;
  std::vector<ZesTiffJob> tj;
  Drain drain;
  const uint8_t* src = d_src;
  if (m.compression != 1) {  // 4. the zlib streams: gathered, decoded, their lengths and trailers checked
    std::vector<InfJob> jobs;
    uint64_t ipos = 0, opos = 0;
    for (const TiffSeg& t : ts) {
      if (t.len) segs.push_back(ZesGzSeg{t.at, ipos, t.len, 0u, 0u});
      InfJob j{ipos, t.len, opos, gz_slot_cap(t.E), 0, ZES_OK, 0};
      j.want_end = true;
      jobs.push_back(j);
      ipos += gz_slot_in(t.len);
      opos += gz_slot_out(t.E);
    }
    if ((rc = ensure(g.gz_bodies, ipos + 64)) || (rc = ensure(g.gz_outs, opos + 64))) return rc;
    if ((rc = gz_gather(d_src, (uint8_t*)g.gz_bodies.p, segs))) return rc;
    // the same kernels for four segments as for many: a single stream's block chain is followed on the device too
    g.device_chain = true;
    rc = inflate_jobs((const uint8_t*)g.gz_bodies.p, (uint8_t*)g.gz_outs.p, jobs, nullptr, flags & ZES_F_PIECES);
    g.device_chain = false;
    if (rc) return rc;
    for (size_t q = 0; q < jobs.size(); q++)
      if (jobs[q].status == ZES_E_NOSPACE || (jobs[q].status == ZES_OK && jobs[q].out_len != ts[q].E)) jobs[q].status = ZES_E_TIFF;
    if ((rc = check_adler_jobs((const uint8_t*)g.gz_bodies.p, nullptr, (const uint8_t*)g.gz_outs.p, jobs))) return rc;
    keep_times();
    for (size_t q = 0; q < jobs.size(); q++) ts[q].status = jobs[q].status, ts[q].src_off = jobs[q].out_off;
    src = (const uint8_t*)g.gz_outs.p;
  } else {  // 3. read where they lie
    for (TiffSeg& t : ts) t.status = t.len < t.E ? ZES_E_TIFF : ZES_OK, t.src_off = t.at;
  }
  // 5. the pixels
  const uint32_t ps = (uint32_t)tiff_ps(m), run = ps % 3 ? 16u : 48u;
  ZesTiffCall call;
  memset(&call, 0, sizeof call);
  call.pitch = (uint64_t)r.w * ps;
  call.rx = r.x, call.ry = r.y;
  call.seg_rowbytes = m.seg_w * ps;  // (at most a segment's decoded size: 32 bits)
  while (call.lanes_log2 < 6 && ((uint64_t)run << call.lanes_log2) < call.seg_rowbytes) call.lanes_log2++;
  const uint32_t side = 64u >> call.lanes_log2;
  call.unit_rows = side * (uint32_t)std::min<uint64_t>(4, std::max<uint64_t>(1, 4096 / ((uint64_t)call.seg_rowbytes * side)));
  call.bps = m.bits / 8u, call.spp = m.spp, call.predictor = m.predictor, call.big_endian = m.big_endian;
  uint64_t units = 0;
  for (const TiffSeg& t : ts) {
    if (t.status != ZES_OK) continue;
    ZesTiffJob j;
    memset(&j, 0, sizeof j);
    j.src_off = t.src_off, j.x0 = t.x0, j.y0 = t.y0;
    j.row_lo = std::max(r.y, t.y0) - t.y0, j.row_hi = (uint32_t)std::min<uint64_t>((uint64_t)r.y + r.h, (uint64_t)t.y0 + t.rows) - t.y0;
    j.col_lo = std::max(r.x, t.x0) - t.x0, j.col_hi = (uint32_t)std::min<uint64_t>((uint64_t)r.x + r.w, (uint64_t)t.x0 + m.seg_w) - t.x0;
    j.first_unit = (uint32_t)units;
    units += tiff_ceil(j.row_hi - j.row_lo, call.unit_rows);
    if (units > 0x7fffffffull) return ZES_E_ARG;
    tj.push_back(j);
  }
  if (tj.empty()) {
    drain.done();  // (inflate_jobs and check_adler_jobs have brought their results down: the stream is past segs)
    return ZES_OK;
  }
  call.njobs = (uint32_t)tj.size();
  ZesTiffJob closing;
  memset(&closing, 0, sizeof closing);
  closing.first_unit = (uint32_t)units;
  tj.push_back(closing);
  if ((rc = ensure(g.gz_tab, sizeof(ZesTiffJob) * tj.size()))) return rc;
  HIPCHK(hipMemcpyAsync(g.gz_tab.p, tj.data(), sizeof(ZesTiffJob) * tj.size(), hipMemcpyHostToDevice, g.stream));
  {
    Timed t("k_tiff_place");
    constexpr uint32_t per = ZES_TIFF_THREADS / 64u;
    hipLaunchKernelGGL(k_tiff_place, dim3((uint32_t)((units + per - 1) / per)), dim3(ZES_TIFF_THREADS), 0, g.stream, src, dst, (const ZesTiffJob*)g.gz_tab.p, call);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  return ZES_OK;
}
static_assert(sizeof(ZesTiffJob) == 40, "ZesTiffJob: 8-byte aligned records back to back");

// the call's status from its segments', and the caller's seg_status filled
static int tiff_verdict(const zes_tiff_image& m, const std::vector<TiffSeg>& ts, int32_t* seg_status) {
  int worst = ZES_OK;
  if (seg_status)
    for (uint64_t k = 0; k < (uint64_t)m.across * m.down; k++) seg_status[k] = ZES_OK;
  for (const TiffSeg& t : ts) {
    if (seg_status) seg_status[t.idx] = t.status;
    if (!worst) worst = t.status;
  }
  return worst;
}

int zes_tiff_read_dev(const uint8_t* d_in, uint64_t c, const zes_tiff_image* img, const uint64_t* seg_off, const uint64_t* seg_len,
                      const zes_tiff_rect* rect, uint8_t* d_out, uint64_t cap, uint64_t* out_len, int32_t* seg_status, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (!out_len) return ZES_E_ARG;
  *out_len = 0;
  zes_tiff_rect r;
  if (!img || !seg_off || !seg_len || (!d_in && c) || (flags & ~ZES_F_PIECES) || !tiff_record_ok(*img) || !tiff_rect_of(*img, rect, &r)) return ZES_E_ARG;
  std::vector<TiffSeg> ts;
  tiff_touched(*img, r, [&](uint32_t k) { return std::make_pair(seg_off[k], seg_len[k]); }, ts);
  for (const TiffSeg& t : ts)
    if (t.at > c || t.len > c - t.at) return ZES_E_ARG;
  *out_len = (uint64_t)r.w * r.h * tiff_ps(*img);
  if (cap < *out_len) return ZES_E_NOSPACE;
  if (!d_out) {
    *out_len = 0;
    return ZES_E_ARG;
  }
  LOCK_READY();
  g.last_tiff_segs = (uint32_t)ts.size(), g.last_tiff_up = 0;
  if ((rc = call_done(tiff_read_core(d_in, *img, ts, r, d_out, flags), true))) return rc;
  return tiff_verdict(*img, ts, seg_status);
}

int zes_tiff_read_alloc(const uint8_t* in, uint64_t c, uint32_t dir, const zes_tiff_rect* rect, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                        zes_tiff_image* img, uint32_t flags) {
  UseDev ud(route_host());
  if (!out_len || !alloc || (!in && c) || (flags & ~ZES_F_PIECES)) return ZES_E_ARG;
  *out_len = 0;
  if (img) memset(img, 0, sizeof *img);
  TiffIndex x;
  const int frc = ZES_OK;
  if (const int rrc = tiff_rule(c, dir, [&](uint64_t pos, uint64_t) { return in + pos; }, &frc, x)) return rrc;
  if (img) *img = x.im;
  zes_tiff_rect r;
  if (!tiff_rect_of(x.im, rect, &r)) return ZES_E_ARG;
  std::vector<TiffSeg> ts;
  tiff_touched(x.im, r, [&](uint32_t k) { return std::make_pair(x.off[k], x.len[k]); }, ts);
  const uint64_t size = (uint64_t)r.w * r.h * tiff_ps(x.im);
  LOCK_READY();
  HostBatch hb(g.gz_in, g.gz_acc);
  uint64_t up = 0;
  for (TiffSeg& t : ts) {
    up += t.len;
    t.at = hb.place(in + t.at, t.len);
  }
  const uint64_t place = hb.room(size);
  g.last_tiff_segs = (uint32_t)ts.size(), g.last_tiff_up = up;
  if ((rc = hb.up())) return rc;
  if ((rc = call_done(tiff_read_core(hb.d_in(), x.im, ts, r, hb.d_out() + place, flags), true))) return rc;
  if ((rc = tiff_verdict(x.im, ts, nullptr))) return rc;
  uint8_t* to = alloc(user, 0, size);
  if (!to) return ZES_E_ARG;
  if ((rc = download(to, hb.d_out() + place, size))) return rc;
  *out_len = size;
  return ZES_OK;
}

int zes_last_tiff_read(uint32_t* segments, uint64_t* bytes_up) {
  UseDev ud(t_last);
  std::lock_guard<std::mutex> lk(g_mu);
  if (segments) *segments = g.last_tiff_segs;
  if (bytes_up) *bytes_up = g.last_tiff_up;
  return ZES_OK;
}

// ---- PNG writer (include/zes.h: "zes_pngwrite*"): filters by k_png_filter, zlib bodies by EncGroup, files by k_png_pack ----
// What the arguments alone say about image i (steps 1 and 2 of include/zes.h), and its sizes
struct PngwPlan {
  int32_t status = ZES_OK;
  uint32_t rowbytes = 0, bpp = 1, mode = 0, aux_off = 0;
  uint64_t F = 0;  // the filtered bytes: height * (1 + rowbytes)
};
static uint64_t pngw_stored_len(uint64_t F) { return 2 + 5 * ((F + ZES_PNGW_BLOCK - 1) / ZES_PNGW_BLOCK) + F + 4; }
// the file around a zlib stream of zlen bytes
static uint64_t pngw_file_len(const zes_pngw_image& m, uint64_t zlen) {
  return 8 + 25 + (m.plte_len ? 12ull + m.plte_len : 0) + (m.trns_len ? 12ull + m.trns_len : 0) + zlen + 12 * ((zlen + ZES_PNGW_IDAT - 1) / ZES_PNGW_IDAT) + 12;
}
static_assert(sizeof(zes_pngw_image) == 16, "zes_pngw_image is 16 bytes");
static PngwPlan pngw_plan(const zes_pngw_image& m, uint64_t in_len) {
  PngwPlan p;
  p.status = ZES_E_ARG;
  const uint32_t dp = m.depth;
  bool ok;
  switch (m.colour) {
    case 0: ok = dp == 1 || dp == 2 || dp == 4 || dp == 8 || dp == 16; break;
    case 3: ok = dp == 1 || dp == 2 || dp == 4 || dp == 8; break;
    case 2: case 4: case 6: ok = dp == 8 || dp == 16; break;
    default: ok = false;
  }
  if (!ok || m.width - 1 > 0x7ffffffeu || m.height - 1 > 0x7ffffffeu || m.filter > 6 || m.pad) return p;
  const uint64_t rowbytes = png_rowbytes(m.width, m.colour, dp);
  if ((unsigned __int128)in_len != (unsigned __int128)m.height * rowbytes) return p;
  switch (m.colour) {
    case 3: ok = m.plte_len % 3 == 0 && m.plte_len >= 3 && m.plte_len <= (3u << dp) && m.trns_len <= m.plte_len / 3; break;
    case 0: ok = m.plte_len == 0 && (m.trns_len == 0 || m.trns_len == 2); break;
    case 2: ok = m.trns_len == 0 || m.trns_len == 6; break;
    case 4: ok = m.plte_len == 0 && m.trns_len == 0; break;
    default: ok = m.trns_len == 0;
  }
  if (!ok || (m.colour != 3 && (m.plte_len % 3 || m.plte_len > 768))) return p;  // (a PLTE the reader's file rule would reject)
  p.status = ZES_E_UNSUPPORTED;
  if (1 + rowbytes > 0xFFFFFFFFull / m.height) return p;
  p.status = ZES_OK;
  p.rowbytes = (uint32_t)rowbytes;
  p.bpp = std::max<uint32_t>(1, png_channels(m.colour) * dp / 8);
  p.F = m.height * (1 + rowbytes);
  p.mode = (m.filter >= 5 && (m.colour == 3 || dp < 8)) ? 0u : m.filter;  // (adaptive: palette and sub-byte images take None)
  return p;
}

// zes_pngwrite*: what both forms check before anything else, and the plans.  ZES_OK with *any == false: nothing to encode
static int pngwrite_args(const std::function<bool(uint32_t)>& data, const uint64_t* in_len, const zes_pngw_image* img, const uint8_t* aux, uint32_t count,
                         uint64_t* out_len, int32_t* status, uint32_t flags, std::vector<PngwPlan>& plan, bool* any) {
  *any = false;
  if (flags & ~ZES_F_PIECES) return ZES_E_ARG;
  if (count && (!in_len || !img || !out_len || !status)) return ZES_E_ARG;
  uint64_t naux = 0;
  for (uint32_t i = 0; i < count; i++) {
    if (in_len[i] && !data(i)) return ZES_E_ARG;
    naux += (uint64_t)img[i].plte_len + img[i].trns_len;
  }
  if ((naux && !aux) || naux > 0xFFFFFFFFull) return ZES_E_ARG;
  plan.resize(count);
  naux = 0;
  for (uint32_t i = 0; i < count; i++) {
    plan[i] = pngw_plan(img[i], in_len[i]);
    plan[i].aux_off = (uint32_t)naux;
    naux += (uint64_t)img[i].plte_len + img[i].trns_len;
    status[i] = plan[i].status;
    out_len[i] = 0;
    *any = *any || plan[i].status == ZES_OK;
  }
  return ZES_OK;
}

// The images whose status[i] is ZES_OK on entry, image i's scanlines at d_in + in_off[i], its file to d_out + out_off[i] when
// it fits out_cap[i] (and d_out is there), else ZES_E_NOSPACE with the size needed.  Group by group as zipwrite_core goes
// (EncGroup::form over the filtered lengths); a group's launches, in order:
//   k_png_filter   once: every row of the group's images into their scratch buffers (g.gz_outs)
//   the encoder    EncGroup without its CRC-32 launch, the scratch buffers as its input: one deflate_batch_core call, whose
//                  read-back is the group's (none when the encoder refuses every length)
//   k_adler_seg    once, and only when the group has lengths that the encoder refuses (F = 1 mod 131072): their Adler-32s
//                  (finished on the host, so this launch has a read-back of its own)
//   k_png_pack     once: everything of the files but the chunk CRCs
//   k_crc32_seg    once: type and data of every chunk as they lie in the output, the words left on the device
//   k_crc32_put    once: the chunk CRCs finished and stored
// The last three only when an image of the group is written.  g.gz_tab holds the filter's records and, behind the read-back,
// aux | pack records | put records.  Every group's records, which asynchronous uploads read, stay until the end of the call;
// they and the encoder's and checksums' tables are declared in front of a Drain.
static int pngwrite_core(const uint8_t* d_in, const uint64_t* in_off, const zes_pngw_image* img, const uint8_t* aux,
                         const std::vector<PngwPlan>& plan, uint32_t count, uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                         uint64_t* out_len, int32_t* status, uint32_t flags) {
  int rc;
  g.carry.clear();
  g.last_tier = 0;
  const uint32_t nlive = (uint32_t)std::count(status, status + count, (int32_t)ZES_OK);
  std::deque<std::vector<uint8_t>> blobs;
  std::deque<std::vector<uint2>> work;
  std::deque<std::vector<ZesCrcSeg>> segs;
  std::vector<ZesCrcSeg> asegs;  // a group's lengths that the encoder refuses
  std::vector<uint64_t> flen;    // the live images' filtered lengths
  EncGroup eg(flags, nlive);
  std::vector<uint64_t> f_off(eg.o_off.size());
  Drain drain;  // (behind everything above: uploads read it)
  auto blob = [&](size_t n) {
    blobs.emplace_back(n);
    return blobs.back().data();
  };
  std::vector<uint32_t> live;
  for (uint32_t i = 0; i < count; i++)
    if (status[i] == ZES_OK) {
      live.push_back(i);
      flen.push_back(plan[i].F);
    }
  CrcSeg ck;
  for (uint32_t e0 = 0; e0 < nlive;) {
    // the group, its scratch buffers and encoder slots, the filter's records
    const uint64_t* f_len = &flen[e0];
    uint64_t slots, fbytes = 0, units = 0;
    const uint32_t cnt = eg.form(f_len, nlive - e0, &slots);
    for (uint32_t k = 0; k < cnt; k++) {
      f_off[k] = fbytes;
      fbytes += gz_up16(f_len[k]) + 16;
    }
    ZesPngwJob* jobs = (ZesPngwJob*)blob(sizeof(ZesPngwJob) * ((size_t)cnt + 1));
    for (uint32_t k = 0; k < cnt; k++) {
      const uint32_t i = live[e0 + k];
      const PngwPlan& p = plan[i];
      jobs[k] = ZesPngwJob{in_off[i], f_off[k], img[i].height, p.rowbytes, p.bpp, p.mode, (uint32_t)units, 0u};
      units += (img[i].height + ZES_PNGW_RUN - 1) / ZES_PNGW_RUN;
    }
    if (units > 0x7fffffffull) return ZES_E_ARG;
    jobs[cnt] = ZesPngwJob{0, 0, 0u, 0u, 0u, 0u, (uint32_t)units, 0u};
    if ((rc = ensure(g.gz_outs, fbytes + 64)) || (rc = ensure(g.gz_tab, sizeof(ZesPngwJob) * ((size_t)cnt + 1)))) return rc;
    uint8_t* filt = (uint8_t*)g.gz_outs.p;
    HIPCHK(hipMemcpyAsync(g.gz_tab.p, jobs, sizeof(ZesPngwJob) * ((size_t)cnt + 1), hipMemcpyHostToDevice, g.stream));
    {
      Timed t("k_png_filter");
      constexpr uint32_t per = ZES_PNGW_THREADS / 64u;
      hipLaunchKernelGGL(k_png_filter, dim3((uint32_t)((units + per - 1) / per)), dim3(ZES_PNGW_THREADS), 0, g.stream, d_in, filt, (const ZesPngwJob*)g.gz_tab.p, cnt);
    }
    HIPCHK(hipGetLastError());
    if ((rc = eg.encode(filt, f_off.data(), f_len, cnt, slots, false))) return rc;
    // the lengths the encoder refuses: their Adler-32s
    asegs.clear();
    for (uint32_t k = 0; k < cnt; k++)
      if (!eg.o_cap[k]) asegs.push_back(ZesCrcSeg{f_off[k], f_len[k]});
    std::vector<uint32_t> adler(asegs.size());
    if (!asegs.empty() && (rc = adler32_batch_locked(filt, asegs.data(), (uint32_t)asegs.size(), adler.data()))) return rc;
    // (the stream has been waited for: the filter's records in g.gz_tab are done with)
    // stream or stored, the files' sizes and places
    uint64_t naux = 0, wgs = 0;
    uint32_t nrec = 0;
    for (uint32_t k = 0; k < cnt; k++) naux += (uint64_t)img[live[e0 + k]].plte_len + img[live[e0 + k]].trns_len;
    const size_t aux_pad = (size_t)gz_up16(naux);
    uint8_t* haux = blob(aux_pad + 16);
    ZesPngwRec* recs = (ZesPngwRec*)blob(sizeof(ZesPngwRec) * ((size_t)cnt + 1));
    segs.emplace_back();
    std::vector<ZesCrcSeg>& csegs = segs.back();
    std::vector<ZesCrcPut> puts;
    uint32_t aux_at = 0, refused = 0;
    for (uint32_t k = 0; k < cnt; k++) {
      const uint32_t i = live[e0 + k];
      const PngwPlan& p = plan[i];
      const zes_pngw_image& m = img[i];
      const uint64_t stored_len = pngw_stored_len(p.F);
      const bool stream = eg.o_cap[k] && eg.raw[k] + 6 < stored_len;
      const uint64_t zlen = stream ? eg.raw[k] + 6 : stored_len;
      const uint32_t my_adler = eg.o_cap[k] ? 0u : adler[refused++];
      out_len[i] = pngw_file_len(m, zlen);
      if (!d_out || out_len[i] > out_cap[i]) {
        status[i] = ZES_E_NOSPACE;
        continue;
      }
      ZesPngwRec& r = recs[nrec++];
      memset(&r, 0, sizeof r);
      r.src_off = stream ? eg.o_off[k] : f_off[k];
      r.dst_off = out_off[i];
      r.zlen = zlen;
      r.adler_off = eg.o_cap[k] ? eg.o_off[k] + eg.raw[k] + 2 : ZES_PNGW_NO_SLOT;
      r.flen = (uint32_t)p.F;
      r.width = m.width, r.height = m.height;
      r.aux_off = aux_at;
      r.first_wg = (uint32_t)wgs;
      r.adler = my_adler;
      r.plte_len = m.plte_len, r.trns_len = m.trns_len;
      r.depth = m.depth, r.colour = m.colour, r.stored = stream ? 0 : 1;
      if (m.plte_len + m.trns_len) memcpy(haux + aux_at, aux + p.aux_off, (size_t)m.plte_len + m.trns_len);
      aux_at += (uint32_t)m.plte_len + m.trns_len;
      // the chunks as they will lie in the output: type and data of each, and the CRC field behind them
      const uint64_t nidat = (zlen + ZES_PNGW_IDAT - 1) / ZES_PNGW_IDAT;
      uint64_t at = out_off[i] + 8;
      auto chunk = [&](uint64_t dlen) {
        csegs.push_back(ZesCrcSeg{at + 4, 4 + dlen});
        const uint64_t a = (uint64_t)(uintptr_t)d_out + at + 4;
        puts.push_back(ck.put(a, a + 4 + dlen, at + 8 + dlen));
        at += 12 + dlen;
      };
      chunk(13);
      if (m.plte_len) chunk(m.plte_len);
      if (m.trns_len) chunk(m.trns_len);
      for (uint64_t c = 0; c < nidat; c++) chunk(std::min<uint64_t>(ZES_PNGW_IDAT, zlen - c * ZES_PNGW_IDAT));
      chunk(0);
      wgs += nidat;
    }
    if (!nrec) {
      e0 += cnt;
      continue;
    }
    if (wgs > 0x7fffffffull || csegs.size() > 0x7fffffffull) return ZES_E_ARG;
    memset(&recs[nrec], 0, sizeof(ZesPngwRec));
    recs[nrec].first_wg = (uint32_t)wgs;
    const size_t o_recs = aux_pad, o_puts = o_recs + sizeof(ZesPngwRec) * ((size_t)nrec + 1), n_puts = sizeof(ZesCrcPut) * puts.size();
    ZesCrcPut* hputs = (ZesCrcPut*)blob(n_puts);
    memcpy(hputs, puts.data(), n_puts);
    if ((rc = ensure(g.gz_tab, o_puts + n_puts))) return rc;
    uint8_t* tab = (uint8_t*)g.gz_tab.p;
    if (aux_pad) HIPCHK(hipMemcpyAsync(tab, haux, aux_pad, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(tab + o_recs, recs, sizeof(ZesPngwRec) * ((size_t)nrec + 1), hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(tab + o_puts, hputs, n_puts, hipMemcpyHostToDevice, g.stream));
    {
      Timed t("k_png_pack");
      hipLaunchKernelGGL(k_png_pack, dim3((uint32_t)wgs), dim3(GZ_GATHER_THREADS), 0, g.stream, (const uint8_t*)filt, (const uint8_t*)g.gz_bodies.p, (const uint8_t*)tab,
                         d_out, (const ZesPngwRec*)(tab + o_recs), nrec);
    }
    HIPCHK(hipGetLastError());
    work.emplace_back();
    unsigned int* d_acc = nullptr;
    rc = seg_checksum_enqueue(ck, d_out, csegs.data(), (uint32_t)csegs.size(), work.back(), &d_acc);
    if (rc || !d_acc) return rc ? rc : ZES_E_DEVICE;
    {
      Timed t("k_crc32_put");
      hipLaunchKernelGGL(k_crc32_put, dim3((uint32_t)((puts.size() + 255) / 256)), dim3(256), 0, g.stream, (const unsigned int*)d_acc, (const ZesCrcPut*)(tab + o_puts),
                         (uint32_t)puts.size(), d_out);
    }
    HIPCHK(hipGetLastError());
    e0 += cnt;
  }
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  return ZES_OK;
}

int zes_pngwrite_bound(const zes_pngw_image* img, uint32_t count, uint64_t* cap) {
  if (count && (!img || !cap)) return ZES_E_ARG;
  for (uint32_t i = 0; i < count; i++) {
    const zes_pngw_image& m = img[i];
    // (the scanlines' size is not an argument here: the one that fits the header)
    const unsigned __int128 n = (unsigned __int128)m.height * png_rowbytes(m.width, m.colour, m.depth);
    const PngwPlan p = n > 0xFFFFFFFFFFFFFFFFull ? PngwPlan{ZES_E_UNSUPPORTED} : pngw_plan(m, (uint64_t)n);
    cap[i] = p.status == ZES_OK ? pngw_file_len(m, pngw_stored_len(p.F)) : 0;
  }
  return ZES_OK;
}

int zes_pngwrite_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, const zes_pngw_image* img, const uint8_t* aux, uint32_t count,
                     uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (count && (!in_off || !out_off || !out_cap)) return ZES_E_ARG;
  std::vector<PngwPlan> plan;
  bool any = false;
  if (const int arc = pngwrite_args([&](uint32_t) { return d_in != nullptr; }, in_len, img, aux, count, out_len, status, flags, plan, &any)) return arc;
  if (!any) {
    call_none();
    return ZES_OK;
  }
  LOCK_READY();
  return call_done(pngwrite_core(d_in, in_off, img, aux, plan, count, d_out, out_off, out_cap, out_len, status, flags), true);
}

int zes_pngwrite(const uint8_t* const* in, const uint64_t* in_len, const zes_pngw_image* img, const uint8_t* aux, uint32_t count, zes_alloc_fn alloc,
                 void* user, uint64_t* out_len, int32_t* status, uint32_t flags) {
  UseDev ud(route_host());
  if (count && (!in || !alloc)) return ZES_E_ARG;
  std::vector<PngwPlan> plan;
  bool any = false;
  if (const int arc = pngwrite_args([&](uint32_t i) { return in[i] != nullptr; }, in_len, img, aux, count, out_len, status, flags, plan, &any)) return arc;
  if (!any) {
    call_none();
    return ZES_OK;
  }
  LOCK_READY();
  // every file gets the bound's room
  HostBatch hb(g.gz_in, g.gz_acc);
  std::vector<uint64_t> in_off(count, 0), out_off(count, 0), out_cap(count, 0);
  for (uint32_t i = 0; i < count; i++) {
    if (status[i] != ZES_OK) continue;
    in_off[i] = hb.place(in[i], in_len[i]);
    out_cap[i] = pngw_file_len(img[i], pngw_stored_len(plan[i].F));
    out_off[i] = hb.room(out_cap[i]);
  }
  if ((rc = hb.up())) return rc;
  rc = pngwrite_core(hb.d_in(), in_off.data(), img, aux, plan, count, hb.d_out(), out_off.data(), out_cap.data(), out_len, status, flags);
  if ((rc = call_done(rc, true))) return rc;
  return hb.hand_out(count, alloc, user, status, out_len, [&](uint32_t i) { return out_len[i]; }, [&](uint32_t i) { return out_off[i]; });
}

// zes_pngpix_expand_dev: k_png_expand alone, over scanlines in device memory that the writer's records describe.  The checks
// are the writer's (pngwrite_args, with the filter field, which says nothing here, taken as 0); the job table and the aux
// bytes go up in one copy and nothing comes back: every status is the host's.
int zes_pngpix_expand_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, const zes_pngw_image* img, const uint8_t* aux, uint32_t count,
                          uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (count && (!in_off || !out_off || !out_cap || !img)) return ZES_E_ARG;
  std::vector<zes_pngw_image> plain(img, img + count);
  for (zes_pngw_image& m : plain) m.filter = 0;
  std::vector<PngwPlan> plan;
  bool any = false;
  if (const int arc = pngwrite_args([&](uint32_t) { return d_in != nullptr; }, in_len, plain.data(), aux, count, out_len, status, flags, plan, &any)) return arc;
  std::vector<uint8_t> table, bytes;
  uint64_t tiles = 0;
  uint32_t njobs = 0;
  for (uint32_t i = 0; i < count; i++) {
    if (status[i] != ZES_OK) continue;
    const zes_pngw_image& m = plain[i];
    out_len[i] = png_pix_size(m.width, m.height);
    if (!d_out || out_cap[i] < out_len[i]) {
      status[i] = ZES_E_NOSPACE;
      continue;
    }
    ZesPngxJob j = pngx_job(m.width, m.height, m.colour, m.depth, m.plte_len, m.trns_len, &tiles);
    j.src_off = in_off[i], j.dst_off = out_off[i];
    j.plte_off = bytes.size(), j.trns_off = bytes.size() + m.plte_len;
    bytes.insert(bytes.end(), aux + plan[i].aux_off, aux + plan[i].aux_off + m.plte_len + m.trns_len);
    table.insert(table.end(), (const uint8_t*)&j, (const uint8_t*)&j + sizeof j);
    njobs++;
  }
  if (!njobs) {
    call_none();
    return ZES_OK;
  }
  table.insert(table.end(), bytes.begin(), bytes.end());
  LOCK_READY();
  g.carry.clear();
  g.last_tier = 0;
  return call_done(pngx_run(d_in, nullptr, d_out, table, njobs, tiles), true);
}

// ---- TIFF writer (include/zes.h: "zes_tiffwrite*"): segments by k_tiff_cut, zlib streams by EncGroup, the file by k_tiff_pack ----
// What the record alone says (statuses 1 and 2 of include/zes.h), and the sizes that follow from it
struct TiffwPlan {
  uint32_t base = 1;      // the photometric's samples: what spp exceeds are extra samples
  uint32_t entries = 0;   // of the directory
  uint64_t nseg = 0;
  uint64_t tail = 0;      // bytes of the out-of-line arrays and the directory
  uint64_t bound = 0;     // the file with every segment in the stored form
};
static uint64_t tiffw_stored_len(const zes_tiff_image& m, uint64_t E) { return m.compression == 1 ? E : pngw_stored_len(E); }
static uint64_t tiffw_even(uint64_t v) { return v + (v & 1); }
static int tiffw_plan(const zes_tiff_image& m, uint64_t n, TiffwPlan* p) {
  const int st = tiff_record_status(m);
  if (st == ZES_E_ARG || n != m.out_size) return ZES_E_ARG;
  if (m.photometric > 2) return ZES_E_ARG;
  p->base = m.photometric == 2 ? 3u : 1u;
  if (m.spp < p->base || m.extra_samples > 2 || (m.spp == p->base && m.extra_samples)) return ZES_E_ARG;
  if (m.sample_format < 1 || m.sample_format > 3 || (m.sample_format == 3 && m.bits != 32)) return ZES_E_ARG;
  if (st) return st;
  p->nseg = (uint64_t)m.across * m.down;
  const bool fmt = m.sample_format != 1;
  p->entries = (m.tiled ? 11u : 10u) + (m.predictor == 2 ? 1u : 0u) + (m.spp > p->base ? 1u : 0u) + (fmt ? 1u : 0u);
  // (every array has an even size: none needs a pad byte in front of the next)
  p->tail = (m.spp >= 3 ? 2ull * m.spp : 0) + (m.spp - p->base == 3 ? 6ull : 0) + (fmt && m.spp >= 3 ? 2ull * m.spp : 0) + (p->nseg >= 2 ? 8 * p->nseg : 0) + 2 +
            12ull * p->entries + 4;
  // the segments: every row of them alike but the last row of strips
  const unsigned __int128 full = (unsigned __int128)(p->nseg - m.across) * tiffw_even(tiffw_stored_len(m, tiff_seg_size(m, 0)));
  const unsigned __int128 bound = 8 + full + (unsigned __int128)m.across * tiffw_even(tiffw_stored_len(m, tiff_seg_size(m, m.down - 1))) + p->tail;
  if (bound > 0xFFFFFFFFull) return ZES_E_UNSUPPORTED;
  p->bound = (uint64_t)bound;
  return ZES_OK;
}

// The out-of-line arrays and the directory as they lie at the even file position `at`, the segments at off[k] with len[k] bytes
static void tiffw_tail(const zes_tiff_image& m, const TiffwPlan& p, const uint64_t* off, const uint64_t* len, uint64_t at, std::vector<uint8_t>& b) {
  const bool be = m.big_endian != 0;
  auto p16 = [&](uint32_t v) {
    b.push_back((uint8_t)(be ? v >> 8 : v));
    b.push_back((uint8_t)(be ? v : v >> 8));
  };
  auto p32 = [&](uint32_t v) {
    for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * (be ? 3 - k : k))));
  };
  struct Ent {
    uint32_t tag, type;  // 3: SHORT, 4: LONG
    std::vector<uint32_t> vals;
    uint32_t pos = 0;    // of values that do not fit the entry
  };
  std::vector<Ent> ents;
  auto add = [&](uint32_t tag, uint32_t type, std::vector<uint32_t> vals) { ents.push_back(Ent{tag, type, std::move(vals), 0u}); };
  std::vector<uint32_t> voff((size_t)p.nseg), vlen((size_t)p.nseg);
  for (uint64_t k = 0; k < p.nseg; k++) voff[(size_t)k] = (uint32_t)off[k], vlen[(size_t)k] = (uint32_t)len[k];
  add(256, 4, {m.width});
  add(257, 4, {m.height});
  add(258, 3, std::vector<uint32_t>(m.spp, m.bits));
  add(259, 3, {m.compression});
  add(262, 3, {m.photometric});
  if (!m.tiled) add(273, 4, voff);
  add(277, 3, {m.spp});
  if (!m.tiled) add(278, 4, {m.seg_h}), add(279, 4, vlen);
  add(284, 3, {1u});
  if (m.predictor == 2) add(317, 3, {2u});
  if (m.tiled) add(322, 4, {m.seg_w}), add(323, 4, {m.seg_h}), add(324, 4, voff), add(325, 4, vlen);
  if (m.spp > p.base) add(338, 3, std::vector<uint32_t>(m.spp - p.base, m.extra_samples));
  if (m.sample_format != 1) add(339, 3, std::vector<uint32_t>(m.spp, m.sample_format));
  auto put = [&](const Ent& e) {
    for (uint32_t v : e.vals) e.type == 3 ? p16(v) : p32(v);
  };
  auto size_of = [](const Ent& e) { return (uint64_t)e.vals.size() * (e.type == 3 ? 2u : 4u); };
  const uint32_t order[5] = {258u, 338u, 339u, m.tiled ? 324u : 273u, m.tiled ? 325u : 279u};
  for (uint32_t tag : order)
    for (Ent& e : ents)
      if (e.tag == tag && size_of(e) > 4) {
        e.pos = (uint32_t)(at + b.size());
        put(e);
      }
  p16((uint32_t)ents.size());
  for (const Ent& e : ents) {
    p16(e.tag), p16(e.type), p32((uint32_t)e.vals.size());
    if (size_of(e) > 4) {
      p32(e.pos);
    } else {
      const size_t before = b.size();
      put(e);
      b.resize(before + 4, 0);
    }
  }
  p32(0);  // no next directory
}

// The image at d_in (m.out_size bytes, any alignment) written as the file of include/zes.h to d_out[0, cap).  Group by group as
// pngwrite_core goes (EncGroup::form over the segments' decoded lengths); a group's launches, in order:
//   k_tiff_cut     once: every segment of the group into its scratch slot (g.gz_outs)
//   the encoder    EncGroup without its CRC-32 launch, the slots as its input: one deflate_batch_core call, whose read-back is the
//                  group's (none for Compression 1, and none when the encoder refuses every length)
//   k_adler_seg    once, and only when the group has lengths that the encoder refuses (1, or 1 mod 131072): their Adler-32s
//   k_tiff_pack    once: the segments at their file positions; in the last group also the tail and the header, a host-built blob
// g.gz_tab holds the cut's records, the pack's records and the blob side by side.  Every group's tables, which asynchronous
// uploads read, stay until the end of the call, in front of a Drain.  A result beyond cap: EncGroup::room's rule.
static int tiffwrite_core(const uint8_t* d_in, const zes_tiff_image& m, const TiffwPlan& p, uint8_t* d_out, uint64_t cap, uint64_t* out_len,
                          uint64_t* seg_off, uint64_t* seg_len, uint32_t flags) {
  int rc;
  g.carry.clear();
  g.last_tier = 0;
  const bool zl = m.compression != 1;
  const uint32_t ps = (uint32_t)tiff_ps(m), run = ps % 3 ? 16u : 48u;
  std::deque<std::vector<uint8_t>> blobs;
  std::vector<ZesCrcSeg> asegs;                                   // a group's lengths that the encoder refuses
  std::vector<uint64_t> off((size_t)p.nseg), len((size_t)p.nseg);  // the segments as written
  EncGroup eg(flags, p.nseg);
  std::vector<uint64_t> c_off(eg.o_off.size()), c_len(eg.o_off.size());
  Drain drain;  // (behind everything above: uploads read it)
  auto blob = [&](size_t n) {
    blobs.emplace_back(n);
    return blobs.back().data();
  };
  ZesTiffCall call;
  memset(&call, 0, sizeof call);
  call.pitch = (uint64_t)m.width * ps;
  call.seg_rowbytes = m.seg_w * ps;
  while (call.lanes_log2 < 6 && ((uint64_t)run << call.lanes_log2) < call.seg_rowbytes) call.lanes_log2++;
  const uint32_t side = 64u >> call.lanes_log2;
  call.unit_rows = side * (uint32_t)std::min<uint64_t>(4, std::max<uint64_t>(1, 4096 / ((uint64_t)call.seg_rowbytes * side)));
  call.bps = m.bits / 8u, call.spp = m.spp, call.predictor = m.predictor, call.big_endian = m.big_endian;
  uint64_t total = 8;
  for (uint64_t e0 = 0; e0 < p.nseg;) {
    // the group, its scratch slots and encoder slots, the cut's records
    const uint64_t win = std::min<uint64_t>(eg.group, p.nseg - e0);
    for (uint64_t k = 0; k < win; k++) c_len[(size_t)k] = tiff_seg_size(m, (uint32_t)((e0 + k) / m.across));
    uint64_t slots, cbytes = 0, units = 0;
    const uint32_t cnt = eg.form(c_len.data(), win, &slots);
    const bool last = e0 + cnt == p.nseg;
    ZesTiffCutJob* jobs = (ZesTiffCutJob*)blob(sizeof(ZesTiffCutJob) * ((size_t)cnt + 1));
    for (uint32_t k = 0; k < cnt; k++) {
      const uint32_t sy = (uint32_t)((e0 + k) / m.across), sx = (uint32_t)((e0 + k) % m.across);
      c_off[k] = cbytes;
      cbytes += gz_up16(c_len[k]) + 16;
      ZesTiffCutJob& j = jobs[k];
      j.dst_off = c_off[k];
      j.x0 = sx * m.seg_w, j.y0 = sy * m.seg_h;
      j.live_rows = tiff_seg_rows(m, sy);
      j.rows = m.tiled ? m.seg_h : j.live_rows;
      j.live_rows = std::min(j.live_rows, m.height - j.y0);
      j.cols = std::min(m.seg_w, m.width - j.x0);
      j.first_unit = (uint32_t)units;
      units += tiff_ceil(j.rows, call.unit_rows);
    }
    if (units > 0x7fffffffull) return ZES_E_ARG;
    memset(&jobs[cnt], 0, sizeof(ZesTiffCutJob));
    jobs[cnt].first_unit = (uint32_t)units;
    const size_t n_jobs = sizeof(ZesTiffCutJob) * ((size_t)cnt + 1), o_recs = (size_t)gz_up16(n_jobs);
    const size_t o_blob = o_recs + (size_t)gz_up16(sizeof(ZesTiffPackRec) * ((size_t)cnt + 3)), o_head = (size_t)gz_up16(p.tail);
    if ((rc = ensure(g.gz_outs, cbytes + 64)) || (rc = ensure(g.gz_tab, o_blob + o_head + 16 + 64))) return rc;
    uint8_t* cut = (uint8_t*)g.gz_outs.p;
    uint8_t* tab = (uint8_t*)g.gz_tab.p;
    HIPCHK(hipMemcpyAsync(tab, jobs, n_jobs, hipMemcpyHostToDevice, g.stream));
    call.njobs = cnt;
    {
      Timed t("k_tiff_cut");
      constexpr uint32_t per = ZES_TIFF_THREADS / 64u;
      hipLaunchKernelGGL(k_tiff_cut, dim3((uint32_t)((units + per - 1) / per)), dim3(ZES_TIFF_THREADS), 0, g.stream, d_in, cut, (const ZesTiffCutJob*)tab, call);
    }
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> adler;
    if (zl) {
      if ((rc = eg.encode(cut, c_off.data(), c_len.data(), cnt, slots, false))) return rc;
      // the lengths the encoder refuses: their Adler-32s
      asegs.clear();
      for (uint32_t k = 0; k < cnt; k++)
        if (!eg.o_cap[k]) asegs.push_back(ZesCrcSeg{c_off[k], c_len[k]});
      adler.resize(asegs.size());
      if (!asegs.empty() && (rc = adler32_batch_locked(cut, asegs.data(), (uint32_t)asegs.size(), adler.data()))) return rc;
    }
    // stream, stored or as it is; the segments' places
    ZesTiffPackRec* recs = (ZesTiffPackRec*)blob(sizeof(ZesTiffPackRec) * ((size_t)cnt + 3));
    memset(recs, 0, sizeof(ZesTiffPackRec) * ((size_t)cnt + 3));
    uint64_t wgs = 0;
    uint32_t nrec = 0, refused = 0;
    for (uint32_t k = 0; k < cnt; k++) {
      const uint64_t E = c_len[k], stored_len = tiffw_stored_len(m, E);
      const bool stream = zl && eg.o_cap[k] && eg.raw[k] + 6 < stored_len;
      ZesTiffPackRec& r = recs[nrec++];
      r.kind = !zl ? ZES_TIFFW_RAW : stream ? ZES_TIFFW_STREAM : ZES_TIFFW_STORED;
      r.src_off = stream ? eg.o_off[k] : c_off[k];
      r.dst_off = total;
      r.adler_off = ZES_PNGW_NO_SLOT;
      if (zl && !stream) {
        if (eg.o_cap[k]) r.adler_off = eg.o_off[k] + eg.raw[k] + 2;
        else r.adler = adler[refused++];
      }
      r.len = (uint32_t)(stream ? eg.raw[k] + 6 : E);
      r.first_wg = (uint32_t)wgs;
      wgs += r.kind == ZES_TIFFW_STORED ? tiff_ceil(E, ZES_PNGW_BLOCK) : std::max<uint64_t>(1, tiff_ceil(r.len, ZES_TIFFW_PIECE));
      off[(size_t)(e0 + k)] = total;
      len[(size_t)(e0 + k)] = stream ? eg.raw[k] + 6 : stored_len;
      total += tiffw_even(len[(size_t)(e0 + k)]);
    }
    uint8_t* hblob = nullptr;
    if (last) {  // the tail behind the last segment, and the header, which states where the tail's directory lies
      std::vector<uint8_t> tail;
      tiffw_tail(m, p, off.data(), len.data(), total, tail);
      if (tail.size() != p.tail) return ZES_E_DEVICE;  // (the plan's arithmetic and the builder disagree: a bug)
      hblob = blob(o_head + 16);
      memcpy(hblob, tail.data(), tail.size());
      const uint32_t dir = (uint32_t)(total + p.tail - (2 + 12ull * p.entries + 4));
      const uint8_t head[8] = {(uint8_t)(m.big_endian ? 0x4d : 0x49), (uint8_t)(m.big_endian ? 0x4d : 0x49), (uint8_t)(m.big_endian ? 0 : 42),
                               (uint8_t)(m.big_endian ? 42 : 0),      (uint8_t)(dir >> (m.big_endian ? 24 : 0)), (uint8_t)(dir >> (m.big_endian ? 16 : 8)),
                               (uint8_t)(dir >> (m.big_endian ? 8 : 16)), (uint8_t)(dir >> (m.big_endian ? 0 : 24))};
      memcpy(hblob + o_head, head, 8);
      for (int q = 0; q < 2; q++) {
        ZesTiffPackRec& r = recs[nrec++];
        r.kind = ZES_TIFFW_BLOB;
        r.src_off = q ? o_head : 0;
        r.dst_off = q ? 0 : total;
        r.adler_off = ZES_PNGW_NO_SLOT;
        r.len = q ? 8u : (uint32_t)p.tail;
        r.first_wg = (uint32_t)wgs;
        wgs += std::max<uint64_t>(1, tiff_ceil(r.len, ZES_TIFFW_PIECE));
      }
      total += p.tail;
    }
    if (wgs > 0x7fffffffull) return ZES_E_ARG;
    recs[nrec].first_wg = (uint32_t)wgs;
    if (eg.room(total, cap, d_out)) {
      HIPCHK(hipMemcpyAsync(tab + o_recs, recs, sizeof(ZesTiffPackRec) * ((size_t)nrec + 1), hipMemcpyHostToDevice, g.stream));
      if (hblob) HIPCHK(hipMemcpyAsync(tab + o_blob, hblob, o_head + 16, hipMemcpyHostToDevice, g.stream));
      Timed t("k_tiff_pack");
      hipLaunchKernelGGL(k_tiff_pack, dim3((uint32_t)wgs), dim3(GZ_GATHER_THREADS), 0, g.stream, (const uint8_t*)cut, (const uint8_t*)g.gz_bodies.p,
                         (const uint8_t*)(tab + o_blob), d_out, (const ZesTiffPackRec*)(tab + o_recs), nrec);
    }
    HIPCHK(hipGetLastError());
    e0 += cnt;
  }
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  for (uint64_t k = 0; k < p.nseg; k++) {
    if (seg_off) seg_off[k] = off[(size_t)k];
    if (seg_len) seg_len[k] = len[(size_t)k];
  }
  *out_len = total;
  return eg.fits ? ZES_OK : ZES_E_NOSPACE;
}
static_assert(sizeof(ZesTiffCutJob) == 32 && sizeof(ZesTiffPackRec) == 40, "the writer's records: 8-byte aligned, back to back");

int zes_tiffwrite_bound(const zes_tiff_image* img, uint64_t* cap, uint64_t* segments) {
  if (!img || !cap) return ZES_E_ARG;
  *cap = 0;
  if (segments) *segments = 0;
  TiffwPlan p;
  if (const int prc = tiffw_plan(*img, img->out_size, &p)) return prc;
  *cap = p.bound;
  if (segments) *segments = p.nseg;
  return ZES_OK;
}

int zes_tiffwrite_dev(const uint8_t* d_in, uint64_t n, const zes_tiff_image* img, uint8_t* d_out, uint64_t cap, uint64_t* out_len, uint64_t* seg_off,
                      uint64_t* seg_len, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (!img || !out_len || (!d_in && n) || (flags & ~ZES_F_PIECES)) return ZES_E_ARG;
  *out_len = 0;
  TiffwPlan p;
  if (const int prc = tiffw_plan(*img, n, &p)) return prc;
  LOCK_READY();
  return call_done(tiffwrite_core(d_in, *img, p, d_out, cap, out_len, seg_off, seg_len, flags), true);
}

int zes_tiffwrite(const uint8_t* in, uint64_t n, const zes_tiff_image* img, zes_alloc_fn alloc, void* user, uint64_t* out_len, uint32_t flags) {
  UseDev ud(route_host());
  if (!img || !out_len || !alloc || (!in && n) || (flags & ~ZES_F_PIECES)) return ZES_E_ARG;
  *out_len = 0;
  TiffwPlan p;
  if (const int prc = tiffw_plan(*img, n, &p)) return prc;
  LOCK_READY();
  HostBatch hb(g.gz_in, g.gz_acc);
  const uint64_t in_at = hb.place(in, n), out_at = hb.room(p.bound);
  if ((rc = hb.up())) return rc;
  uint64_t total = 0;
  if ((rc = call_done(tiffwrite_core(hb.d_in() + in_at, *img, p, hb.d_out() + out_at, p.bound, &total, nullptr, nullptr, flags), true))) return rc;
  uint8_t* to = alloc(user, 0, total);
  if (!to) return ZES_E_ARG;
  if ((rc = download(to, hb.d_out() + out_at, total))) return rc;
  *out_len = total;
  return ZES_OK;
}

// ---- gzip files as one batch (include/zes.h: "zes_gzip_batch*", "zes_gunzip_batch*") ----
constexpr uint64_t GZB_LEN_MAX = 0xFFFFFFFFull;  // (ISIZE is exact up to here)
static uint64_t gzip_batch_cap(uint64_t n) { return 18 + zes_gz_stored_len(n); }

// What both writer forms decide from the arguments alone (`data(i)`: file i's bytes are there): ZES_E_ARG, then every file's
// status, ZES_E_UNSUPPORTED for a length that ISIZE cannot state.  *any: a file is left to encode
static int gzip_batch_args(const std::function<bool(uint32_t)>& data, const uint64_t* in_len, uint32_t count, uint64_t* out_len, int32_t* status,
                           uint32_t flags, bool* any) {
  *any = false;
  if (flags & ~ZES_F_PIECES) return ZES_E_ARG;
  if (count && (!in_len || !out_len || !status)) return ZES_E_ARG;
  for (uint32_t i = 0; i < count; i++)
    if (in_len[i] && !data(i)) return ZES_E_ARG;
  for (uint32_t i = 0; i < count; i++) {
    status[i] = in_len[i] > GZB_LEN_MAX ? ZES_E_UNSUPPORTED : ZES_OK;
    out_len[i] = 0;
    *any = *any || status[i] == ZES_OK;
  }
  return ZES_OK;
}

// The files whose status[i] is ZES_OK on entry, file i's bytes at d_in + in_off[i], its gzip file to d_out + out_off[i] when it
// fits out_cap[i] (and d_out is there), else ZES_E_NOSPACE with the size needed.  Group by group as zipwrite_core goes
// (EncGroup::form over the lengths): EncGroup::encode with its one CRC-32 launch, whose read-back is the group's, the host
// chooses stream or stored form per file, and one k_gz_pack launch writes the group's files.  g.gz_tab holds the group's
// records; every group's records, which asynchronous uploads read, stay until the end of the call, in front of a Drain.
static int gzip_batch_core(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out, const uint64_t* out_off,
                           const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t flags) {
  int rc;
  g.carry.clear();
  g.last_tier = 0;
  std::vector<uint32_t> live;
  std::vector<uint64_t> l_off, l_len;
  for (uint32_t i = 0; i < count; i++)
    if (status[i] == ZES_OK) {
      live.push_back(i);
      l_off.push_back(in_off[i]);
      l_len.push_back(in_len[i]);
    }
  const uint32_t nlive = (uint32_t)live.size();
  std::deque<std::vector<ZesGzPackRec>> tables;
  EncGroup eg(flags, nlive);
  Drain drain;  // (behind the tables and eg)
  for (uint32_t e0 = 0; e0 < nlive;) {
    uint64_t slots;
    const uint32_t cnt = eg.form(&l_len[e0], nlive - e0, &slots);
    if ((rc = eg.encode(d_in, &l_off[e0], &l_len[e0], cnt, slots))) return rc;
    tables.emplace_back();
    std::vector<ZesGzPackRec>& recs = tables.back();
    uint64_t wgs = 0;
    for (uint32_t k = 0; k < cnt; k++) {
      const uint32_t i = live[e0 + k];
      const uint64_t len = l_len[e0 + k], stored_len = zes_gz_stored_len(len);
      const bool stream = eg.o_cap[k] && eg.raw[k] < stored_len;
      const uint64_t body = stream ? eg.raw[k] : stored_len;
      out_len[i] = 18 + body;
      if (!d_out || out_len[i] > out_cap[i]) {
        status[i] = ZES_E_NOSPACE;
        continue;
      }
      ZesGzPackRec r;
      memset(&r, 0, sizeof r);
      r.src_off = stream ? eg.o_off[k] + 2 : l_off[e0 + k];
      r.dst_off = out_off[i];
      r.body_len = body;
      r.len = (uint32_t)len;
      r.crc = eg.crc[k];
      r.first_wg = (uint32_t)wgs;
      r.stored = stream ? 0u : 1u;
      recs.push_back(r);
      wgs += std::min<uint64_t>(std::max<uint64_t>((body + GZ_GATHER_PIECE - 1) / GZ_GATHER_PIECE, 1), ZES_GZ_PACK_SHARES);
    }
    e0 += cnt;
    if (recs.empty()) continue;
    if (wgs > 0x7fffffffull) return ZES_E_ARG;
    const uint32_t nrec = (uint32_t)recs.size();
    ZesGzPackRec end;
    memset(&end, 0, sizeof end);
    end.first_wg = (uint32_t)wgs;
    recs.push_back(end);
    if ((rc = ensure(g.gz_tab, sizeof(ZesGzPackRec) * recs.size()))) return rc;
    HIPCHK(hipMemcpyAsync(g.gz_tab.p, recs.data(), sizeof(ZesGzPackRec) * recs.size(), hipMemcpyHostToDevice, g.stream));
    {
      Timed t("k_gz_pack");
      hipLaunchKernelGGL(k_gz_pack, dim3((uint32_t)wgs), dim3(GZ_GATHER_THREADS), 0, g.stream, d_in, (const uint8_t*)g.gz_bodies.p, d_out,
                         (const ZesGzPackRec*)g.gz_tab.p, nrec);
    }
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  return ZES_OK;
}

int zes_gzip_batch_bound(const uint64_t* in_len, uint32_t count, uint64_t* cap) {
  if (count && (!in_len || !cap)) return ZES_E_ARG;
  for (uint32_t i = 0; i < count; i++) cap[i] = in_len[i] > GZB_LEN_MAX ? 0 : gzip_batch_cap(in_len[i]);
  return ZES_OK;
}

int zes_gzip_batch_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out, const uint64_t* out_off,
                       const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (count && (!in_off || !out_off || !out_cap)) return ZES_E_ARG;
  bool any = false;
  if (const int arc = gzip_batch_args([&](uint32_t) { return d_in != nullptr; }, in_len, count, out_len, status, flags, &any)) return arc;
  if (!any) {
    call_none();
    return ZES_OK;
  }
  LOCK_READY();
  return call_done(gzip_batch_core(d_in, in_off, in_len, count, d_out, out_off, out_cap, out_len, status, flags), true);
}

int zes_gzip_batch(const uint8_t* const* in, const uint64_t* in_len, uint32_t count, zes_alloc_fn alloc, void* user, uint64_t* out_len, int32_t* status,
                   uint32_t flags) {
  UseDev ud(route_host());
  if (!alloc || (count && !in)) return ZES_E_ARG;
  bool any = false;
  if (const int arc = gzip_batch_args([&](uint32_t i) { return in[i] != nullptr; }, in_len, count, out_len, status, flags, &any)) return arc;
  if (!any) {
    call_none();
    return ZES_OK;
  }
  LOCK_READY();
  // every file gets the bound's room
  HostBatch hb(g.gz_in, g.gz_acc);
  std::vector<uint64_t> in_off(count, 0), out_off(count, 0), out_cap(count, 0);
  for (uint32_t i = 0; i < count; i++) {
    if (status[i] != ZES_OK) continue;
    in_off[i] = hb.place(in[i], in_len[i]);
    out_cap[i] = gzip_batch_cap(in_len[i]);
    out_off[i] = hb.room(out_cap[i]);
  }
  if ((rc = hb.up())) return rc;
  rc = gzip_batch_core(hb.d_in(), in_off.data(), in_len, count, hb.d_out(), out_off.data(), out_cap.data(), out_len, status, flags);
  if ((rc = call_done(rc, true))) return rc;
  return hb.hand_out(count, alloc, user, status, out_len, [&](uint32_t i) { return out_len[i]; }, [&](uint32_t i) { return out_off[i]; });
}

// the first min(len, ZES_GZ_HLEN_MAX) bytes of a file in host memory, for zes_gz_candidate
struct GzHostBytes {
  const uint8_t* h;
  uint32_t avail;
  uint32_t byte(uint32_t i) const { return h[i]; }
  uint32_t nul_from(uint32_t p) const {
    while (p < avail && h[p]) p++;
    return p;
  }
};

// One file of a gunzip batch: where it lies in the source and in the caller's memory (host forms), what k_gz_heads or the
// host rule says of it, where its output goes and how much room that has
struct GzbFile {
  uint64_t off, len;
  const uint8_t* h;
  ZesGzHead head;
  uint64_t dst_off, cap;
};

// Step 1 of the device form: one k_gz_heads launch over every file, one read-back of the records
static int gzb_heads_dev(const uint8_t* d_src, std::vector<GzbFile>& fs) {
  int rc;
  const uint32_t n = (uint32_t)fs.size();
  std::vector<ZesGzFile> tab(n);
  std::vector<ZesGzHead> heads(n);
  Drain drain;  // (behind tab, which an upload reads, and heads, which the read-back writes)
  for (uint32_t i = 0; i < n; i++) tab[i] = ZesGzFile{fs[i].off, fs[i].len, fs[i].cap};
  const size_t o_heads = sizeof(ZesGzFile) * (size_t)n;
  if ((rc = ensure(g.gz_tab, o_heads + sizeof(ZesGzHead) * (size_t)n))) return rc;
  ZesGzHead* d_heads = (ZesGzHead*)((uint8_t*)g.gz_tab.p + o_heads);
  HIPCHK(hipMemcpyAsync(g.gz_tab.p, tab.data(), o_heads, hipMemcpyHostToDevice, g.stream));
  {
    constexpr uint32_t per = ZES_GZ_HEADS_THREADS / 64u;
    Timed t("k_gz_heads");
    hipLaunchKernelGGL(k_gz_heads, dim3((n + per - 1) / per), dim3(ZES_GZ_HEADS_THREADS), 0, g.stream, d_src, (const ZesGzFile*)g.gz_tab.p, d_heads, n);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(heads.data(), d_heads, sizeof(ZesGzHead) * (size_t)n, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  for (uint32_t i = 0; i < n; i++) fs[i].head = heads[i];
  return ZES_OK;
}

// Step 2: the candidates as one batch on the plan of the gzip members (body_plan, one k_gz_gather of the bodies, body_run
// per part): done[i] for a candidate that comes back ZES_OK, whose head.isize bytes then stand at dst + dst_off.  A candidate
// with a status has decided nothing: it is the per-file route's.
static int gzb_batch(const uint8_t* d_src, const std::vector<GzbFile>& fs, uint8_t* dst, uint32_t flags, std::vector<uint8_t>& done) {
  int rc;
  std::vector<uint32_t> ids;
  std::vector<BodyPart> bs;
  for (uint32_t i = 0; i < fs.size(); i++)
    if (fs[i].head.candidate) {
      const ZesGzHead& h = fs[i].head;
      ids.push_back(i);
      bs.push_back(BodyPart{fs[i].len - h.hlen - 8, h.isize, h.crc, fs[i].dst_off, 0u, h.isize, true, ZES_OK});
    }
  if (ids.empty()) return ZES_OK;
  if ((rc = body_plan(bs, dst, 0, true))) return rc;
  std::vector<ZesGzSeg> segs;
  for (size_t k = 0; k < ids.size(); k++) segs.push_back(ZesGzSeg{fs[ids[k]].off + fs[ids[k]].head.hlen, bs[k].islot + 2, bs[k].len, 1u, 0u});
  Drain drain;  // (behind segs, which gz_gather's upload reads)
  if ((rc = gz_gather(d_src, (uint8_t*)g.gz_bodies.p, segs))) return rc;
  if ((rc = body_run(bs, dst, flags & ZES_F_PIECES, false, nullptr))) return rc;
  HIPCHK(hipStreamSynchronize(g.stream));
  drain.done();
  for (size_t k = 0; k < ids.size(); k++) done[ids[k]] = bs[k].status == ZES_OK;
  return ZES_OK;
}

// Step 3, one file: what zes_gunzip_dev does with it alone (gunzip_any), into d_to with capacity cap.  d_to is at a 16-byte
// boundary, and the decoders' whole 16-byte groups have room behind cap.
static int gzb_one(const GzbFile& f, const uint8_t* d_src, uint8_t* d_to, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  *out_len = 0;
  if (f.len == 0) return ZES_E_GZIP;
  GzSrc S{f.h, d_src + f.off, f.len};
  uint64_t hlen = 0;
  int rc = f.h ? gz_header(f.h, f.len, f.len, &hlen) : S.header(0, &hlen);
  if (rc) return rc;
  rc = gunzip_any(S, hlen, true, d_to, cap, out_len, flags & ZES_F_PIECES);
  if (rc && rc != ZES_E_NOSPACE) {
    *out_len = 0;
    (void)hipGetLastError();
  }
  return rc;
}

// The same through g.gz_batch (the decoders write whole 16-byte groups, a file's place may begin and end at any byte): the
// scratch has min(cap, a guess) bytes first and the size needed when the answer is that this was too little; the verdict is
// the one for `cap`.
static int gzb_one_scratch(const GzbFile& f, const uint8_t* d_src, uint64_t cap, uint64_t* out_len, uint32_t flags) {
  int rc;
  uint64_t room = std::min<uint64_t>(cap, std::max<uint64_t>(4 * f.len, 65536));
  for (;;) {
    if ((rc = ensure(g.gz_batch, gz_up16(room) + 64))) return rc;
    rc = gzb_one(f, d_src, (uint8_t*)g.gz_batch.p, room, out_len, flags);
    if (rc != ZES_E_NOSPACE || *out_len > cap || *out_len <= room) return rc;
    room = *out_len;
  }
}

// a gunzip batch of no files: no device work, and nothing of the call before stays
static void gzb_none() {
  call_none();
  std::lock_guard<std::mutex> lk(g_mu);
  g.last_members = 0;
  g.last_gzb[0] = g.last_gzb[1] = 0;
}

static int gunzip_batch_args(const std::function<bool(uint32_t)>& data, const uint64_t* in_len, uint32_t count, uint64_t* out_len, int32_t* status,
                             uint32_t flags) {
  if (flags & ~(ZES_F_PIECES | ZES_F_GZIP_SERIAL)) return ZES_E_ARG;
  if (count && (!in_len || !out_len || !status)) return ZES_E_ARG;
  for (uint32_t i = 0; i < count; i++)
    if (in_len[i] && !data(i)) return ZES_E_ARG;
  return ZES_OK;
}

int zes_gunzip_batch_dev(const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t count, uint8_t* d_out, const uint64_t* out_off,
                         const uint64_t* out_cap, uint64_t* out_len, int32_t* status, uint32_t flags) {
  ROUTE_DEV(d_in, d_out);
  if (count && (!in_off || !out_off || !out_cap)) return ZES_E_ARG;
  if (const int arc = gunzip_batch_args([&](uint32_t) { return d_in != nullptr; }, in_len, count, out_len, status, flags)) return arc;
  for (uint32_t i = 0; i < count; i++)
    if (out_cap[i] && !d_out) return ZES_E_ARG;
  if (!count) {
    gzb_none();
    return ZES_OK;
  }
  LOCK_READY();
  g.carry.clear();
  g.last_tier = 0;
  g.last_members = 0;
  g.last_gzb[0] = g.last_gzb[1] = 0;
  std::vector<GzbFile> fs(count);
  for (uint32_t i = 0; i < count; i++) {
    fs[i] = GzbFile{in_off[i], in_len[i], nullptr, ZesGzHead{0, 0, 0, 0}, out_off[i], out_cap[i]};
    out_len[i] = 0;
    status[i] = ZES_OK;
  }
  std::vector<uint8_t> done(count, 0);
  if (!(flags & ZES_F_GZIP_SERIAL)) {
    if ((rc = gzb_heads_dev(d_in, fs)) || (rc = gzb_batch(d_in, fs, d_out, flags, done))) return call_done(rc, true);
  }
  std::vector<ZesGzSeg> seg(1);
  Drain drain;  // (behind seg, which gz_gather's upload reads)
  for (uint32_t i = 0; i < count; i++) {
    if (done[i]) {
      out_len[i] = fs[i].head.isize;
      g.last_gzb[0]++;
      continue;
    }
    g.last_gzb[1]++;
    uint64_t n = 0;
    rc = gzb_one_scratch(fs[i], d_in, out_cap[i], &n, flags);
    if (rc == ZES_OK && n) {  // (n <= out_cap[i]: exactly the result's bytes go to their place)
      seg[0] = ZesGzSeg{0, out_off[i], n, 0u, 0u};
      int grc = gz_gather((const uint8_t*)g.gz_batch.p, d_out, seg);
      if (!grc && hipStreamSynchronize(g.stream) != hipSuccess) grc = ZES_E_DEVICE;
      if (grc) return call_done(grc, true);
    }
    if (rc == ZES_E_DEVICE) return call_done(rc, true);
    status[i] = rc;
    out_len[i] = n;
  }
  drain.done();
  return call_done(ZES_OK, false);
}

int zes_gunzip_batch_alloc(const uint8_t* const* in, const uint64_t* in_len, uint32_t count, zes_alloc_fn alloc, void* user, uint64_t* out_len,
                           int32_t* status, uint32_t flags) {
  UseDev ud(route_host());
  if (!alloc || (count && !in)) return ZES_E_ARG;
  if (const int arc = gunzip_batch_args([&](uint32_t i) { return in[i] != nullptr; }, in_len, count, out_len, status, flags)) return arc;
  if (!count) {
    gzb_none();
    return ZES_OK;
  }
  LOCK_READY();
  g.carry.clear();
  g.last_tier = 0;
  g.last_members = 0;
  g.last_gzb[0] = g.last_gzb[1] = 0;
  // step 1 on the host; a candidate's output gets its place at once, the others' sizes are known behind their own decode
  HostBatch hb(g.gz_in, g.gz_acc);
  std::vector<GzbFile> fs(count);
  for (uint32_t i = 0; i < count; i++) {
    const uint64_t len = in_len[i];
    GzbFile& f = fs[i];
    f = GzbFile{hb.place(in[i], len), len, in[i], ZesGzHead{0, 0, 0, 0}, 0, 0};
    out_len[i] = 0;
    status[i] = ZES_OK;
    if (len >= 8) f.head.crc = get_le32(in[i] + len - 8), f.head.isize = get_le32(in[i] + len - 4);
    if (!(flags & ZES_F_GZIP_SERIAL)) {
      const GzHostBytes a{in[i], (uint32_t)std::min<uint64_t>(len, ZES_GZ_HLEN_MAX)};
      f.head.candidate = zes_gz_candidate(a, len, ZES_GZB_NO_CAP, f.head.isize, &f.head.hlen) ? 1u : 0u;
    }
    if (f.head.candidate) f.dst_off = hb.room(f.head.isize);
  }
  if ((rc = hb.up())) return rc;
  std::vector<uint8_t> done(count, 0);
  if ((rc = gzb_batch(hb.d_in(), fs, hb.d_out(), flags, done))) return call_done(rc, true);
  // the per-file route: every result waits in host memory until all files have their verdict
  std::vector<std::vector<uint8_t>> kept(count);
  for (uint32_t i = 0; i < count; i++) {
    if (done[i]) {
      out_len[i] = fs[i].head.isize;
      g.last_gzb[0]++;
      continue;
    }
    g.last_gzb[1]++;
    uint64_t n = 0;
    rc = gzb_one_scratch(fs[i], hb.d_in(), ZES_GZB_NO_CAP & ~15ull, &n, flags);
    if (rc == ZES_E_DEVICE) return call_done(rc, true);
    status[i] = rc;
    out_len[i] = rc == ZES_OK ? n : 0;
    if (rc == ZES_OK && n) {
      kept[i].resize(n);
      if ((rc = download(kept[i].data(), (const uint8_t*)g.gz_batch.p, n))) return call_done(rc, true);
    }
  }
  if ((rc = call_done(ZES_OK, false))) return rc;
  for (uint32_t i = 0; i < count; i++) {
    if (status[i] != ZES_OK) continue;
    const uint64_t n = out_len[i];
    uint8_t* to = alloc(user, i, n);
    if (!to) {
      status[i] = ZES_E_ARG;
      out_len[i] = 0;
      continue;
    }
    if (done[i]) {
      if ((rc = download(to, hb.d_out() + fs[i].dst_off, n, nullptr, false))) return rc;
    } else if (n) {
      memcpy(to, kept[i].data(), n);
    }
  }
  HIPCHK(hipStreamSynchronize(g.stream));
  return ZES_OK;
}

int zes_stage_lz77_dev(const uint8_t* d_in, uint64_t n, uint64_t start, uint32_t len, uint32_t* h_tokens, uint32_t* ntokens) {
  ROUTE_DEV(d_in);
  if (!h_tokens || !ntokens || len < 2 || len > ZES_BLK || start + len > n || (start % ZES_BLK)) return ZES_E_ARG;
  LOCK_READY();
  ZesBuf b;
  memset(&b, 0, sizeof b);
  b.in_off = 0;
  b.n = n;  // the halo reads up to the real input end
  b.n_read = n;
  b.nblk = (uint32_t)((n + ZES_BLK - 1) / ZES_BLK);
  ZesBlk z;
  memset(&z, 0, sizeof z);
  z.buf = 0;
  z.blk = (uint32_t)(start / ZES_BLK);
  z.len = len;
  if ((rc = ensure(g.bufs, sizeof b))) return rc;
  if ((rc = ensure(g.blks, sizeof z))) return rc;
  if ((rc = ensure(g.idx_a, (size_t)ZES_BLK * 4))) return rc;
  if ((rc = ensure(g.idx_b, (size_t)ZES_BLK * 4))) return rc;
  if ((rc = ensure(g.sdelta, (size_t)ZES_BLK * 2 + 64))) return rc;
  if ((rc = ensure(g.hists, 320 * 4))) return rc;
  if ((rc = ensure(g.tmask, ZES_TMASK_WORDS * 4))) return rc;
  if ((rc = ensure(g.mlist, ZES_MLIST_WORDS * 4))) return rc;
  HIPCHK(hipMemcpyAsync(g.bufs.p, &b, sizeof b, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipMemcpyAsync(g.blks.p, &z, sizeof z, hipMemcpyHostToDevice, g.stream));
  // the route record: a kernel that leaves before its word (a block without keys, a dense block left to k_lz_index) reports 0
  uint32_t route[ZES_ROUTE_WORDS] = {0};
  memset(g.route, 0, sizeof g.route);
  HIPCHK(hipMemsetAsync((uint32_t*)g.idx_b.p + ZES_BLK - 1, 0, 4, g.stream));
  rc = launch_lz77(d_in, 1, getenv("ZES_NO_INDEX") == nullptr, false, false, [&]() -> int {
    if (const char* dump = getenv("ZES_DUMP_INDEX")) {  // development: the block's index as the match finders will see it
      HIPCHK(hipStreamSynchronize(g.stream));
      std::vector<uint32_t> hinv(ZES_BLK), hflag(1);
      std::vector<uint16_t> hsd(ZES_BLK);
      HIPCHK(hipMemcpy(hinv.data(), g.idx_a.p, ZES_BLK * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(hsd.data(), g.sdelta.p, ZES_BLK * 2, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(hflag.data(), (uint32_t*)g.idx_a.p + ZES_BLK - 1, 4, hipMemcpyDeviceToHost));
      if (FILE* f = fopen(dump, "wb")) {
        fwrite(hflag.data(), 4, 1, f);
        fwrite(hinv.data(), 4, ZES_BLK, f);
        fwrite(hsd.data(), 2, ZES_BLK, f);
        fclose(f);
      }
    }
    return ZES_OK;
  }, route);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&z, g.blks.p, sizeof z, hipMemcpyDeviceToHost, g.stream));
  uint32_t thead[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&route[5], g.mlist.p, 4, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipMemcpyAsync(thead, g.tmask.p, sizeof thead, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  {
    // words of launches the block did not take part in say 0, not what an earlier call left in the pools
    const bool to_index = (route[0] & ZES_SORT_INDEX) != 0u, lazy = route[5] == 0xFFFFFFFFu;
    if (!to_index) route[1] = route[2] = route[4] = 0;
    else route[3] = 0;
    route[6] = lazy ? thead[0] : 0u;
    route[7] = lazy ? thead[1] : 0u;
    route[8] = z.ntok;
    memcpy(g.route, route, sizeof route);
  }
  // (with profiling on the sequence's Timed scopes have recorded: their events go back to the pool; what
  // zes_last_kernel_times reports stays the last pipeline call's)
  for (auto& p : g.pending) g.event_pool.insert(g.event_pool.end(), {p.second.first, p.second.second});
  g.pending.clear();
  *ntokens = z.ntok;
  HIPCHK(hipMemcpy(h_tokens, g.idx_a.p, (size_t)z.ntok * 4, hipMemcpyDeviceToHost));
  return ZES_OK;
}

int zes_stage_lz77_route(uint32_t* words, uint32_t cap) {
  if (!words || cap < ZES_ROUTE_WORDS) return ZES_E_ARG;
  UseDev ud(t_last);  // the context that served this thread's last call
  std::lock_guard<std::mutex> lk(g_mu);
  memcpy(words, g.route, sizeof g.route);
  return ZES_OK;
}

int zes_stage_huff_lengths_dev(const uint32_t* h_hist, uint32_t nsym, uint32_t maxlen, uint8_t* h_lens) {
  if (!h_hist || !h_lens || nsym == 0 || nsym > 288 || maxlen == 0 || maxlen > 15) return ZES_E_ARG;
  LOCK_READY();
  if ((rc = ensure(g.hists, 320 * 4))) return rc;
  if ((rc = ensure(g.codes, 320))) return rc;
  HIPCHK(hipMemcpyAsync(g.hists.p, h_hist, nsym * 4, hipMemcpyHostToDevice, g.stream));
  hipLaunchKernelGGL(k_huff_lengths_only, dim3(1), dim3(HUFF_THREADS_HOST), 0, g.stream, (const uint32_t*)g.hists.p, nsym, maxlen,
                     (uint8_t*)g.codes.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_lens, g.codes.p, nsym, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  return ZES_OK;
}

// (records beyond this many: not a case, ZES_E_ARG — T1's own cap for a stream of 2^29 bytes is 2^23 + 64)
constexpr uint32_t STAGE_CHAIN_MAX = 1u << 20;
int zes_stage_chain(const uint32_t* start_bit, const uint64_t* end_bit, const uint32_t* out_len, const uint32_t* flags, uint32_t count, uint32_t cap,
                    uint32_t first_bit, int on_device, int32_t* status, uint64_t* total, uint32_t* aux, uint32_t* map) {
  if (!status || !total || !aux || count > STAGE_CHAIN_MAX || cap > STAGE_CHAIN_MAX || first_bit < 16) return ZES_E_ARG;
  if (count && (!start_bit || !end_bit || !out_len || !flags || !map)) return ZES_E_ARG;
  const uint32_t n = std::min(count, cap);  // the records a list of `cap` entries holds
  std::vector<ZesCandRes> cres(n);
  std::vector<uint32_t> rel(n);  // the device's form of the start bits
  for (uint32_t k = 0; k < count; k++) {
    if (start_bit[k] < 16 || (k && start_bit[k] <= start_bit[k - 1])) return ZES_E_ARG;
    if (k >= n) continue;
    cres[k] = ZesCandRes{end_bit[k], out_len[k], flags[k]};
    rel[k] = start_bit[k] - 16u;
  }
  ZesInfBuf tab[2] = {};
  tab[0].cand_cap = cap;
  tab[0].start_rel = first_bit - 16u;
  const uint32_t hc[5] = {1u, 0u, 0u, 0u, count};  // the search found something; `count` candidates
  ZesRes r;
  if (!on_device) {  // as a one-buffer call: the launch bound is the cap
    r = t1_host_chain(start_bit, cres.data(), hc, 1u, tab[0], cap, map);
  } else {  // as a buffer of a batch: a work item per candidate of a list that is whole
    LOCK_READY();
    tab[1].work_first = count <= cap ? count : 0u;
    // every list has cap + 1 entries, and the kernel reads min(count, cap) of them
    if ((rc = t1_pools(1, 0, (uint64_t)cap + 1, sizeof hc, 1))) return rc;
    if ((rc = ensure(g.map, (size_t)cap * 4 + 4))) return rc;
    uint32_t* counters = (uint32_t*)g.counters.p;
    HIPCHK(hipMemcpyAsync(g.ibufs.p, tab, sizeof tab, hipMemcpyHostToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(counters, hc, sizeof hc, hipMemcpyHostToDevice, g.stream));
    if (n) {
      HIPCHK(hipMemcpyAsync(g.cand_sorted.p, rel.data(), (size_t)n * 4, hipMemcpyHostToDevice, g.stream));
      HIPCHK(hipMemcpyAsync(g.cres.p, cres.data(), sizeof(ZesCandRes) * n, hipMemcpyHostToDevice, g.stream));
    }
    hipLaunchKernelGGL(k_inf_chain, dim3(1), dim3(256), 0, g.stream, (const ZesInfBuf*)g.ibufs.p, (const uint32_t*)(counters + 4),
                       (const uint32_t*)g.cand_sorted.p, (const ZesCandRes*)g.cres.p, (const uint32_t*)nullptr, (uint32_t*)g.map.p, (ZesRes*)g.res.p,
                       (const uint32_t*)counters, 0u, (uint32_t*)nullptr);
    HIPCHK(hipGetLastError());
    if ((rc = read_res(&r))) return rc;
    if (r.status != 1 && r.aux <= n) HIPCHK(hipMemcpy(map, g.map.p, (size_t)r.aux * 4, hipMemcpyDeviceToHost));
  }
  *status = r.status;
  *total = r.out_len;
  *aux = r.aux;
  return ZES_OK;
}

// one context, its lock held: everything a call could find from an earlier one becomes `word`
static int poison_locked(Ctx& c, uint32_t word, uint64_t* filled) {
  HIPCHK(hipSetDevice(c.device));
  const hipStream_t streams[] = {c.stream, c.cs_in, c.cs_out, c.s_adler};
  for (hipStream_t s : streams) HIPCHK(hipStreamSynchronize(s));
  hipError_t e = hipSuccess;
  for_each_pool(c, [&](DevBuf& b) {
    const size_t words = b.p ? b.cap / 4 : 0;
    if (!words || e != hipSuccess) return;
    e = hipMemsetD32Async((hipDeviceptr_t)b.p, (int)word, words, c.stream);
    *filled += (uint64_t)words * 4;
  });
  HIPCHK(e);
  // the page-locked areas are host memory: no launch is in flight, so the host fills them
  auto fill = [&](void* p, size_t bytes) {
    if (!p) return;
    std::fill((uint32_t*)p, (uint32_t*)p + bytes / 4, word);
    *filled += bytes / 4 * 4;
  };
  fill(c.pinned, PINNED_BYTES);
  fill(c.mirror, sizeof(ParMirror));
  fill(c.res_more, sizeof(ZesRes) * c.res_more_n);
  c.sv.drop();     // (of `surv`)
  c.crc_npow = 0;  // (of `crctab`: crc_ready builds the table again)
  HIPCHK(hipStreamSynchronize(c.stream));
  return ZES_OK;
}

int zes_stage_poison(uint32_t word, uint64_t* bytes) {
  std::lock_guard<std::mutex> cfg(g_cfg_mu);
  uint64_t filled = 0;
  int rc = ZES_OK;
  for (int i = 0; i < ZES_MAX_DEV; i++) {
    std::lock_guard<std::mutex> lk(g_mus[i]);
    if (!g_ctx[i].ready) continue;
    const int r = poison_locked(g_ctx[i], word, &filled);
    if (r && !rc) rc = r;
  }
  if (bytes) *bytes = filled;
  return rc;
}

int zes_selftest_lds_order(uint32_t iters, uint32_t seed, uint64_t* bad, uint64_t* checked) {
  if (!bad || !checked || iters == 0 || iters > 100000u) return ZES_E_ARG;
  LOCK_READY();
  if ((rc = ensure(g.hists, 320 * 4))) return rc;
  HIPCHK(hipMemsetAsync(g.hists.p, 0, 16, g.stream));
  hipLaunchKernelGGL(k_selftest_lds_order, dim3(256), dim3(SORT_THREADS), 0, g.stream, (unsigned long long*)g.hists.p, iters, seed);
  HIPCHK(hipGetLastError());
  unsigned long long h[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(h, g.hists.p, 16, hipMemcpyDeviceToHost, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  *bad = h[0];
  *checked = h[1];
  return ZES_OK;
}

int zes_last_inflate_tier(void) {
  UseDev ud(t_last);  // the context that served this thread's last call (single host calls go round robin over the contexts)
  std::lock_guard<std::mutex> lk(g_mu);
  return g.last_tier;
}

int zes_last_gunzip_members(void) {
  UseDev ud(t_last);
  std::lock_guard<std::mutex> lk(g_mu);
  return g.last_members;
}

int zes_last_gunzip_batch(uint32_t* batched, uint32_t* serial) {
  UseDev ud(t_last);
  std::lock_guard<std::mutex> lk(g_mu);
  if (batched) *batched = g.last_gzb[0];
  if (serial) *serial = g.last_gzb[1];
  return ZES_OK;
}

int zes_set_profiling(int on) {
  std::lock_guard<std::mutex> cfg(g_cfg_mu);
  for (int i = 0; i < ZES_MAX_DEV; i++) {  // every context: a call may be served by any of them
    std::lock_guard<std::mutex> lk(g_mus[i]);
    g_ctx[i].profiling = on != 0;
  }
  return ZES_OK;
}

uint64_t zes_pool_bytes(void) {
  uint64_t total = 0;
  for (int i = 0; i < ZES_MAX_DEV; i++) {
    std::lock_guard<std::mutex> lk(g_mus[i]);
    for_each_pool(g_ctx[i], [&](const DevBuf& b) { total += b.cap; });
  }
  return total;
}

int zes_last_kernel_times(zes_ktime* out, int cap) {
  UseDev ud(t_last);
  std::lock_guard<std::mutex> lk(g_mu);
  int n = 0;
  g.name_pool.clear();
  for (auto& e : g.last_times) g.name_pool.push_back(e.first);
  for (size_t i = 0; i < g.last_times.size() && n < cap; i++, n++) {
    out[n].name = g.name_pool[i].c_str();
    out[n].ms = (float)g.last_times[i].second.ms;
    out[n].launches = g.last_times[i].second.launches;
  }
  return n;
}

}  // extern "C"
