// zes_napi.cc — N-API addon: the binding between the TypeScript façade (zlib.ts) and the C-ABI of
// include/zes.h.  Thin on purpose: argument marshalling and error translation only; every byte
// of work happens in libzes_hip.so (HIP kernels).  Synchronous like the reference's functions
// (src/zlib.ts:11,25); deflateAsync / inflateAsync run the same calls on the libuv thread pool and return
// Promises (the JS thread stays free while a GPU works).  N-API version 3 calls only (Node >= 10).
#include <node_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <csignal>
#include <execinfo.h>
#include <unistd.h>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/zes.h"

namespace {

napi_value throw_status(napi_env env, int status) {
  // plain `Error` with the reference's exact message (src/zlib.ts:15, src/inflate.ts:32,35,50,...)
  napi_throw_error(env, nullptr, zes_strerror(status));
  return nullptr;
}
napi_value throw_type(napi_env env, const std::string& text) {
  napi_throw_type_error(env, nullptr, text.c_str());
  return nullptr;
}
// the same plain `Error` as an object: what a promise is rejected with and what stands for a failed buffer of a batch
napi_value make_error(napi_env env, const char* text) {
  napi_value msg, err = nullptr;
  napi_create_string_utf8(env, text, NAPI_AUTO_LENGTH, &msg);
  napi_create_error(env, nullptr, msg, &err);
  return err;
}
napi_value undefined_unless(napi_env env, int rc) {
  if (rc) return throw_status(env, rc);
  napi_value v;
  napi_get_undefined(env, &v);
  return v;
}

bool get_bytes(napi_env env, napi_value v, const uint8_t** data, size_t* len) {
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) == napi_ok && is_ta) {
    napi_typedarray_type type;
    void* p = nullptr;
    size_t n = 0;
    napi_value ab;
    size_t off;
    if (napi_get_typedarray_info(env, v, &type, &n, &p, &ab, &off) != napi_ok) return false;
    if (type != napi_uint8_array && type != napi_uint8_clamped_array && type != napi_int8_array) return false;
    *data = static_cast<const uint8_t*>(p);
    *len = n;
    return true;
  }
  bool is_buf = false;
  if (napi_is_buffer(env, v, &is_buf) == napi_ok && is_buf) {
    void* p = nullptr;
    size_t n = 0;
    if (napi_get_buffer_info(env, v, &p, &n) != napi_ok) return false;
    *data = static_cast<const uint8_t*>(p);
    *len = n;
    return true;
  }
  return false;
}

// ---- result memory ----
// A result is a fresh Uint8Array with its own exact-length ArrayBuffer (src/zlib.ts:42).  Fresh memory is what a large call
// pays most for on the host side: 64 MiB of untouched pages are 16 384 page faults under the copy that fills them, ~30 ms
// where the GPU's work and both trips over PCIe take 2.5.  So results of 1 MiB and more live in blocks of page-locked memory
// (zes_host_alloc: no faults, and the copy engines write them directly) that come back to a small pool when the ArrayBuffer is
// collected and are handed out again.  Node runs the finalizers of external ArrayBuffers between event-loop turns, not
// inside a synchronous loop: a host that awaits (deflateAsync / inflateAsync, any server) gets its blocks back and runs at
// the library's pace; a tight synchronous loop over 64 MiB calls gets fresh blocks until BIG_OUTSTANDING_MAX are out, then
// plain malloc as before.  trim() empties the pool.
// Set when the last environment (or the process) goes down: from then on nothing here calls into the library or the HIP
// runtime any more — page-locked blocks are left to the process's end.
std::atomic<bool> g_exiting{false};
std::atomic<long> g_dbg_hit{0}, g_dbg_miss{0}, g_dbg_released{0};
std::atomic<int> g_envs{0};
void mark_exiting_atexit() { g_exiting.store(true); }

constexpr size_t BIG_MIN = 1u << 20;                 // smaller results: malloc, as before
constexpr size_t BIG_KEEP_MAX = 768u << 20;          // bytes the pool keeps for reuse
constexpr size_t BIG_OUTSTANDING_MAX = 1024u << 20;  // (V8 collects a few calls behind: 64 MiB calls in an awaited loop hold ~0.5 GiB at any time)  // pooled bytes in the hands of JS beyond which new results are not pooled
struct BigPool {
  struct Blk {
    uint8_t* p;
    size_t cap;
  };
  std::mutex mu;
  std::vector<Blk> free_;
  size_t kept = 0, out = 0;
  size_t want = 0;  // a request the pool could not serve from inside the library (see take): the next top_up() gets such a block
  // a block of at least n bytes, or nullptr (the caller falls back to malloc).  fresh = false: from inside one of the
  // library's allocator callbacks — they run under the library's lock, and a new page-locked block comes from the library
  // (zes_host_alloc takes that lock): only what the pool holds; the miss is noted and made good after the call.
  uint8_t* take(size_t n, size_t* cap, bool fresh, bool note_miss = true) {
    {
      std::lock_guard<std::mutex> lk(mu);
      size_t best = free_.size();
      for (size_t i = 0; i < free_.size(); i++)
        if (free_[i].cap >= n && free_[i].cap <= 2 * n + (8u << 20) && (best == free_.size() || free_[i].cap < free_[best].cap)) best = i;
      if (best != free_.size()) {
        g_dbg_hit++;
        Blk b = free_[best];
        free_.erase(free_.begin() + (long)best);
        kept -= b.cap;
        out += b.cap;
        *cap = b.cap;
        return b.p;
      }
      g_dbg_miss++;
      if (out + n > BIG_OUTSTANDING_MAX) return nullptr;
      if (!fresh) {
        if (note_miss) want = n > want ? n : want;
        return nullptr;
      }
    }
    void* p = nullptr;
    const size_t want = (n + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
    if (zes_host_alloc(want, &p) != 0 || !p) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    out += want;
    *cap = want;
    return static_cast<uint8_t*>(p);
  }
  void give(uint8_t* p, size_t cap) {
    if (g_exiting.load()) return;
    {
      std::lock_guard<std::mutex> lk(mu);
      out -= cap < out ? cap : out;
      if (kept + cap <= BIG_KEEP_MAX) {
        free_.push_back({p, cap});
        kept += cap;
        return;
      }
    }
    zes_host_free(p);
  }
  // after a library call whose callback missed: one block of the size it asked for, for the next call of that kind
  void top_up() {
    size_t n = 0;
    {
      std::lock_guard<std::mutex> lk(mu);
      n = want;
      want = 0;
      if (!n || out + kept + n > BIG_OUTSTANDING_MAX) return;
    }
    void* p = nullptr;
    const size_t cap = (n + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
    if (zes_host_alloc(cap, &p) != 0 || !p) return;
    std::lock_guard<std::mutex> lk(mu);
    if (kept + cap <= BIG_KEEP_MAX) {
      free_.push_back({static_cast<uint8_t*>(p), cap});
      kept += cap;
      return;
    }
    zes_host_free(p);  // (cannot happen under the limits above; never keep more than the budget)
  }
  void clear() {
    if (g_exiting.load()) return;
    std::vector<Blk> all;
    {
      std::lock_guard<std::mutex> lk(mu);
      all.swap(free_);
      kept = 0;
    }
    for (Blk& b : all) zes_host_free(b.p);
  }
};
BigPool& g_big = *new BigPool;  // (never destroyed: an environment's cleanup may still come by during exit())

// memory for a result of up to n bytes: pooled (cap > 0) or malloc'd (cap == 0)
struct ResultMem {
  uint8_t* p = nullptr;
  size_t cap = 0;
};
// only what the pool holds (fresh = false: what may be asked from inside one of the library's calls), or nothing
ResultMem pooled(size_t n, bool note_miss = true) {
  ResultMem m;
  if (n >= BIG_MIN) m.p = g_big.take(n, &m.cap, false, note_miss);
  if (!m.p) m.cap = 0;
  return m;
}
ResultMem result_malloc(size_t n) {
  ResultMem m;
  m.p = static_cast<uint8_t*>(malloc(n ? n : 1));
  return m;
}
ResultMem result_alloc(size_t n, bool fresh = true) {
  ResultMem m;
  if (n >= BIG_MIN) m.p = g_big.take(n, &m.cap, fresh);
  return m.p ? m : result_malloc(n);
}
void result_free(ResultMem m) {
  if (!m.p) return;
  if (m.cap)
    g_big.give(m.p, m.cap);
  else
    free(m.p);
}

// A synchronous deflate() that finds no pooled block (a tight loop: Node runs no finalizer inside it) would hand the
// library ~64 MiB of untouched malloc'd memory to download into piece by piece — every page faulted under the copy
// engine's hands, ~40 ms.  Instead the library writes into ONE page-locked scratch block the addon keeps for this purpose,
// and the exact-length result is copied out of it by a few threads (the faults of the fresh result spread over them).
// One block per environment (EnvState): a synchronous call owns it from get() until the copy out of it is done, and
// two environments' JS threads run such calls side by side.
struct SyncScratch {
  uint8_t* p = nullptr;
  size_t cap = 0;
  uint8_t* get(size_t n) {
    if (n <= cap) return p;
    clear();
    void* q = nullptr;
    const size_t want = (n + (4u << 20) - 1) & ~(size_t)((4u << 20) - 1);
    if (zes_host_alloc(want, &q) != 0 || !q) return nullptr;
    p = static_cast<uint8_t*>(q);
    cap = want;
    return p;
  }
  void clear() {
    if (p) zes_host_free(p);
    p = nullptr;
    cap = 0;
  }
};

// ---- whose memory is still in use: no finalizers ----
// The memory behind an array handed to JS (a result, an allocPinned() array) is an external ArrayBuffer WITHOUT a finalizer;
// the addon keeps a weak reference to it and looks, at the start of every call, which of them the collector has cleared:
// those blocks go back (to the pool, to the library, to free()).  Why not a finalizer: Node 12 hands an N-API finalizer to
// the environment's immediate queue without keeping the N-API environment alive, frees that environment in a cleanup hook
// when the process ends, and runs the queue afterwards — v8::HandleScope on freed memory: seven of ten bench_host.js runs
// ended in SIGSEGV behind their last line (any array alive at exit has its finalizer queued there).  And a finalizer only
// ever runs between two turns of the event loop, so a synchronous loop over deflate() got fresh memory for every result,
// page by page; a weak reference is cleared by the collection itself, and the next call of the loop has the block again.
struct Track {
  napi_ref ref;   // weak: to the ArrayBuffer
  uint8_t* p;
  size_t cap;     // pooled block: its capacity; 0: malloc'd (results) — or page-locked by allocPinned (pinned)
  int64_t told;   // bytes reported with napi_adjust_external_memory
  bool pinned;    // allocPinned(): goes back with zes_host_free
};
// what one environment owns: the arrays it handed to JS and what its synchronous calls keep between them
struct EnvState {
  napi_env env;
  std::vector<Track> v;
  size_t cursor = 0;
  SyncScratch scratch;
  size_t last_inflate_out = 0;  // what the last synchronous inflate produced (Inflate sizes the scratch block by it)
};
std::mutex g_tracks_mu;
std::vector<EnvState*> g_tracks;  // one per environment (a Worker has its own); an entry is used by its environment's thread only
EnvState* tracks_of(napi_env env) {
  std::lock_guard<std::mutex> lk(g_tracks_mu);
  for (EnvState* t : g_tracks)
    if (t->env == env) return t;
  return nullptr;
}
void release_memory(const Track& t) {
  if (t.pinned) {
    if (!g_exiting.load()) zes_host_free(t.p);
  } else {
    ResultMem m;
    m.p = t.p;
    m.cap = t.cap;
    result_free(m);
  }
}
constexpr size_t SWEEP_MAX = 4096;  // references looked at per call (a host that keeps more arrays alive is swept in turns)
void sweep(napi_env env) {
  EnvState* et = tracks_of(env);
  if (!et || et->v.empty()) return;
  size_t todo = et->v.size() < SWEEP_MAX ? et->v.size() : SWEEP_MAX;
  size_t i = et->cursor < et->v.size() ? et->cursor : 0;
  while (todo--) {
    if (i >= et->v.size()) i = 0;
    if (et->v.empty()) break;
    napi_value val = nullptr;
    if (napi_get_reference_value(env, et->v[i].ref, &val) == napi_ok && val == nullptr) {
      const Track t = et->v[i];
      et->v[i] = et->v.back();
      et->v.pop_back();
      napi_delete_reference(env, t.ref);
      if (t.told) {
        int64_t now = 0;
        napi_adjust_external_memory(env, -t.told, &now);
      }
      release_memory(t);
      g_dbg_released++;
    } else {
      i++;
    }
  }
  et->cursor = i;
}
// the environment goes down: its arrays and its scratch block with it (no N-API call from here; pooled blocks stay pooled
// for other environments)
void env_cleanup(void* arg) {
  napi_env env = static_cast<napi_env>(arg);
  EnvState* mine = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_tracks_mu);
    for (size_t i = 0; i < g_tracks.size(); i++)
      if (g_tracks[i]->env == env) {
        mine = g_tracks[i];
        g_tracks.erase(g_tracks.begin() + (long)i);
        break;
      }
  }
  if (getenv("ZES_NAPI_DEBUG"))
    fprintf(stderr, "zes_napi: pool hits %ld misses %ld, arrays released by sweeps %ld, still tracked %zu\n", g_dbg_hit.load(), g_dbg_miss.load(),
            g_dbg_released.load(), mine ? mine->v.size() : 0);
  const bool last = g_envs.fetch_sub(1) == 1;
  if (last) g_exiting.store(true);
  if (mine) {
    if (!last) {
      for (const Track& t : mine->v) release_memory(t);
      mine->scratch.clear();
    }
    delete mine;
  }
}
// hands p[0, n) to JS as the ArrayBuffer of a fresh Uint8Array and starts tracking it; on failure the memory is released
napi_value adopt(napi_env env, uint8_t* p, size_t n, size_t cap, bool pinned) {
  Track t;
  t.ref = nullptr;
  t.p = p;
  t.cap = cap;
  t.told = (int64_t)(cap ? cap : n);
  t.pinned = pinned;
  EnvState* et = tracks_of(env);
  napi_value ab, ta;
  if (!et || napi_create_external_arraybuffer(env, p, n, nullptr, nullptr, &ab) != napi_ok) {
    release_memory(t);
    return nullptr;
  }
  if (napi_create_reference(env, ab, 0, &t.ref) != napi_ok) {  // (the ArrayBuffer is garbage from here; its memory must outlive it: kept)
    napi_throw_error(env, nullptr, "zes: out of memory");
    return nullptr;
  }
  int64_t now = 0;
  if (napi_adjust_external_memory(env, t.told, &now) != napi_ok) t.told = 0;
  et->v.push_back(t);
  if (napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta) != napi_ok) return nullptr;  // (tracked: released once collected)
  return ta;
}
// the result's memory becomes its ArrayBuffer (exact length: `buffer.byteLength === length` like src/zlib.ts:42; a pooled
// block is longer than what the ArrayBuffer shows of it): no second copy of the result on the JS thread.  Takes the
// memory over (gives it back on failure).  V8 is told how much memory hangs on the object — it does not count an external
// ArrayBuffer's bytes by itself — so that a loop over large calls makes it collect, and the blocks come back to the pool.
napi_value take_u8(napi_env env, ResultMem m, size_t n) {
  if (!m.cap) {
    void* shrunk = realloc(m.p, n ? n : 1);
    if (shrunk) m.p = static_cast<uint8_t*>(shrunk);
  }
  return adopt(env, m.p, n, m.cap, false);
}

// ---- arguments ----
struct Args {
  size_t argc = 4;  // (in: the length of argv, the longest signature's; out: how many the caller passed)
  napi_value argv[4];  // (the ones not passed are undefined)
};
Args get_args(napi_env env, napi_callback_info info) {
  Args a;
  napi_get_cb_info(env, info, &a.argc, a.argv, nullptr, nullptr);
  return a;
}

// argument i as bytes, or (ok = false) the TypeError "<sig>: <name> must be a Uint8Array" is thrown
struct Bytes {
  const uint8_t* p = nullptr;
  size_t n = 0;
  bool ok = false;
};
Bytes need_bytes(napi_env env, const Args& a, size_t i, const char* sig, const char* name) {
  Bytes b;
  b.ok = i < a.argc && get_bytes(env, a.argv[i], &b.p, &b.n);
  if (!b.ok) throw_type(env, std::string(sig) + ": " + name + " must be a Uint8Array");
  return b;
}

// a non-negative safe integer given as a number — nothing else: null, a string, a bigint are not numbers
bool get_safe_uint(napi_env env, napi_value v, uint64_t* out) {
  double d = 0;
  if (napi_get_value_double(env, v, &d) != napi_ok || !(d >= 0) || d > 9007199254740991.0 || d != (double)(uint64_t)d) return false;
  *out = (uint64_t)d;
  return true;
}
// a position or length: that, or a bigint below 2^64
bool get_offset(napi_env env, napi_value v, uint64_t* out) {
  napi_valuetype vt;
  if (napi_typeof(env, v, &vt) != napi_ok) return false;
  if (vt != napi_bigint) return get_safe_uint(env, v, out);
  bool lossless = false;
  return napi_get_value_bigint_uint64(env, v, out, &lossless) == napi_ok && lossless;
}
int32_t int32_or_0(napi_env env, napi_value v) {
  int32_t x = 0;
  napi_get_value_int32(env, v, &x);  // (not a number: x stays 0)
  return x;
}

// the optional `options` argument of the inflate forms, { verify?: boolean }: ZES_F_CHECK_ADLER when verify is true, else
// nothing (no second argument, undefined, null, an object without the property: the call is the one-argument call)
uint32_t verify_flag(napi_env env, const Args& a, size_t at) {
  if (a.argc <= at) return 0;
  napi_valuetype t = napi_undefined;
  if (napi_typeof(env, a.argv[at], &t) != napi_ok || t != napi_object) return 0;
  napi_value v;
  bool on = false;
  if (napi_get_named_property(env, a.argv[at], "verify", &v) != napi_ok || napi_typeof(env, v, &t) != napi_ok || t != napi_boolean) return 0;
  return napi_get_value_bool(env, v, &on) == napi_ok && on ? ZES_F_CHECK_ADLER : 0;
}

// ---- the bounded result ----
// A call that writes at most a known number of bytes into memory it is given: fill() makes the call and gives the memory
// back when it answers a status (no N-API call: the worker thread of deflateAsync fills too); as_u8() turns what fill()
// left into the exact-length Uint8Array or the thrown Error; bounded() is both, the whole of most synchronous entry points.
struct Filled {
  ResultMem m;
  uint64_t len = 0;
  int rc = 0;
};
template <class Call>  // int call(uint8_t* out, uint64_t* out_len)
Filled fill(ResultMem m, Call call) {
  Filled f;
  f.m = m;
  f.rc = m.p ? call(m.p, &f.len) : ZES_E_ARG;
  if (f.rc) {
    result_free(f.m);
    f.m = ResultMem();
  }
  return f;
}
napi_value as_u8(napi_env env, const Filled& f) { return f.rc ? throw_status(env, f.rc) : take_u8(env, f.m, (size_t)f.len); }
template <class Call>
napi_value bounded(napi_env env, ResultMem m, Call call) {
  return as_u8(env, fill(m, call));
}

void copy_parallel(uint8_t* dst, const uint8_t* src, size_t n) {
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned nt = n < (8u << 20) ? 1u : (hw >= 8 ? 4u : 2u);
  if (nt == 1) {
    memcpy(dst, src, n);
    return;
  }
  std::vector<std::thread> th;
  const size_t part = ((n / nt) + 4095) & ~(size_t)4095;
  for (unsigned i = 1; i < nt; i++) {
    const size_t o = i * part;
    if (o < n) th.emplace_back([=] { memcpy(dst + o, src + o, (o + part < n) ? part : n - o); });
  }
  memcpy(dst, src, part < n ? part : n);
  for (auto& t : th) t.join();
}
// the result a call left at the head of the scratch block, copied out into m
napi_value out_of_scratch(napi_env env, const uint8_t* scratch, ResultMem m, uint64_t len) {
  if (!m.p) return throw_status(env, ZES_E_ARG);
  copy_parallel(m.p, scratch, (size_t)len);
  return take_u8(env, m, (size_t)len);
}

// ---- zes_alloc_fn: the library asks for the result's memory from inside its call ----
// The exact-size leg of every such callback: the block handed out before goes back (ZES_F_ALLOC_BOUND: a second call when
// the first one's estimate fell short, or the call started over), then a pooled block or malloc — never zes_host_alloc,
// which takes the lock the library is holding.
struct ExactMem {
  ResultMem m;
  bool failed = false;
  void drop() {
    result_free(m);
    m = ResultMem();
  }
  uint8_t* renew(size_t n) {
    drop();
    m = result_alloc(n, false);
    if (!m.p) failed = true;
    return m.p;
  }
};
uint8_t* exact_alloc(void* user, uint32_t, uint64_t n) { return static_cast<ExactMem*>(user)->renew((size_t)n); }  // gunzip: no early request

// the synchronous inflate's: runs on the JS thread, inside zes_inflate_alloc
struct SyncAlloc : ExactMem {
  const SyncScratch* scratch = nullptr;  // its environment's
  bool in_scratch = false;  // the early estimate was served from the scratch block: the result is copied out of it afterwards
};
uint8_t* sync_alloc(void* user, uint32_t index, uint64_t n) {
  SyncAlloc* a = static_cast<SyncAlloc*>(user);
  a->in_scratch = false;
  if (!(index & ZES_ALLOC_EARLY)) return a->renew((size_t)n);
  // an early request (ZES_F_ALLOC_BOUND: an upper estimate, the bytes then come down beside the decode) is only worth
  // taking with page-locked memory: downloads piece by piece into fresh malloc'd memory pay its page faults the slow way.
  // A pooled block if the pool holds one; else the scratch block when it is long enough (grown outside the library's call,
  // from what the calls before needed): the exact-length result is copied out by a few threads afterwards — a tight
  // loop's results are fresh memory either way, but this way its page faults are spread over the copy's threads instead
  // of being taken under the copy engine, and no block is page-locked for the next call (a loop over 64 MiB results
  // alternated between 2.5 ms and 25 ms a call)
  a->drop();
  a->m = pooled((size_t)n, false);
  if (a->m.p) return a->m.p;
  if (a->scratch && a->scratch->p && n <= a->scratch->cap) {
    a->in_scratch = true;
    return a->scratch->p;
  }
  a->m = pooled((size_t)n);  // (notes the miss: the pool is topped up after the call)
  return a->m.p;             // (nullptr unless a block came back meanwhile: "not now" — the exact size is asked for once, later)
}

napi_value Deflate(napi_env env, napi_callback_info info) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, "deflate(input)", "input");
  if (!in.ok) return nullptr;
  uint64_t cap = 0;
  zes_deflate_bound(in.n, &cap);
  ResultMem tmp = pooled(cap);  // a block the pool holds, if any
  if (!tmp.p && cap >= (4u << 20)) {  // none (a tight synchronous loop): through this environment's scratch block, see SyncScratch
    EnvState* es = tracks_of(env);
    uint8_t* sc = es ? es->scratch.get(cap) : nullptr;
    if (sc) {
      uint64_t out_len = 0;
      const int rc = zes_deflate(in.p, in.n, sc, cap, &out_len);
      return rc ? throw_status(env, rc) : out_of_scratch(env, sc, result_malloc(out_len), out_len);
    }
  }
  return bounded(env, tmp.p ? tmp : result_alloc(cap, false), [&](uint8_t* out, uint64_t* len) { return zes_deflate(in.p, in.n, out, cap, len); });
}

napi_value Inflate(napi_env env, napi_callback_info info) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, "inflate(input)", "input");
  if (!in.ok) return nullptr;
  // one call, one lock: the library decodes, then asks for the exact ArrayBuffer (the reference grows a
  // Uint8WriteStream instead, src/inflate.ts:17) and copies straight into it — nothing is kept between calls,
  // so an inflateAsync() in flight on a worker thread cannot get in between
  SyncAlloc sa;
  uint64_t out_len = 0;
  // the scratch block, long enough for what this environment's last synchronous inflate produced (a loop decodes like
  // after like) and never shorter than the stream: grown here, outside the library's call
  EnvState* es = tracks_of(env);
  if (es) {
    const size_t last = es->last_inflate_out;
    const size_t want = last > in.n ? last + last / 16 + (1u << 20) : 0;
    if (want >= (4u << 20) && want <= (1024u << 20)) (void)es->scratch.get(want);
    sa.scratch = &es->scratch;
  }
  // (the pooled block is longer than the ArrayBuffer shows of it anyway: the library may ask early for an upper estimate and
  // send the bytes down while it is still decoding)
  // (with ZES_F_CHECK_ADLER the library takes its one-pass path, where ZES_F_ALLOC_BOUND asks for nothing early)
  const int rc = zes_inflate_alloc(in.p, in.n, sync_alloc, &sa, &out_len, ZES_F_ALLOC_BOUND | verify_flag(env, a, 1));
  if (!sa.in_scratch) g_big.top_up();
  if (rc) {
    sa.drop();
    return throw_status(env, sa.failed ? ZES_E_ARG : rc);
  }
  if (es) es->last_inflate_out = (size_t)out_len;
  if (!sa.in_scratch) return take_u8(env, sa.m, (size_t)out_len);
  // (the estimate held: the result is the scratch block's head)
  const ResultMem m = pooled((size_t)out_len, false);
  return out_of_scratch(env, sa.scratch->p, m.p ? m : result_malloc((size_t)out_len), out_len);
}

// deflateRaw(input): the raw stream of the reference's src/deflate.ts:14 (no zlib wrapper)
napi_value DeflateRaw(napi_env env, napi_callback_info info) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, "deflateRaw(input)", "input");
  if (!in.ok) return nullptr;
  uint64_t cap = 0;
  zes_deflate_bound(in.n, &cap);
  return bounded(env, result_alloc(cap), [&](uint8_t* out, uint64_t* len) { return zes_deflate_raw(in.p, in.n, out, cap, len); });
}

// inflateRaw(input, offset = 0): the reference's src/inflate.ts:16 (what src/zlib.ts:21 calls with offset 2)
napi_value InflateRaw(napi_env env, napi_callback_info info) {
  static const char SIG[] = "inflateRaw(input, offset)";
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, SIG, "input");
  if (!in.ok) return nullptr;
  uint64_t offset = 0;
  napi_valuetype vt = napi_undefined;
  if (napi_typeof(env, a.argv[1], &vt) != napi_ok || (vt != napi_undefined && !get_safe_uint(env, a.argv[1], &offset)))
    return throw_type(env, std::string(SIG) + ": offset must be a non-negative safe integer");
  // grow-and-retry like the reference's Uint8WriteStream (src/utils/Uint8WriteStream.ts:13-21)
  uint64_t cap = in.n * 4 + 65536;
  for (int attempt = 0; attempt < 8; attempt++) {
    const Filled f = fill(result_alloc(cap), [&](uint8_t* out, uint64_t* len) { return zes_inflate_raw(in.p, in.n, offset, out, cap, len, ZES_F_DEFAULT); });
    if (f.rc != ZES_E_NOSPACE || f.len <= cap) return as_u8(env, f);
    cap = f.len;
  }
  return throw_status(env, ZES_E_DEVICE);
}

// gzip(input): one gzip member (RFC 1952) whose body is the reference's raw stream (include/zes.h: zes_gzip)
napi_value Gzip(napi_env env, napi_callback_info info) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, "gzip(input)", "input");
  if (!in.ok) return nullptr;
  uint64_t cap = 0;
  zes_gzip_bound(in.n, &cap);
  return bounded(env, result_alloc(cap), [&](uint8_t* out, uint64_t* len) { return zes_gzip(in.p, in.n, out, cap, len); });
}

// bgzip(input) / bgzipIndex(input): a BGZF file, a gzip member per 65280-byte chunk and the end-of-file marker
// (include/zes.h: zes_bgzip); with_index: { data, offsets } with the position of every member, the marker's last
napi_value bgzip_common(napi_env env, napi_callback_info info, bool with_index) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, with_index ? "bgzipIndex(input)" : "bgzip(input)", "input");
  if (!in.ok) return nullptr;
  uint64_t cap = 0, members = 0;
  if (zes_bgzip_bound(in.n, &cap) || zes_bgzip_members(in.n, &members)) return throw_status(env, ZES_E_ARG);
  std::vector<uint64_t> off(with_index ? (size_t)members : 0);
  napi_value data = bounded(env, result_alloc(cap), [&](uint8_t* out, uint64_t* len) {
    return zes_bgzip(in.p, in.n, out, cap, len, with_index ? off.data() : nullptr, ZES_F_DEFAULT);
  });
  if (!with_index || !data) return data;
  napi_value res, arr;
  if (napi_create_object(env, &res) != napi_ok || napi_create_array_with_length(env, off.size(), &arr) != napi_ok) return nullptr;
  for (size_t i = 0; i < off.size(); i++) {
    napi_value v;
    if (napi_create_double(env, (double)off[i], &v) != napi_ok) return nullptr;  // (far below 2^53)
    napi_set_element(env, arr, (uint32_t)i, v);
  }
  napi_set_named_property(env, res, "data", data);
  napi_set_named_property(env, res, "offsets", arr);
  return res;
}
napi_value Bgzip(napi_env env, napi_callback_info info) { return bgzip_common(env, info, false); }
napi_value BgzipIndex(napi_env env, napi_callback_info info) { return bgzip_common(env, info, true); }

// bgzfIndex(file): the member index of a BGZF file, { compressed, uncompressed }: two BigUint64Arrays of members + 1 entries
// (include/zes.h: zes_bgzf_index, the host form: no device is touched)
napi_value BgzfIndex(napi_env env, napi_callback_info info) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, "bgzfIndex(file)", "file");
  if (!in.ok) return nullptr;
  uint64_t members = 0;
  int rc = zes_bgzf_index(in.p, in.n, nullptr, nullptr, 0, &members, ZES_F_DEFAULT);  // (the count: ZES_E_NOSPACE on a valid file)
  if (rc != ZES_E_NOSPACE) return throw_status(env, rc ? rc : ZES_E_ARG);
  napi_value res, ab[2], ta[2];
  void* mem[2] = {nullptr, nullptr};
  const size_t entries = (size_t)members + 1;
  for (int k = 0; k < 2; k++)
    if (napi_create_arraybuffer(env, entries * 8, &mem[k], &ab[k]) != napi_ok || napi_create_typedarray(env, napi_biguint64_array, entries, ab[k], 0, &ta[k]) != napi_ok)
      return nullptr;
  rc = zes_bgzf_index(in.p, in.n, static_cast<uint64_t*>(mem[0]), static_cast<uint64_t*>(mem[1]), entries, &members, ZES_F_DEFAULT);
  if (rc) return throw_status(env, rc);
  if (napi_create_object(env, &res) != napi_ok) return nullptr;
  napi_set_named_property(env, res, "compressed", ta[0]);
  napi_set_named_property(env, res, "uncompressed", ta[1]);
  return res;
}

bool get_u64_array(napi_env env, napi_value v, const uint64_t** data, size_t* len) {
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return false;
  napi_typedarray_type type;
  void* p = nullptr;
  napi_value ab;
  size_t off;
  if (napi_get_typedarray_info(env, v, &type, len, &p, &ab, &off) != napi_ok || type != napi_biguint64_array) return false;
  *data = static_cast<const uint64_t*>(p);
  return true;
}

// bgzfRead(file, index, pos, len): bytes [pos, pos + len) of the uncompressed data, clipped at its end, through the index
// bgzfIndex(file) returned; only the members that hold the range are uploaded and decoded (include/zes.h: zes_bgzf_read)
napi_value BgzfRead(napi_env env, napi_callback_info info) {
  static const char SIG[] = "bgzfRead(file, index, pos, len)";
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, SIG, "file");
  if (!in.ok) return nullptr;
  const uint64_t *coff = nullptr, *uoff = nullptr;
  size_t nc = 0, nu = 0;
  napi_value vc, vu;
  if (napi_get_named_property(env, a.argv[1], "compressed", &vc) != napi_ok || napi_get_named_property(env, a.argv[1], "uncompressed", &vu) != napi_ok ||
      !get_u64_array(env, vc, &coff, &nc) || !get_u64_array(env, vu, &uoff, &nu) || nc != nu || nc < 2)
    return throw_type(env, std::string(SIG) + ": index must be what bgzfIndex(file) returned");
  uint64_t pos = 0, len = 0;
  if (!get_offset(env, a.argv[2], &pos) || !get_offset(env, a.argv[3], &len))
    return throw_type(env, std::string(SIG) + ": pos and len must be non-negative safe integers or bigints");
  const uint64_t total = uoff[nu - 1];
  const uint64_t cap = pos <= total ? std::min<uint64_t>(len, total - pos) : 0;  // (pos > total: the library answers ZES_E_ARG)
  return bounded(env, result_alloc((size_t)cap), [&](uint8_t* out, uint64_t* out_len) {
    return zes_bgzf_read(in.p, in.n, coff, uoff, nu - 1, pos, len, out, cap, out_len, ZES_F_DEFAULT);
  });
}

// gunzip(input): every member of a gzip file, their outputs concatenated; one decode, then the exact-size result
napi_value Gunzip(napi_env env, napi_callback_info info) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, "gunzip(input)", "input");
  if (!in.ok) return nullptr;
  ExactMem ga;
  uint64_t out_len = 0;
  const int rc = zes_gunzip_alloc(in.p, in.n, exact_alloc, &ga, &out_len, ZES_F_DEFAULT);
  if (rc) {
    ga.drop();
    return throw_status(env, ga.failed ? ZES_E_ARG : rc);
  }
  return take_u8(env, ga.m, (size_t)out_len);
}

napi_value Adler32(napi_env env, napi_callback_info info) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, "adler32(input)", "input");
  if (!in.ok) return nullptr;
  uint32_t sum = 0;
  const int rc = zes_adler32(in.p, in.n, &sum);
  if (rc) return throw_status(env, rc);
  napi_value v;
  napi_create_uint32(env, sum, &v);
  return v;
}

napi_value Init(napi_env env, napi_callback_info info) { return undefined_unless(env, zes_init(int32_or_0(env, get_args(env, info).argv[0]))); }

// initDevices(n): one process, n GPUs (n omitted or <= 0: every visible one) — the batch calls then partition their
// buffers over all of them, single calls take them in turn (zes_init_devices).  Returns the number of devices in use.
napi_value InitDevices(napi_env env, napi_callback_info info) {
  const int rc = zes_init_devices(int32_or_0(env, get_args(env, info).argv[0]));
  if (rc) return throw_status(env, rc);
  napi_value v;
  napi_create_int32(env, zes_device_count(), &v);
  return v;
}

// lastGunzipMembers(): members the member-parallel path decoded in this thread's last gunzip() (zes_last_gunzip_members)
napi_value LastGunzipMembers(napi_env env, napi_callback_info) {
  napi_value v;
  napi_create_int32(env, zes_last_gunzip_members(), &v);
  return v;
}

// trim(): the addon's pooled blocks, the calling environment's scratch block and the library's pooled device scratch go
// back to the driver (zes_trim); the next call allocates again
napi_value Trim(napi_env env, napi_callback_info) {
  g_big.clear();
  if (EnvState* es = tracks_of(env)) es->scratch.clear();
  return undefined_unless(env, zes_trim());
}

// ---- Promise-returning forms: the blocking C-ABI call runs on a libuv worker thread ----
struct Job {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  napi_ref input_ref = nullptr;  // keeps the caller's value alive (and its memory in place) while the worker reads it
};
// The promise of a job, and the job on its way to a worker thread; takes the job over.  The reference on `keep` keeps the
// input (and its memory) alive while the worker reads it.  The caller must not transfer or detach its ArrayBuffer
// before the promise settles (documented in zlib.ts): N-API v3 has no way to pin a backing store against a transfer.
template <class J>
napi_value start_job(napi_env env, J* j, napi_value keep, const char* work_name, napi_async_execute_callback execute, napi_async_complete_callback complete) {
  napi_value promise, name;
  if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) {
    delete j;
    napi_throw_error(env, nullptr, "zes: could not create a promise");
    return nullptr;
  }
  bool ok = napi_create_reference(env, keep, 1, &j->input_ref) == napi_ok && napi_create_string_utf8(env, work_name, NAPI_AUTO_LENGTH, &name) == napi_ok &&
            napi_create_async_work(env, nullptr, name, execute, complete, j, &j->work) == napi_ok;
  if (ok && napi_queue_async_work(env, j->work) != napi_ok) {
    napi_delete_async_work(env, j->work);
    ok = false;
  }
  if (!ok) {  // nothing was queued: settle the promise here, free the job
    napi_reject_deferred(env, j->deferred, make_error(env, "zes: could not queue the work"));
    if (j->input_ref) napi_delete_reference(env, j->input_ref);
    delete j;
  }
  return promise;
}
// the end of a completion, on the JS thread again: the promise settles (no result: a plain Error with the status's
// message, as a rejection), the input is let go, the job ends
template <class J>
void finish_job(napi_env env, J* j, napi_value result, int rc) {
  if (result)
    napi_resolve_deferred(env, j->deferred, result);
  else
    napi_reject_deferred(env, j->deferred, make_error(env, zes_strerror(rc ? rc : ZES_E_ARG)));
  napi_delete_reference(env, j->input_ref);
  napi_delete_async_work(env, j->work);
  delete j;
}

struct AsyncJob : Job {
  Bytes in;
  bool inflate = false;
  uint32_t flags = 0;  // inflate: ZES_F_CHECK_ADLER when the caller asked for { verify: true }
  ExactMem out;
  uint64_t out_len = 0;
  int rc = 0;
  ~AsyncJob() { out.drop(); }  // (what no ArrayBuffer took over)
};

uint8_t* async_alloc(void* user, uint32_t index, uint64_t n) {  // zes_alloc_fn on the worker thread: pool or malloc, no N-API calls
  ExactMem& out = static_cast<AsyncJob*>(user)->out;
  if (!(index & ZES_ALLOC_EARLY)) return out.renew((size_t)n);
  out.drop();
  out.m = pooled((size_t)n);  // (an early request is only worth taking with a pooled block: see sync_alloc)
  return out.m.p;
}

void async_execute(napi_env, void* data) {  // worker thread: no N-API calls here
  AsyncJob* j = static_cast<AsyncJob*>(data);
  if (!j->inflate) {
    uint64_t cap = 0;
    zes_deflate_bound(j->in.n, &cap);
    const Filled f = fill(result_alloc(cap), [&](uint8_t* out, uint64_t* len) { return zes_deflate(j->in.p, j->in.n, out, cap, len); });
    j->out.m = f.m;
    j->out_len = f.len;
    j->rc = f.rc;
    return;
  }
  // one call: the library decodes, then asks for memory of the exact size (no state is kept in the library between calls)
  j->rc = zes_inflate_alloc(j->in.p, j->in.n, async_alloc, j, &j->out_len, ZES_F_ALLOC_BOUND | j->flags);
  g_big.top_up();
}

void async_complete(napi_env env, napi_status, void* data) {  // JS thread again
  AsyncJob* j = static_cast<AsyncJob*>(data);
  napi_value result = nullptr;
  if (j->rc == 0) {
    // the worker's memory becomes the result's ArrayBuffer (exact length, no copy on the JS thread)
    result = take_u8(env, j->out.m, (size_t)j->out_len);
    j->out.m = ResultMem();  // owned by the ArrayBuffer now (or given back by take_u8)
  }
  finish_job(env, j, result, j->rc);
}

napi_value start_async(napi_env env, napi_callback_info info, bool inflate) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, inflate ? "inflateAsync(input)" : "deflateAsync(input)", "input");
  if (!in.ok) return nullptr;
  AsyncJob* j = new AsyncJob();
  j->in = in;
  j->inflate = inflate;
  if (inflate) j->flags = verify_flag(env, a, 1);
  return start_job(env, j, a.argv[0], inflate ? "zes_inflate" : "zes_deflate", async_execute, async_complete);
}
napi_value DeflateAsync(napi_env env, napi_callback_info info) { return start_async(env, info, false); }
napi_value InflateAsync(napi_env env, napi_callback_info info) { return start_async(env, info, true); }

// ---- batch forms (deflateBatch / inflateBatch): an array of independent buffers in one call, so that
// small buffers share the launches and fill the chip together (zes_deflate_batch / zes_inflate_batch_alloc) ----
struct BatchJob : Job {  // (deferred null: a synchronous call)
  bool inflate = false;
  uint32_t flags = 0;  // inflate: ZES_F_CHECK_ADLER when the caller asked for { verify: true }
  uint32_t count;
  // one element more than count: an empty batch still hands the library pointers (zes_deflate_batch answers ZES_E_ARG to
  // a null one) and returns []
  std::vector<const uint8_t*> in;
  std::vector<uint64_t> in_len;
  std::vector<uint8_t*> out;
  std::vector<size_t> out_pool;  // capacity of the pooled block behind out[i], or 0: malloc'd
  std::vector<uint64_t> out_cap, out_len;
  std::vector<int32_t> status;
  int rc = 0;
  explicit BatchJob(uint32_t n)
      : count(n), in((size_t)n + 1), in_len((size_t)n + 1), out((size_t)n + 1), out_pool((size_t)n + 1), out_cap((size_t)n + 1), out_len((size_t)n + 1), status((size_t)n + 1) {}
  uint8_t* put(uint32_t i, ResultMem m) {
    out[i] = m.p;
    out_pool[i] = m.cap;
    return m.p;
  }
  ResultMem claim(uint32_t i) {  // out[i] is the caller's from here on
    ResultMem m;
    m.p = out[i];
    m.cap = out_pool[i];
    put(i, ResultMem());
    return m;
  }
  ~BatchJob() {  // (the blocks no ArrayBuffer took over)
    for (uint32_t i = 0; i < count; i++) result_free(claim(i));
  }
};

uint8_t* batch_alloc(void* user, uint32_t i, uint64_t n) {  // any thread: pool or malloc, wrapped into an ArrayBuffer later
  return static_cast<BatchJob*>(user)->put(i, result_alloc((size_t)n, false));  // (inside the library's call, possibly on one of its threads)
}

void batch_execute(napi_env, void* data) {
  BatchJob* j = static_cast<BatchJob*>(data);
  if (j->inflate) {
    j->rc = zes_inflate_batch_alloc(j->in.data(), j->in_len.data(), batch_alloc, j, j->out_len.data(), j->status.data(), j->count, ZES_F_DEFAULT | j->flags);
    return;
  }
  for (uint32_t i = 0; i < j->count; i++) {
    zes_deflate_bound(j->in_len[i], &j->out_cap[i]);
    if (!j->put(i, result_alloc((size_t)j->out_cap[i]))) {
      j->rc = ZES_E_ARG;
      return;
    }
  }
  j->rc = zes_deflate_batch(j->in.data(), j->in_len.data(), j->out.data(), j->out_cap.data(), j->out_len.data(), j->status.data(), j->count);
}

// results: an array with, per buffer, a fresh Uint8Array or an Error carrying the reference's message
// (a batch never throws for one bad buffer: the caller sees which ones failed)
napi_value batch_results(napi_env env, BatchJob* j) {
  napi_value arr;
  if (napi_create_array_with_length(env, j->count, &arr) != napi_ok) return nullptr;
  for (uint32_t i = 0; i < j->count; i++) {
    napi_value v = j->status[i] == 0 ? take_u8(env, j->claim(i), (size_t)j->out_len[i]) : make_error(env, zes_strerror(j->status[i]));
    if (!v) return nullptr;
    napi_set_element(env, arr, i, v);
  }
  return arr;
}

void batch_complete(napi_env env, napi_status, void* data) {
  BatchJob* j = static_cast<BatchJob*>(data);
  finish_job(env, j, j->rc == 0 ? batch_results(env, j) : nullptr, j->rc);
}

napi_value start_batch(napi_env env, napi_callback_info info, bool inflate, bool async) {
  const Args a = get_args(env, info);
  bool is_arr = false;
  uint32_t count = 0;
  if (a.argc < 1 || napi_is_array(env, a.argv[0], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, a.argv[0], &count) != napi_ok)
    return throw_type(env, "batch(inputs): inputs must be an array of Uint8Array");
  std::unique_ptr<BatchJob> j(new BatchJob(count));
  j->inflate = inflate;
  if (inflate) j->flags = verify_flag(env, a, 1);
  for (uint32_t i = 0; i < count; i++) {
    napi_value e;
    size_t n = 0;
    if (napi_get_element(env, a.argv[0], i, &e) != napi_ok || !get_bytes(env, e, &j->in[i], &n))
      return throw_type(env, "batch(inputs): every element must be a Uint8Array");
    j->in_len[i] = n;
  }
  if (async)  // (the outer array keeps every element alive)
    return start_job(env, j.release(), a.argv[0], inflate ? "zes_inflate_batch" : "zes_deflate_batch", batch_execute, batch_complete);
  batch_execute(env, j.get());
  return j->rc == 0 ? batch_results(env, j.get()) : throw_status(env, j->rc);
}
napi_value DeflateBatch(napi_env env, napi_callback_info info) { return start_batch(env, info, false, false); }
napi_value InflateBatch(napi_env env, napi_callback_info info) { return start_batch(env, info, true, false); }
napi_value DeflateBatchAsync(napi_env env, napi_callback_info info) { return start_batch(env, info, false, true); }
napi_value InflateBatchAsync(napi_env env, napi_callback_info info) { return start_batch(env, info, true, true); }

// ---- ZIP archives (include/zes.h: zes_zip_index, zes_zip_read_alloc) ----
// a fresh Uint8Array of n bytes in memory of the engine's own (*mem: where to fill it)
napi_value new_u8(napi_env env, size_t n, void** mem) {
  napi_value ab, ta;
  if (napi_create_arraybuffer(env, n, mem, &ab) != napi_ok || napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta) != napi_ok) return nullptr;
  return ta;
}

// zipIndex(file): { raw, names } — the entries as zes_zip_entry records (what zipRead hands back to the library) and the
// names back to back; the façade makes the entry objects out of the two.  The host form: no device is touched.
napi_value ZipIndex(napi_env env, napi_callback_info info) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, "zipIndex(file)", "file");
  if (!in.ok) return nullptr;
  uint64_t entries = 0, names_len = 0;
  int rc = zes_zip_index(in.p, in.n, nullptr, 0, &entries, nullptr, 0, &names_len, ZES_F_DEFAULT);  // (the counts: ZES_E_NOSPACE on a valid archive)
  if (rc != ZES_E_NOSPACE) return throw_status(env, rc ? rc : ZES_E_ARG);
  void *raw = nullptr, *names = nullptr;
  napi_value res, vraw = new_u8(env, (size_t)entries * sizeof(zes_zip_entry), &raw), vnames = new_u8(env, (size_t)names_len, &names);
  if (!vraw || !vnames) return nullptr;
  std::vector<zes_zip_entry> ent((size_t)entries + 1);  // (an ArrayBuffer's memory need not be aligned for the records)
  uint8_t none = 0;
  rc = zes_zip_index(in.p, in.n, ent.data(), entries, &entries, names ? static_cast<uint8_t*>(names) : &none, names_len, &names_len, ZES_F_DEFAULT);
  if (rc) return throw_status(env, rc);
  if (entries) memcpy(raw, ent.data(), (size_t)entries * sizeof(zes_zip_entry));
  if (napi_create_object(env, &res) != napi_ok) return nullptr;
  napi_set_named_property(env, res, "raw", vraw);
  napi_set_named_property(env, res, "names", vnames);
  return res;
}

// zipRead(file, index, sel): the selected entries (all without sel) as one batch: per entry a fresh Uint8Array or the Error
// that says why not, as the batch forms answer
napi_value ZipRead(napi_env env, napi_callback_info info) {
  static const char SIG[] = "zipRead(file, index, sel)";
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, SIG, "file");
  if (!in.ok) return nullptr;
  napi_value vraw;
  napi_valuetype vt = napi_undefined;
  const uint8_t* raw = nullptr;
  size_t raw_n = 0;
  if (a.argc < 2 || napi_typeof(env, a.argv[1], &vt) != napi_ok || vt != napi_object || napi_get_named_property(env, a.argv[1], "raw", &vraw) != napi_ok ||
      !get_bytes(env, vraw, &raw, &raw_n) || raw_n % sizeof(zes_zip_entry))
    return throw_type(env, std::string(SIG) + ": index must be what zipIndex(file) returned");
  std::vector<zes_zip_entry> ent(raw_n / sizeof(zes_zip_entry) + 1);
  if (raw_n) memcpy(ent.data(), raw, raw_n);
  const uint64_t nent = raw_n / sizeof(zes_zip_entry);
  std::vector<uint32_t> sel;
  bool all = a.argc < 3 || napi_typeof(env, a.argv[2], &vt) != napi_ok || vt == napi_undefined || vt == napi_null;
  if (!all) {
    bool is_arr = false, is_ta = false;
    uint32_t n = 0;
    if (napi_is_array(env, a.argv[2], &is_arr) == napi_ok && is_arr && napi_get_array_length(env, a.argv[2], &n) == napi_ok) {
      sel.resize(n);
      for (uint32_t i = 0; i < n; i++) {
        napi_value e;
        uint64_t v = 0;
        if (napi_get_element(env, a.argv[2], i, &e) != napi_ok || !get_safe_uint(env, e, &v) || v > 0xFFFFFFFFull)
          return throw_type(env, std::string(SIG) + ": sel must be an array of entry numbers or a Uint32Array");
        sel[i] = (uint32_t)v;
      }
    } else if (napi_is_typedarray(env, a.argv[2], &is_ta) == napi_ok && is_ta) {
      napi_typedarray_type type;
      void* p = nullptr;
      size_t len = 0, off = 0;
      napi_value ab;
      if (napi_get_typedarray_info(env, a.argv[2], &type, &len, &p, &ab, &off) != napi_ok || type != napi_uint32_array || len > 0xFFFFFFFFull)
        return throw_type(env, std::string(SIG) + ": sel must be an array of entry numbers or a Uint32Array");
      sel.assign(static_cast<const uint32_t*>(p), static_cast<const uint32_t*>(p) + len);
    } else {
      return throw_type(env, std::string(SIG) + ": sel must be an array of entry numbers or a Uint32Array");
    }
  }
  if (all && nent > 0xFFFFFFFFull) return throw_status(env, ZES_E_ARG);
  BatchJob j(all ? (uint32_t)nent : (uint32_t)sel.size());
  j.rc = zes_zip_read_alloc(in.p, in.n, ent.data(), nent, all ? nullptr : sel.data(), j.count, batch_alloc, &j, j.out_len.data(), j.status.data(), ZES_F_DEFAULT);
  return j.rc == 0 ? batch_results(env, &j) : throw_status(env, j.rc);
}

// ---- PNG images (include/zes.h: zes_png_info_get, zes_png_decode_alloc, zes_pngpix_alloc) ----
// pngInfo(file): the file's zes_png_info record as 72 bytes; the façade makes the object.  The host form: no device is touched.
napi_value PngInfo(napi_env env, napi_callback_info info) {
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, "pngInfo(file)", "file");
  if (!in.ok) return nullptr;
  zes_png_info rec;
  const int rc = zes_png_info_get(in.p, in.n, &rec, ZES_F_DEFAULT);
  if (rc) return throw_status(env, rc);
  void* raw = nullptr;
  napi_value v = new_u8(env, sizeof rec, &raw);
  if (!v) return nullptr;
  memcpy(raw, &rec, sizeof rec);
  return v;
}

// pngDecodeBatch(files[, options]) and pngPixelsBatch(files[, options]): the files decoded as one batch: { results, info } — per file the scanlines
// (the pixels: width * height * 4 bytes of R, G, B, A) as a fresh Uint8Array or the Error that says why not, as the batch
// forms answer, and the files' zes_png_info records back to back.  The two differ in the entry point alone.  options,
// { interlaced?: boolean }: ZES_F_PNG_INTERLACED when interlaced is true (Adam7 files decode too); anything but an object or
// undefined in its place, an array included, is a TypeError
using PngBatchFn = int (*)(const uint8_t* const*, const uint64_t*, uint32_t, zes_alloc_fn, void*, uint64_t*, int32_t*, zes_png_info*, uint32_t);
napi_value png_batch(napi_env env, napi_callback_info info, const char* SIG, PngBatchFn fn) {
  const Args a = get_args(env, info);
  bool is_arr = false;
  uint32_t count = 0;
  if (a.argc < 1 || napi_is_array(env, a.argv[0], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, a.argv[0], &count) != napi_ok)
    return throw_type(env, std::string(SIG) + ": files must be an array of Uint8Array");
  BatchJob j(count);
  for (uint32_t i = 0; i < count; i++) {
    napi_value e;
    size_t n = 0;
    if (napi_get_element(env, a.argv[0], i, &e) != napi_ok || !get_bytes(env, e, &j.in[i], &n))
      return throw_type(env, std::string(SIG) + ": every element must be a Uint8Array");
    j.in_len[i] = n;
  }
  uint32_t flags = ZES_F_DEFAULT;
  napi_valuetype vt = napi_undefined;
  if (a.argc > 1 && (napi_typeof(env, a.argv[1], &vt) != napi_ok || vt != napi_undefined)) {
    napi_value v;
    bool on = false;
    bool opt_arr = false;
    if (vt != napi_object || napi_is_array(env, a.argv[1], &opt_arr) != napi_ok || opt_arr)
      return throw_type(env, std::string(SIG) + ": options must be an object { interlaced?: boolean }");
    if (napi_get_named_property(env, a.argv[1], "interlaced", &v) == napi_ok && napi_typeof(env, v, &vt) == napi_ok && vt == napi_boolean &&
        napi_get_value_bool(env, v, &on) == napi_ok && on)
      flags |= ZES_F_PNG_INTERLACED;
  }
  std::vector<zes_png_info> recs((size_t)count + 1);
  j.rc = fn(j.in.data(), j.in_len.data(), count, batch_alloc, &j, j.out_len.data(), j.status.data(), recs.data(), flags);
  if (j.rc) return throw_status(env, j.rc);
  void* raw = nullptr;
  napi_value res, vres = batch_results(env, &j), vinfo = new_u8(env, (size_t)count * sizeof(zes_png_info), &raw);
  if (!vres || !vinfo) return nullptr;
  if (count) memcpy(raw, recs.data(), (size_t)count * sizeof(zes_png_info));
  if (napi_create_object(env, &res) != napi_ok) return nullptr;
  napi_set_named_property(env, res, "results", vres);
  napi_set_named_property(env, res, "info", vinfo);
  return res;
}
napi_value PngDecodeBatch(napi_env env, napi_callback_info info) { return png_batch(env, info, "pngDecodeBatch(files)", zes_png_decode_alloc); }
napi_value PngPixelsBatch(napi_env env, napi_callback_info info) { return png_batch(env, info, "pngPixelsBatch(files)", zes_pngpix_alloc); }

// pngEncodeBatch(rows, records, aux): images written as PNG files in one batch (include/zes.h: zes_pngwrite) — rows[i] the
// scanlines of image i, records its zes_pngw_image record (16 bytes each, back to back; the façade makes them) and aux every
// image's PLTE then tRNS data.  Per image the file as a fresh Uint8Array or the Error that says why not.
napi_value PngEncodeBatch(napi_env env, napi_callback_info info) {
  static const char SIG[] = "pngEncodeBatch(rows, records, aux)";
  const Args a = get_args(env, info);
  bool is_arr = false;
  uint32_t count = 0;
  if (a.argc < 3 || napi_is_array(env, a.argv[0], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, a.argv[0], &count) != napi_ok)
    return throw_type(env, std::string(SIG) + ": rows must be an array of Uint8Array");
  const Bytes recs = need_bytes(env, a, 1, SIG, "records");
  if (!recs.ok) return nullptr;
  const Bytes aux = need_bytes(env, a, 2, SIG, "aux");
  if (!aux.ok) return nullptr;
  if (recs.n != (size_t)count * sizeof(zes_pngw_image)) return throw_type(env, std::string(SIG) + ": records must hold 16 bytes an image");
  BatchJob j(count);
  uint64_t naux = 0;
  std::vector<zes_pngw_image> img((size_t)count + 1);
  if (count) memcpy(img.data(), recs.p, recs.n);
  for (uint32_t i = 0; i < count; i++) {
    napi_value e;
    size_t n = 0;
    if (napi_get_element(env, a.argv[0], i, &e) != napi_ok || !get_bytes(env, e, &j.in[i], &n))
      return throw_type(env, std::string(SIG) + ": every element of rows must be a Uint8Array");
    j.in_len[i] = n;
    naux += (uint64_t)img[i].plte_len + img[i].trns_len;
  }
  if (naux != aux.n) return throw_type(env, std::string(SIG) + ": aux must hold every image's PLTE and tRNS data");
  j.rc = zes_pngwrite(j.in.data(), j.in_len.data(), img.data(), aux.p, count, batch_alloc, &j, j.out_len.data(), j.status.data(), ZES_F_DEFAULT);
  return j.rc == 0 ? batch_results(env, &j) : throw_status(env, j.rc);
}

// ---- TIFF images (include/zes.h: zes_tiff_index, zes_tiff_read_alloc) ----
// the optional directory number at argument k: undefined counts as 0
bool tiff_dir(napi_env env, const Args& a, size_t k, uint32_t* dir) {
  *dir = 0;
  napi_valuetype vt = napi_undefined;
  if (a.argc <= k || napi_typeof(env, a.argv[k], &vt) != napi_ok || vt == napi_undefined) return true;
  uint64_t d = 0;
  if (!get_safe_uint(env, a.argv[k], &d) || d > 0xFFFFFFFFull) return false;
  *dir = (uint32_t)d;
  return true;
}
// a zes_tiff_image record and the chain's length behind it as 52 bytes; the façade makes the object
napi_value tiff_record(napi_env env, const zes_tiff_image& rec, uint32_t dirs) {
  void* raw = nullptr;
  napi_value v = new_u8(env, sizeof rec + 4, &raw);
  if (!v) return nullptr;
  memcpy(raw, &rec, sizeof rec);
  memcpy(static_cast<uint8_t*>(raw) + sizeof rec, &dirs, 4);
  return v;
}
// tiffInfo(file[, dir]): what the file rule says about directory dir.  The host form: no device is touched.
napi_value TiffInfo(napi_env env, napi_callback_info info) {
  static const char SIG[] = "tiffInfo(file[, dir])";
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, SIG, "file");
  if (!in.ok) return nullptr;
  uint32_t dir = 0, dirs = 0;
  if (!tiff_dir(env, a, 1, &dir)) return throw_type(env, std::string(SIG) + ": dir must be a non-negative integer below 2^32");
  zes_tiff_image rec;
  uint64_t nseg = 0;
  const int rc = zes_tiff_index(in.p, in.n, dir, &rec, nullptr, nullptr, 0, &nseg, &dirs, ZES_F_DEFAULT);  // (the sizing call: ZES_E_NOSPACE on a valid file)
  if (rc != ZES_E_NOSPACE) return throw_status(env, rc ? rc : ZES_E_ARG);
  return tiff_record(env, rec, dirs);
}
// tiffRead(file, dir, rect): a rectangle (a Uint32Array of x, y, w, h; undefined: the whole image) of directory dir decoded
// by zes_tiff_read_alloc, through the batch forms' marshalling as a batch of one: { results: [pixels], info }
napi_value TiffRead(napi_env env, napi_callback_info info) {
  static const char SIG[] = "tiffRead(file, dir, rect)";
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, SIG, "file");
  if (!in.ok) return nullptr;
  uint32_t dir = 0;
  if (!tiff_dir(env, a, 1, &dir)) return throw_type(env, std::string(SIG) + ": dir must be a non-negative integer below 2^32");
  zes_tiff_rect rect;
  bool have_rect = false;
  napi_valuetype vt = napi_undefined;
  if (a.argc > 2 && napi_typeof(env, a.argv[2], &vt) == napi_ok && vt != napi_undefined) {
    napi_typedarray_type type;
    void* p = nullptr;
    size_t len = 0, off = 0;
    napi_value ab;
    bool is_ta = false;
    if (napi_is_typedarray(env, a.argv[2], &is_ta) != napi_ok || !is_ta || napi_get_typedarray_info(env, a.argv[2], &type, &len, &p, &ab, &off) != napi_ok ||
        type != napi_uint32_array || len != 4)
      return throw_type(env, std::string(SIG) + ": rect must be a Uint32Array of x, y, w, h");
    memcpy(&rect, p, sizeof rect);
    have_rect = true;
  }
  BatchJob j(1);
  zes_tiff_image rec;
  j.rc = zes_tiff_read_alloc(in.p, in.n, dir, have_rect ? &rect : nullptr, batch_alloc, &j, j.out_len.data(), &rec, ZES_F_DEFAULT);
  if (j.rc) return throw_status(env, j.rc);
  napi_value res, vres = batch_results(env, &j), vinfo = tiff_record(env, rec, 0);
  if (!vres || !vinfo) return nullptr;
  if (napi_create_object(env, &res) != napi_ok) return nullptr;
  napi_set_named_property(env, res, "results", vres);
  napi_set_named_property(env, res, "info", vinfo);
  return res;
}

// tiffWrite(pixels, record): one image written as a TIFF file by zes_tiffwrite, through the batch forms' marshalling as a batch
// of one.  record: the 48 bytes of a zes_tiff_image (the façade packs its info object)
napi_value TiffWrite(napi_env env, napi_callback_info info) {
  static const char SIG[] = "tiffWrite(pixels, record)";
  const Args a = get_args(env, info);
  const Bytes in = need_bytes(env, a, 0, SIG, "pixels");
  if (!in.ok) return nullptr;
  const Bytes r = need_bytes(env, a, 1, SIG, "record");
  if (!r.ok) return nullptr;
  if (r.n != sizeof(zes_tiff_image)) return throw_type(env, std::string(SIG) + ": record must hold the 48 bytes of a zes_tiff_image");
  zes_tiff_image rec;
  memcpy(&rec, r.p, sizeof rec);
  BatchJob j(1);
  j.rc = zes_tiffwrite(in.p, in.n, &rec, batch_alloc, &j, j.out_len.data(), ZES_F_DEFAULT);
  return j.rc == 0 ? batch_results(env, &j) : throw_status(env, j.rc);
}

// gzipBatch(inputs) and gunzipBatch(files): independent buffers written as one gzip file each, and independent gzip files
// decoded, as one batch (include/zes.h: zes_gzip_batch, zes_gunzip_batch_alloc): per item a fresh Uint8Array or the Error that
// says why not, as the batch forms answer.  The two differ in the entry point alone.
using GzBatchFn = int (*)(const uint8_t* const*, const uint64_t*, uint32_t, zes_alloc_fn, void*, uint64_t*, int32_t*, uint32_t);
napi_value gz_batch(napi_env env, napi_callback_info info, const char* SIG, GzBatchFn fn) {
  const Args a = get_args(env, info);
  bool is_arr = false;
  uint32_t count = 0;
  if (a.argc < 1 || napi_is_array(env, a.argv[0], &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, a.argv[0], &count) != napi_ok)
    return throw_type(env, std::string(SIG) + ": the argument must be an array of Uint8Array");
  BatchJob j(count);
  for (uint32_t i = 0; i < count; i++) {
    napi_value e;
    size_t n = 0;
    if (napi_get_element(env, a.argv[0], i, &e) != napi_ok || !get_bytes(env, e, &j.in[i], &n))
      return throw_type(env, std::string(SIG) + ": every element must be a Uint8Array");
    j.in_len[i] = n;
  }
  j.rc = fn(j.in.data(), j.in_len.data(), count, batch_alloc, &j, j.out_len.data(), j.status.data(), ZES_F_DEFAULT);
  return j.rc == 0 ? batch_results(env, &j) : throw_status(env, j.rc);
}
napi_value GzipBatch(napi_env env, napi_callback_info info) { return gz_batch(env, info, "gzipBatch(inputs)", zes_gzip_batch); }
napi_value GunzipBatch(napi_env env, napi_callback_info info) { return gz_batch(env, info, "gunzipBatch(files)", zes_gunzip_batch_alloc); }

// zip(names, datas): a ZIP archive of datas[i] under names[i], two arrays of Uint8Array of one length (the façade takes the
// file objects apart and encodes string names): one call, the bounded result (include/zes.h: zes_zipwrite)
napi_value Zip(napi_env env, napi_callback_info info) {
  static const char SIG[] = "zip(files)";
  const Args a = get_args(env, info);
  bool arr_n = false, arr_d = false;
  uint32_t count = 0, count_d = 0;
  if (a.argc < 2 || napi_is_array(env, a.argv[0], &arr_n) != napi_ok || !arr_n || napi_is_array(env, a.argv[1], &arr_d) != napi_ok || !arr_d ||
      napi_get_array_length(env, a.argv[0], &count) != napi_ok || napi_get_array_length(env, a.argv[1], &count_d) != napi_ok || count != count_d)
    return throw_type(env, std::string(SIG) + ": files must be an array of { name, data }");
  std::vector<const uint8_t*> in((size_t)count + 1);
  std::vector<uint64_t> in_len((size_t)count + 1);
  std::vector<uint16_t> name_len((size_t)count + 1);
  std::vector<uint8_t> names(1);
  for (uint32_t i = 0; i < count; i++) {
    napi_value vn, vd;
    const uint8_t* np = nullptr;
    size_t nn = 0, dn = 0;
    if (napi_get_element(env, a.argv[0], i, &vn) != napi_ok || !get_bytes(env, vn, &np, &nn) || nn > 65535)
      return throw_type(env, std::string(SIG) + ": every name must be a string or a Uint8Array of at most 65535 bytes");
    if (napi_get_element(env, a.argv[1], i, &vd) != napi_ok || !get_bytes(env, vd, &in[i], &dn))
      return throw_type(env, std::string(SIG) + ": every data must be a Uint8Array");
    in_len[i] = dn;
    name_len[i] = (uint16_t)nn;
    names.insert(names.end(), np, np + nn);
  }
  uint64_t cap = 0;
  if (zes_zipwrite_bound(in_len.data(), name_len.data(), count, &cap)) return throw_status(env, ZES_E_ARG);
  return bounded(env, result_alloc(cap), [&](uint8_t* out, uint64_t* len) {
    return zes_zipwrite(in.data(), in_len.data(), names.data() + 1, name_len.data(), count, out, cap, len, nullptr, ZES_F_DEFAULT);
  });
}

// allocPinned(n): a Uint8Array in page-locked memory (zes_host_alloc) — buffers from here cross PCIe without the
// library's staging copy; released when the array is collected.  The release runs on the JS thread and takes
// the library's lock for a moment (no stream is waited for: hipHostFree itself waits for work that uses the block), so
// it can stall behind a call that is holding the lock; zes_host_free also works after zes_shutdown.
napi_value AllocPinned(napi_env env, napi_callback_info info) {
  uint64_t n = 0;
  if (!get_safe_uint(env, get_args(env, info).argv[0], &n) || n > 1000000000000ull) return throw_type(env, "allocPinned(n): n must be a non-negative integer");
  void* p = nullptr;
  const int rc = zes_host_alloc(n, &p);
  if (rc) return throw_status(env, rc);
  return adopt(env, static_cast<uint8_t*>(p), (size_t)n, 0, true);  // (released by a later call's sweep once the array is collected)
}

// every entry point first looks which arrays the collector has taken since the last call
template <napi_callback F>
napi_value swept(napi_env env, napi_callback_info info) {
  sweep(env);
  return F(env, info);
}

napi_value ModuleInit(napi_env env, napi_value exports) {
  const struct {
    const char* name;
    napi_callback fn;
  } entries[] = {
      {"deflate", swept<Deflate>},
      {"inflate", swept<Inflate>},
      {"deflateRaw", swept<DeflateRaw>},
      {"inflateRaw", swept<InflateRaw>},
      {"deflateAsync", swept<DeflateAsync>},
      {"inflateAsync", swept<InflateAsync>},
      {"deflateBatch", swept<DeflateBatch>},
      {"inflateBatch", swept<InflateBatch>},
      {"deflateBatchAsync", swept<DeflateBatchAsync>},
      {"inflateBatchAsync", swept<InflateBatchAsync>},
      {"allocPinned", swept<AllocPinned>},
      {"adler32", swept<Adler32>},
      {"gzip", swept<Gzip>},
      {"gunzip", swept<Gunzip>},
      {"gzipBatch", swept<GzipBatch>},
      {"gunzipBatch", swept<GunzipBatch>},
      {"bgzip", swept<Bgzip>},
      {"bgzipIndex", swept<BgzipIndex>},
      {"bgzfIndex", swept<BgzfIndex>},
      {"bgzfRead", swept<BgzfRead>},
      {"zipIndex", swept<ZipIndex>},
      {"zipRead", swept<ZipRead>},
      {"zip", swept<Zip>},
      {"pngInfo", swept<PngInfo>},
      {"pngDecodeBatch", swept<PngDecodeBatch>},
      {"pngPixelsBatch", swept<PngPixelsBatch>},
      {"pngEncodeBatch", swept<PngEncodeBatch>},
      {"tiffInfo", swept<TiffInfo>},
      {"tiffRead", swept<TiffRead>},
      {"tiffWrite", swept<TiffWrite>},
      {"lastGunzipMembers", swept<LastGunzipMembers>},
      {"init", swept<Init>},
      {"initDevices", swept<InitDevices>},
      {"trim", swept<Trim>},
  };
  std::vector<napi_property_descriptor> props;
  for (const auto& e : entries) props.push_back({e.name, nullptr, e.fn, nullptr, nullptr, nullptr, napi_default, nullptr});
  napi_define_properties(env, exports, props.size(), props.data());
  if (getenv("ZES_NAPI_SEGV_TRACE")) {  // development: where a SIGSEGV comes from
    signal(SIGSEGV, [](int) {
      void* bt[64];
      const int n = backtrace(bt, 64);
      backtrace_symbols_fd(bt, n, 2);
      _exit(139);
    });
  }
  g_envs.fetch_add(1);
  g_exiting.store(false);
  {
    EnvState* es = new EnvState;
    es->env = env;
    std::lock_guard<std::mutex> lk(g_tracks_mu);
    g_tracks.push_back(es);
  }
  napi_add_env_cleanup_hook(env, env_cleanup, env);
  static bool once = false;
  if (!once) {
    once = true;
    atexit(mark_exiting_atexit);
  }
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, ModuleInit)
