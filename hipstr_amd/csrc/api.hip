// api.hip — the C-ABI of include/hipstr_hmm.h on top of the HIP kernels.
//
// Host responsibilities only: prepare (prep.cpp), move bytes, launch, time with HIP events on
// the launch stream, and re-impose the reference's "leave untouched what was not realigned"
// output contract.  There is no CPU compute path here: without a gfx950 device every entry
// point fails and hipstr_last_error() says so.
#include <hip/hip_runtime.h>
#include <unistd.h>
#include <sched.h>
#include <atomic>

#include <cfloat>
#include <chrono>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "layout.h"
#include "post_layout.h"
#include "readmat_layout.h"
#include "census_layout.h"
#include "prep.h"
#include "api_internal.h"
#include "float_lse.h"

extern "C" __global__ void hs_str_kernel(const hs_dev_t* dp, int active_begin, int only_long);
extern "C" __global__ void hs_str_kernel_generic(const hs_dev_t* dp, int active_begin, int pw_grouped);
extern "C" __global__ void hs_combine_kernel(const hs_dev_t* dp, int active_begin);
extern "C" int hs_combine_waves();
extern "C" __global__ void hs_posterior_kernel(const hs_post_dev_t* dp);
extern "C" __global__ void hs_posterior_accumulate_kernel(const hs_post_dev_t* dp);
extern "C" __global__ void hs_posterior_finish_kernel(const hs_post_dev_t* dp);
extern "C" __global__ void hs_genotype_kernel(const hs_gt_dev_t* dp);
extern "C" __global__ void hs_gt_permute_kernel(const hs_gt_perm_dev_t* dp);
extern "C" __global__ void hs_gt_gather_kernel(const hs_gt_perm_dev_t* dp);
extern "C" __global__ void hs_cr_math_kernel(int which, const double* x, double* y, int64_t n);
extern "C" __global__ void hs_float_fn_kernel(int which, uint32_t bits_lo, int64_t count, uint32_t* out);
extern "C" __global__ void hs_fast_lse2_kernel(const double* a, const double* b, double* out, int64_t n, double thr);
extern "C" __global__ void hs_fast_lse_vec_kernel(const double* v, const int64_t* row_off, double* out, int64_t n_rows, double thr);
extern "C" __global__ void hs_assign_kernel(const hs_assign_dev_t* dp);
extern "C" __global__ void hs_assign_kernel_wg(const hs_assign_dev_t* dp);
extern "C" __global__ void hs_assign_scan_kernel(const hs_assign_dev_t* dp);
extern "C" __global__ void hs_assign_requests_kernel(const hs_assign_dev_t* dp);
extern "C" __global__ void hs_census_wave_kernel(const hs_census_dev_t* dp);
extern "C" __global__ void hs_census_lds_kernel(const hs_census_dev_t* dp);
extern "C" __global__ void hs_census_global_kernel(const hs_census_dev_t* dp);
extern "C" __global__ void hs_census_scan_kernel(const hs_census_dev_t* dp);
extern "C" __global__ void hs_census_emit_kernel(const hs_census_dev_t* dp);
extern "C" __global__ void hs_census_check_kernel(const hs_census_dev_t* dp);
extern "C" __global__ void hs_census_gather_kernel(const hs_census_dev_t* dp);
extern "C" __global__ void hs_trace_stats_kernel(const hs_tstat_dev_t* dp);
extern "C" __global__ void hs_rm_scatter_kernel(const hs_rm_scatter_t d);
extern "C" __global__ void hs_rm_remap_kernel(const hs_rm_remap_t d);
extern "C" __global__ void hs_rm_fill_kernel(double* p, int64_t n, double v);
extern "C" size_t hs_str_lds_bytes(int lds_len, int max_B);
extern "C" __global__ void hs_str_group_kernel(const hs_dev_t* dp, int item_begin, int short_only);
extern "C" __global__ void hs_str_group_kernel_pw(const hs_dev_t* dp, int item_begin);
extern "C" __global__ void hs_str_group_kernel_rp(const hs_dev_t* dp, int item_begin);
extern "C" __global__ void hs_str_group_kernel_p(const hs_dev_t* dp, int item_begin);
extern "C" __global__ void hs_nd_kernel(const hs_dev_t* dp, int active_begin);
extern "C" __global__ void hs_expand_stropts_kernel(const hs_dev_t* dp);
extern "C" __global__ void hs_expand_recs_kernel(const hs_dev_t* dp);
extern "C" size_t hs_str_group_lds_bytes(int max_B, int nd_cap, int with_ilog);
extern "C" size_t hs_str_group_p_lds_bytes();
extern "C" void hs_launch_lead2(unsigned n_active, unsigned n_wavefronts, hipStream_t st, const hs_dev_t* dp, int active_begin, int item_begin, int item_end, int chunk, int max_cols, int n_clear);
extern "C" void hs_launch_trail(unsigned n_wavefronts, hipStream_t st, const hs_dev_t* dp, int item_begin, int item_end, int chunk, int max_cols, int max_rows);
extern "C" int hs_flank_route(int trail, int n_items, int max_cols, int max_rows);
extern "C" void hs_flank_shape(int trail, int route, int* R, int* W);
extern "C" void hs_flank_limits(int32_t out[5]);

namespace {

thread_local std::string g_err;
int fail(const std::string& m){ g_err = m; return 1; }

#define HS_HIP_NULL(call) do { hipError_t e_ = (call); if (e_ != hipSuccess){ \
  g_err = std::string(#call) + ": " + hipGetErrorString(e_); return NULL; } } while (0)

// Free lists of device / pinned blocks (see api_internal.h).  Sizes are rounded up to 256 B below 1 MiB and to 1/16 of the
// next power of two above, so that batches of similar size hit the same classes.
std::atomic<int64_t> g_driver_allocs(0);
// Blocks are carved from large chunks taken from the driver (256 MiB at first, doubling up to 16 GiB of device / 2 GiB of pinned memory)
// and never go back to it one by one: a hipMalloc / hipHostMalloc next to running kernels stalls for 0.1-0.3 s (seen in the middle of a
// stream: profiles/r04_notes.md), a hipFree synchronises the device.  A freed block goes to a free list by size; a request takes the
// smallest free block that holds it if that is at most twice as large, else a fresh piece of the current chunk.  No coalescing: the
// requests of a stream repeat, so the free list saturates after a few batches and the driver is not called again.  `cap` bounds the IDLE
// bytes (free blocks): a put() that leaves more gives the chunks nobody uses back to the driver; when the driver refuses a new chunk,
// get() falls back to any free block that is large enough, then trims idle chunks and tries once more.
struct BlockCache {
  bool pinned = false;
  std::mutex m;
  std::multimap<size_t, void*> free_;
  std::unordered_map<void*, size_t> size_;
  struct Chunk { char* base; size_t size, used; int live = 0; bool small = false; };       // live: blocks of the chunk that are out
  // Requests of up to 1 MiB are carved from chunks of their own (32 MiB each): the handful of small, fixed-size blocks every batch takes
  // would otherwise be re-used out of every old chunk and keep all of them from ever being trimmed.
  static constexpr size_t SMALL_MAX = (size_t)1 << 20, SMALL_CHUNK = (size_t)32 << 20;
  std::vector<Chunk> chunks;
  size_t next_chunk = (size_t)256 << 20;
  size_t cached = 0, cap = 0, in_use = 0;
  int64_t n_fallback = 0, n_trim_retry = 0;       // requests served by a free block beyond the 2x window / by a chunk taken after trimming (driver refusals survived)
  static size_t round_up(size_t n){
    if (n < 256) return 256;
    if (n <= ((size_t)1 << 20)) return (n + 255) & ~(size_t)255;
    size_t p2 = (size_t)1 << 20; while (p2 < n) p2 <<= 1;
    const size_t step = n > ((size_t)64 << 20) ? p2 >> 3 : p2 >> 4;
    return (n + step - 1) / step * step;
  }
  void* driver_alloc(size_t bytes){
    void* p = NULL;
    g_driver_allocs++;
    if (getenv("HIPSTR_TIMING")) fprintf(stderr, "block cache: %s chunk of %zu bytes from the driver\n", pinned ? "pinned" : "device", bytes);
    // tests: a driver that runs out at HIPSTR_DEBUG_DRIVER_LIMIT_MIB of device chunks (the recovery paths of get() without filling 288 GB)
    static const size_t dbg_limit = getenv("HIPSTR_DEBUG_DRIVER_LIMIT_MIB") ? (size_t)atol(getenv("HIPSTR_DEBUG_DRIVER_LIMIT_MIB")) << 20 : 0;
    if (dbg_limit && !pinned){
      size_t held = 0; for (const Chunk& c : chunks) held += c.size;
      if (held + bytes > dbg_limit){ g_err = "hipMalloc: out of memory (HIPSTR_DEBUG_DRIVER_LIMIT_MIB)"; return NULL; }
    }
    const hipError_t e = pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess){ g_err = std::string(pinned ? "hipHostMalloc: " : "hipMalloc: ") + hipGetErrorString(e); return NULL; }
    return p;
  }
  // (lock held) a free block of at least `want` bytes, the smallest one; `limit`: largest size accepted (0 = any)
  void* take_free(size_t want, size_t limit){
    auto it = free_.lower_bound(want);
    if (it == free_.end() || (limit && it->first > limit)) return NULL;
    void* p = it->second; cached -= it->first; free_.erase(it); in_use++;
    if (Chunk* c = chunk_of(p)) c->live++;
    return p;
  }
  void* get(size_t bytes){
    size_t want = round_up(bytes);
    std::unique_lock<std::mutex> g(m);
    if (void* p = take_free(want, 2*want)) return p;
    const size_t exact = want;
    if (want > ((size_t)16 << 20)) want = round_up(want + want/8);        // a new large block comes with headroom for its successors
    const bool small = exact <= SMALL_MAX;
    int ci = -1;                                         // the newest chunk of this class with room
    for (int i = (int)chunks.size() - 1; i >= 0; i--) if (chunks[i].small == small){ if (chunks[i].used + want <= chunks[i].size) ci = i; break; }
    if (ci < 0){
      const size_t max_chunk = pinned ? (size_t)2 << 30 : (size_t)16 << 30;
      size_t sz = small ? SMALL_CHUNK : std::max(next_chunk, want);
      if (!small) next_chunk = std::min(max_chunk, next_chunk*2);
      char* base = (char*)driver_alloc(sz);
      if (!base && sz > want) base = (char*)driver_alloc(sz = want);       // the device is nearly full: just what is needed
      if (!base){
        // the driver has no more: a larger free block, whatever its size, before giving up ...
        if (void* p = take_free(exact, 0)){ g_err.clear(); n_fallback++; return p; }
        // ... then the chunks without a block in use go back to the driver and the request is tried once more
        g.unlock();
        const size_t freed = trim();
        g.lock();
        if (void* p = take_free(exact, 0)){ g_err.clear(); n_fallback++; return p; }    // (another thread may have returned one meanwhile)
        if (freed){ g_err.clear(); base = (char*)driver_alloc(sz = exact); if (base) n_trim_retry++; }
        if (!base) return NULL;                                            // (the driver's message is in g_err)
        want = exact;
      }
      Chunk nc{base, sz, 0, 0}; nc.small = small;
      chunks.push_back(nc);
      ci = (int)chunks.size() - 1;
    }
    Chunk& c = chunks[ci];
    void* p = c.base + c.used;
    c.used += (want + 255) & ~(size_t)255;
    size_[p] = want;
    in_use++; c.live++;
    return p;
  }
  Chunk* chunk_of(const void* p){ for (Chunk& c : chunks) if ((const char*)p >= c.base && (const char*)p < c.base + c.size) return &c; return NULL; }
  void put(void* p){
    if (!p) return;
    std::unique_lock<std::mutex> g(m);
    auto it = size_.find(p);
    if (it == size_.end()) return;
    bool over;
    {
      free_.insert(std::make_pair(it->second, p)); cached += it->second;
      if (in_use > 0) in_use--;
      if (Chunk* c = chunk_of(p)) if (c->live > 0) c->live--;
      over = cap && cached > cap;
      if (over){                                   // (nothing to give back while every chunk has a block out: no second pass over the lists)
        over = false;
        for (const Chunk& c : chunks) if (c.live == 0){ over = true; break; }
      }
    }
    // more idle bytes than the cap allows (HIPSTR_DEV_CACHE_GIB / HIPSTR_PIN_CACHE_GIB): chunks nobody uses go back to the driver — down to
    // a low-water mark of 0.8 x cap, not all of them: a stream that sits near the cap would otherwise alternate a hipFree here (it
    // synchronises the device) with a hipMalloc at its next get(), the stall the cache exists to avoid
    if (over){ g.unlock(); trim(cap - cap/5); }
  }
  // chunks none of whose blocks is out go back to the driver (hipstr_hmm_trim: after a stream of large batches a process may sit on tens
  // of gigabytes it no longer needs — another process on the device, a child of this one, then fails its kernel launches with "out of
  // memory"); returns the bytes released
  // keep_idle: stop once the idle bytes are down to this (0: every chunk without a block out, hipstr_hmm_trim's meaning)
  size_t trim(size_t keep_idle = 0){
    std::vector<Chunk> gone; size_t bytes = 0;
    {
      std::lock_guard<std::mutex> g(m);
      for (size_t i = 0; i < chunks.size(); ){
        if (keep_idle && cached <= keep_idle) break;
        if (chunks[i].live != 0){ i++; continue; }
        const Chunk c = chunks[i];
        for (auto it = free_.begin(); it != free_.end(); ){
          if ((char*)it->second >= c.base && (char*)it->second < c.base + c.size){ cached -= it->first; size_.erase(it->second); it = free_.erase(it); } else ++it;
        }
        gone.push_back(c); bytes += c.size;
        chunks.erase(chunks.begin() + (long)i);
      }
      if (chunks.empty()) next_chunk = (size_t)256 << 20;
    }
    for (Chunk& c : gone){ if (pinned) hipHostFree(c.base); else hipFree(c.base); }
    return bytes;
  }
  // everything back to the driver — only when no block is out (hipstr_hmm_shutdown)
  void release(){
    std::vector<Chunk> v;
    { std::lock_guard<std::mutex> g(m); if (in_use > 0) return; v.swap(chunks); free_.clear(); size_.clear(); cached = 0; next_chunk = (size_t)256 << 20; }
    for (Chunk& c : v){ if (pinned) hipHostFree(c.base); else hipFree(c.base); }
  }
};

}  // namespace

namespace hipstr {
struct Ctx {
  int device = -1;
  double *int_log = NULL, *qc = NULL, *qe = NULL, *m2m = NULL, *m2i = NULL;
  double* rec_table = NULL; std::mutex rec_m;      // record.hip's gamma table, made on its first call (ctx_record_table)
  hipStream_t stream = NULL;
  BlockCache dev_cache, pin_cache;
  // events are pooled like the blocks: a device batch needs five (hipEventCreate / Destroy cost ~10 us each: a tenth of a one-locus call)
  std::mutex ev_m;
  std::vector<hipEvent_t> ev_timing, ev_plain;
  hipEvent_t get_event(bool timing){
    { std::lock_guard<std::mutex> g(ev_m);
      std::vector<hipEvent_t>& v = timing ? ev_timing : ev_plain;
      if (!v.empty()){ hipEvent_t e = v.back(); v.pop_back(); return e; } }
    hipEvent_t e = NULL;
    if ((timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming)) != hipSuccess) return NULL;
    return e;
  }
  void put_event(hipEvent_t e, bool timing){ if (!e) return; std::lock_guard<std::mutex> g(ev_m); (timing ? ev_timing : ev_plain).push_back(e); }
};
}  // namespace hipstr

namespace {
using hipstr::Ctx;
std::mutex g_ctx_mutex;
std::map<int, Ctx*> g_ctxs;                 // by device ordinal; contexts live until hipstr_hmm_shutdown
thread_local Ctx* t_ctx = NULL;             // what hipstr_hmm_init selected on this thread

int upload_table(const std::vector<double>& v, double** out){
  *out = NULL;
  HS_HIP(hipMalloc((void**)out, v.size()*sizeof(double)));
  HS_HIP(hipMemcpy(*out, v.data(), v.size()*sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

Ctx* ctx_for_device(int device_ordinal){
  std::lock_guard<std::mutex> lock(g_ctx_mutex);          // concurrent first calls must not both build the tables
  auto it = g_ctxs.find(device_ordinal);
  if (it != g_ctxs.end()){ if (hipSetDevice(device_ordinal) != hipSuccess){ g_err = "hipSetDevice failed"; return NULL; } return it->second; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0){
    g_err = "no HIP device available: this library has no CPU path (build/run on an MI355X)"; return NULL; }
  if (device_ordinal < 0 || device_ordinal >= ndev){ g_err = "device ordinal out of range"; return NULL; }
  HS_HIP_NULL(hipSetDevice(device_ordinal));
  hipDeviceProp_t prop;
  HS_HIP_NULL(hipGetDeviceProperties(&prop, device_ordinal));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0){
    g_err = std::string("kernels are built for gfx950 only; device is ") + prop.gcnArchName; return NULL; }
  const hipstr::HostTables& T = hipstr::host_tables();
  std::vector<double> m2m(T.m2m, T.m2m+16), m2i(T.m2i, T.m2i+16);
  Ctx* c = new Ctx();
  c->device = device_ordinal;
  c->pin_cache.pinned = true;
  // free blocks the caches may hold: every batch in flight returns its workspaces at once when a stream drains (eight 2 Mi-pair batches of
  // 500-read loci: 60 GB), and a block given back to the driver is a hipFree (which synchronises the device) plus a hipMalloc later —
  // so: 70 % of the device's memory (288 GB on an MI355X), 24 GiB of pinned host memory as the most IDLE bytes a cache keeps (BlockCache::put
  // trims the chunks nobody uses beyond that; BlockCache::get reuses any large-enough free block and trims when the driver refuses)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = (size_t)96 << 30;
  c->dev_cache.cap = getenv("HIPSTR_DEV_CACHE_GIB") ? (size_t)(atof(getenv("HIPSTR_DEV_CACHE_GIB"))*1073741824.0) : (size_t)(0.7*(double)total_b);
  c->pin_cache.cap = (size_t)((getenv("HIPSTR_PIN_CACHE_GIB") ? atof(getenv("HIPSTR_PIN_CACHE_GIB")) : 24.0)*1073741824.0);
  if (upload_table(T.int_log, &c->int_log) || upload_table(T.qual_correct, &c->qc) || upload_table(T.qual_error, &c->qe) ||
      upload_table(m2m, &c->m2m) || upload_table(m2i, &c->m2i) ||
      hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess){
    if (g_err.empty()) g_err = "hipStreamCreate failed";
    delete c; return NULL;
  }
  g_ctxs[device_ordinal] = c;
  return c;
}

Ctx* current_ctx(){
  if (t_ctx) return t_ctx;
  {     // a thread that never called hipstr_hmm_init uses the process' first context, or device 0
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    if (!g_ctxs.empty()) t_ctx = g_ctxs.begin()->second;
  }
  if (!t_ctx) t_ctx = ctx_for_device(0);
  return t_ctx;
}

int bind(Ctx* c){ HS_HIP(hipSetDevice(c->device)); return 0; }
}  // namespace

namespace {
// HIPSTR_WAIT: 0 spin (the driver's own wait), 1 yield then sleep, 2 sleep from the first poll
int wait_mode(){
  static const int mode = []{ const char* e = getenv("HIPSTR_WAIT"); return !e ? 1 : !strcmp(e, "spin") ? 0 : !strcmp(e, "sleep") ? 2 : 1; }();
  return mode;
}
// the one polling loop of wait_stream and wait_event: `query` until it is no longer hipErrorNotReady
template <typename Query> hipError_t poll_until_ready(Query query){
  const auto t0 = std::chrono::steady_clock::now();
  bool slow = (wait_mode() == 2);
  for (unsigned n = 0;; n++){
    const hipError_t e = query();
    if (e != hipErrorNotReady) return e;
    if (slow) usleep(50);
    else {
      sched_yield();
      if ((n & 15) == 15 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) slow = true;
    }
  }
}
}  // namespace

hipError_t hipstr::wait_event(hipEvent_t ev){
  if (wait_mode() == 0) return hipEventSynchronize(ev);
  return poll_until_ready([&]{ return hipEventQuery(ev); });
}

hipError_t hipstr::wait_stream(hipStream_t st){
  if (wait_mode() == 0) return hipStreamSynchronize(st);
  // (round 6: an event recorded behind the stream's work and hipEventQuery — a hipStreamQuery that finds the stream busy leaves work for the
  //  HSA runtime's event thread: 0.45 s of its CPU per 3 s of polling against 0.03 with an event, profiles/r06_runtime_thread_probe.txt; sixteen host threads
  //  of one-shot calls share that one thread)
  // (the event comes from this thread's context: only when that is the device the entry point bound — the stream's)
  Ctx* c = t_ctx;
  { int cur = -1; if (!c || hipGetDevice(&cur) != hipSuccess || cur != c->device) c = NULL; }
  hipEvent_t ev = c ? c->get_event(false) : NULL;
  if (ev && hipEventRecord(ev, st) != hipSuccess){ c->put_event(ev, false); ev = NULL; }
  if (!ev) return poll_until_ready([&]{ return hipStreamQuery(st); });
  const hipError_t e = poll_until_ready([&]{ return hipEventQuery(ev); });
  c->put_event(ev, false);
  return e;
}

namespace {

// Device-to-host copy into the caller's (pageable) array: small ones directly, large ones through a pinned block from the cache
// (the driver stages pageable copies itself at a fraction of the link rate) and onto the caller's pages by the host threads.
int fetch_array(Ctx* c, hipStream_t st, void* dst, const void* src, size_t bytes){
  if (bytes == 0) return 0;
  if (bytes < ((size_t)4 << 20)){ HS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); HS_HIP(hipstr::wait_stream(st)); return 0; }
  char* pin = (char*)c->pin_cache.get(bytes);
  if (!pin) return 1;
  if (hipMemcpyAsync(pin, src, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipstr::wait_stream(st) != hipSuccess){
    c->pin_cache.put(pin); return fail("device-to-host copy failed"); }
  const size_t span = (size_t)8 << 20; const int n = (int)((bytes + span - 1)/span);
  hipstr::parallel_for(n, hipstr::host_threads(), [&](int i){ const size_t o = (size_t)i*span; memcpy((char*)dst + o, pin + o, std::min(span, bytes - o)); });
  c->pin_cache.put(pin);
  return 0;
}

// One stream per (host thread, device) for the one-shot and resident entry points: calls made from different host threads — several
// loci in flight, one thread each — neither queue behind one another nor wait for each other's work when they synchronise.
// Objects remember the stream of the thread that created them; streams live until the process ends.
hipStream_t thread_stream(Ctx* c){
  thread_local std::map<Ctx*, hipStream_t> mine;
  auto it = mine.find(c);
  if (it != mine.end()) return it->second;
  hipStream_t st = NULL;
  if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = c->stream;
  mine[c] = st;
  return st;
}

// A second stream per (host thread, device): the tables the device builds for itself (expand_kernels.hip) are inputs of the STR-block kernels
// only, so on the one-shot path they are built here while the caller's stream runs the column tables and the leading flanks (20 us of a
// 190 us one-locus call).  NULL when it cannot be made: the expansion then stays on the upload's stream.  The stutter EM runs its
// allele-frequency scans here (ctx_aux_stream; em.hip joins them into its own stream before it returns).
hipStream_t thread_aux_stream(Ctx* c){
  thread_local std::map<Ctx*, hipStream_t> mine;
  auto it = mine.find(c);
  if (it != mine.end()) return it->second;
  hipStream_t st = NULL;
  if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) st = NULL;
  mine[c] = st;
  return st;
}

}  // namespace

// what the other translation units of the library (trace.hip, em.hip, nw.hip) need from this one: api_internal.h
namespace hipstr {
int api_fail(const std::string& m){ return fail(m); }
Ctx* api_current_ctx(){ Ctx* c = current_ctx(); if (c && bind(c)) return NULL; return c; }
int api_bind(Ctx* c){ return bind(c); }
int api_device_tables(ApiTables* t){
  Ctx* c = api_current_ctx();
  if (!c) return 1;
  t->int_log = c->int_log; t->qual_correct = c->qc; t->qual_error = c->qe; t->m2m = c->m2m; t->m2i = c->m2i;
  t->stream = thread_stream(c); t->ctx = c;
  return 0;
}
void* dev_alloc(Ctx* c, size_t bytes){ return c->dev_cache.get(bytes); }
void  dev_free(Ctx* c, void* p){ c->dev_cache.put(p); }
void* pin_alloc(Ctx* c, size_t bytes){ return c->pin_cache.get(bytes); }
void  pin_free(Ctx* c, void* p){ c->pin_cache.put(p); }
}  // namespace hipstr

namespace hipstr {
// Batch-wide facts the launch decisions of hipstr_hmm_align depend on (computed by the upload, and by hipstr_debug_launch_plan from the same code).
struct LaunchFacts {
  int band_cols = 1;             // the longest read side (at least 1): columns of the flank sweeps' boundary rows, picks the systolic form
  int max_rows = 0;              // longest flank rowset of the batch (rows of a flank block): picks the band shape of the trailing-flank sweep
  bool any_pw = false;           // some locus has alleles with piecewise simple lists (hs_str_group_kernel_pw)
  bool any_rp = false;           // ... with lists replayed in the grouped layout (hs_str_group_kernel_rp)
  bool any_short = false;        // some locus has tabulated alleles hs_str_group_kernel_p does not take (period above HS_GRP_MAXP)
};
static LaunchFacts launch_facts(const Prepared& P){
  LaunchFacts f;
  f.band_cols = P.max_side_len > 0 ? P.max_side_len : 1;
  for (const hs_rowset_t& rs : P.rowsets) f.max_rows = std::max(f.max_rows, (int)rs.len);
  for (const hs_locus_t& l : P.loci){
    f.any_short |= (l.n_short[0] > 0 || l.n_short[1] > 0);
    f.any_pw |= (l.n_pw[0] > l.n_tab[0] || l.n_pw[1] > l.n_tab[1]);
    f.any_rp |= (l.n_rp[0] > l.n_pw[0] || l.n_rp[1] > l.n_pw[1]);
  }
  return f;
}
// A call of a locus or two: the interrupted alleles' kernels run beside the tabulated alleles' on the thread's second stream when a chunk
// has at most this many STR items
#define HS_SIDE_STREAM_ITEMS 256
// The STR-block kernels one chunk launches — the one place it is decided: hipstr_hmm_align launches what it says, hipstr_debug_launch_plan
// reports it.  HIPSTR_STR_GROUP=0: one workgroup per read for every tabulated allele (hs_str_kernel), for comparison.
struct StrLaunch { bool per_read, nd, group_p, group, pw, rp, side_stream, long_sides; };
static StrLaunch str_launch(const Prepared& P, const Prepared::Chunk& ch, const LaunchFacts& f){
  StrLaunch L;
  const bool str_group = !(getenv("HIPSTR_STR_GROUP") && atoi(getenv("HIPSTR_STR_GROUP")) == 0);
  const bool items = ch.str_end > ch.str_begin;
  L.per_read = !str_group;
  L.nd = str_group && items && P.ws_nd_size > 0;                   // read-end deletion sums of the tabulated alleles
  L.group_p = str_group && items;                                  // blocks of at least six repeat units (nearly all) through the kernel with a compile-time period
  L.group = str_group && items && f.any_short;                     // periods above HS_GRP_MAXP only
  L.pw = str_group && items && f.any_pw;
  L.rp = str_group && items && f.any_rp;
  L.side_stream = str_group && items && ch.str_end - ch.str_begin <= HS_SIDE_STREAM_ITEMS && (f.any_pw || f.any_rp);
  L.long_sides = str_group && ch.n_long_sides > 0;                 // sides with more columns than a group holds: one workgroup per read
  return L;
}
// workspace budget (doubles per workspace; there are two large ones): HIPSTR_WS_GIB, else 3 Gi doubles
static int64_t ws_budget(double gib){
  int64_t budget = (int64_t)3 << 30;
  if (gib > 0) budget = (int64_t)(gib*134217728.0);
  else if (getenv("HIPSTR_WS_GIB")) budget = (int64_t)(atof(getenv("HIPSTR_WS_GIB"))*134217728.0);
  if (budget < 1024) budget = 1024;
  return budget;
}
}  // namespace hipstr

struct hipstr_dev_batch {
  Ctx* ctx = NULL;
  hipstr::Prepared prep;
  hs_dev_t h;             // host copy of the argument block (device pointers inside)
  hs_dev_t* d_args = NULL;
  std::vector<void*> dev_blocks, pin_blocks;      // from the context's caches
  int grid_y = 1, max_alleles = 1, n_lead_items = 0, n_trail_items = 0, trail_waves = 1;
  hipstr::LaunchFacts facts;     // what the launch decisions depend on (band_cols, max_rows, any_pw / any_rp / any_short)
  size_t grp_lds_bytes = 0, grp_pw_lds_bytes = 0;
  size_t lds_bytes = 0;
  hipEvent_t ev0 = NULL, ev1 = NULL;
  hipEvent_t ev_expand = NULL;            // the device-built tables are ready (recorded on the thread's aux stream; the first pass waits for it before the STR-block kernels)
  hipStream_t aux_pw_stream = NULL;      // the side stream a pass launched the interrupted alleles' kernels on (joined back by an event; hipstr_hmm_free waits for it all the same)
  hipStream_t aux_stream = NULL; bool expand_joined = false; hipStream_t expand_joined_on = NULL;      // (the stream whose first pass waited for ev_expand)
  hipEvent_t ev_h2d = NULL, ev_done = NULL, ev_d2h = NULL;     // upload finished / last pass finished / results in host_out (pipelined use)
  hipStream_t stream = NULL;                // launches, copies and waits of this batch default to it (the creating thread's stream)
  hipStream_t h2d_stream = NULL, d2h_stream = NULL;
  double* host_out = NULL;                  // pinned copy of aln_probs (fetch_begin)
  bool profiling = false, foreign_stream = false, sleepy_wait = false;
  bool aligned = false;                     // hipstr_hmm_align has queued a pass: aln_probs holds (or will hold, in stream order) a forward pass' rows
  bool d2h_pending = false;            // fetch_begin: the copy back is queued once ev_done has fired (fetch_poll / results_wait), not behind a cross-stream wait
  std::mutex d2h_m;
  std::vector<hipEvent_t> prof_pool;        // reusable events; every pass records 5 per chunk (phase boundaries)
  size_t prof_used = 0;
  int64_t algo_bytes = 0, dp_cells = 0;
  double t_prepare = 0, t_stage = 0;        // seconds spent in the host preparation / in packing the staging buffer
};

extern "C" {

const char* hipstr_last_error(void){ return g_err.c_str(); }

int hipstr_batch_out_offsets(const hipstr_batch_t* b, int64_t* out_off){
  if (!b || !out_off) return fail("null argument");
  int64_t acc = 0;
  for (int l = 0; l < b->n_loci; l++){
    out_off[l] = acc;
    acc += (int64_t)(b->read_off[l+1]-b->read_off[l]) * (b->hap_off[l+1]-b->hap_off[l]);
  }
  out_off[b->n_loci] = acc;
  return 0;
}

int hipstr_hmm_init(int device_ordinal){
  Ctx* c = ctx_for_device(device_ordinal);
  if (!c) return 1;
  t_ctx = c;
  return 0;
}

int64_t hipstr_hmm_trim(void){
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  int64_t bytes = 0;
  for (auto& kv : g_ctxs){
    Ctx* c = kv.second;
    if (hipSetDevice(c->device) != hipSuccess) continue;
    bytes += (int64_t)c->dev_cache.trim() + (int64_t)c->pin_cache.trim();
  }
  return bytes;
}

void hipstr_hmm_shutdown(void){
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  for (auto& kv : g_ctxs){
    Ctx* c = kv.second;
    if (hipSetDevice(c->device) != hipSuccess) continue;
    hipDeviceSynchronize();
    c->dev_cache.release(); c->pin_cache.release();
    hipFree(c->int_log); hipFree(c->qc); hipFree(c->qe); hipFree(c->m2m); hipFree(c->m2i);
    if (c->rec_table) hipFree(c->rec_table);
    hipStreamDestroy(c->stream);
    delete c;
  }
  g_ctxs.clear();
  t_ctx = NULL;
}

int hipstr_calc_seed_bases(const hipstr_batch_t* b, int32_t* seeds){
  hipstr::ApiTimer prof_t(hipstr::PB_SEED_BASES);
  if (!b || !seeds) return fail("null argument");
  { std::string bad; if (hipstr::validate_tables(b, bad)) return fail(bad); }
  for (int l = 0; l < b->n_loci; l++)
    for (int r = b->read_off[l]; r < b->read_off[l+1]; r++){
      seeds[r] = hipstr::calc_seed_base(b, l, r);
      if (seeds[r] == -2) return fail("Invalid alignment seed or unrecognized CIGAR char (HapAligner.cpp:309,316)");
    }
  return 0;
}

void hipstr_hmm_free(hipstr_dev_batch_t* dev){
  if (!dev) return;
  if (dev->ctx && bind(dev->ctx) == 0){
    // blocks go back to the cache, which hands them to the next batch: whatever still runs on them must have finished
    if (!dev->dev_blocks.empty() || !dev->pin_blocks.empty()){
      hipStreamSynchronize(dev->stream);
      if (dev->h2d_stream && dev->h2d_stream != dev->stream) hipStreamSynchronize(dev->h2d_stream);
      if (dev->d2h_stream && dev->d2h_stream != dev->stream) hipStreamSynchronize(dev->d2h_stream);
      if (dev->ev_expand) hipStreamSynchronize(dev->aux_stream);       // (a batch that was never aligned)
      if (dev->aux_pw_stream && hipStreamQuery(dev->aux_pw_stream) != hipSuccess) hipStreamSynchronize(dev->aux_pw_stream); // (a pass ran the interrupted alleles' kernels on the aligning thread's side stream)
    }
    for (void* p : dev->dev_blocks) dev->ctx->dev_cache.put(p);
    for (void* p : dev->pin_blocks) dev->ctx->pin_cache.put(p);
  }
  if (dev->ctx){         // back to the context's pool (an event that is still pending is simply recorded again by its next user)
    dev->ctx->put_event(dev->ev0, true); dev->ctx->put_event(dev->ev1, true);
    dev->ctx->put_event(dev->ev_h2d, false); dev->ctx->put_event(dev->ev_done, false); dev->ctx->put_event(dev->ev_d2h, false);
    dev->ctx->put_event(dev->ev_expand, false);
  }
  for (hipEvent_t e : dev->prof_pool) hipEventDestroy(e);
  hipstr::recycle_prepared(dev->prep);       // the tables' host storage goes to the next batch (prep.h)
  delete dev;
}

hipstr_dev_batch_t* hipstr_hmm_upload(const hipstr_batch_t* batch){ return hipstr_hmm_upload_seeded(batch, NULL); }

// failure inside hipstr_hmm_upload: release what the half-built batch already owns
#define HS_HIP_DEV(call) do { hipError_t e_ = (call); if (e_ != hipSuccess){ \
  g_err = std::string(#call) + ": " + hipGetErrorString(e_); hipstr_hmm_free(dev); return NULL; } } while (0)

hipstr_dev_batch_t* hipstr_hmm_upload_seeded(const hipstr_batch_t* batch, const int32_t* seed_base){
  Ctx* ctx = hipstr::api_current_ctx();
  if (!ctx) return NULL;
  hipStream_t st = thread_stream(ctx);
  return hipstr::upload_on(ctx, batch, seed_base, st, st);
}

}  // extern "C"

// SURVEY.md §8(d) algorithmic traffic and flank-cell work of one pass (hipstr_hmm_workload; computed when asked for)
static void workload_of(hipstr_dev_batch_t* dev){
  const hipstr::Prepared& P = dev->prep;
  int64_t bytes = 0, cells = 0;
  for (const hs_locus_t& loc : P.loci){
    int64_t hap_bytes = 0, flank_rows = 0; int n_re = 0;
    for (int k = 0; k < loc.n_alleles; k++){
      const hs_allele_t& al = P.alleles[loc.hap_begin + k];
      if (!al.realign) continue;
      const int B = P.stropts[al.str_opt[0]].B;
      hap_bytes += 2*(int64_t)(al.n_flank + B) + 8*13 + 2*6*(int64_t)B + 16;
      flank_rows += al.n_flank; n_re++;
    }
    bytes += hap_bytes;
    for (int i = 0; i < loc.n_reads; i++){
      const hs_read_t& rd = P.reads[loc.read_begin + i];
      if (!P.realign_read[loc.read_begin + i] || rd.seed < 0) continue;
      bytes += 2*(int64_t)rd.len + 8 + 4 + 8*(int64_t)n_re;
      cells += (int64_t)(rd.len - 1) * flank_rows;      // (n_L + n_R) x flank rows, leading flank counted per allele as the reference recomputes it without reuse
    }
  }
  dev->algo_bytes = bytes; dev->dp_cells = cells;
}

// The upload with the copy on a stream of the caller's choice (the pipelined path copies on its own stream so that the next
// batch's tables travel while the previous batch's kernels run); hipstr_hmm_align waits for it through an event.
hipstr_dev_batch_t* hipstr::upload_on(Ctx* ctx, const hipstr_batch_t* batch, const int32_t* seed_base, hipStream_t copy_stream, hipStream_t compute_stream, bool reads_pinned){
  if (bind(ctx)) return NULL;
  hipstr_dev_batch_t* dev = new hipstr_dev_batch_t();
  dev->ctx = ctx;
  dev->h2d_stream = copy_stream;
  dev->stream = compute_stream;
  std::string err;
  const int64_t budget = hipstr::ws_budget(0);
  const auto t_prep0 = std::chrono::steady_clock::now();
  hipstr::adopt_recycled(dev->prep);
  if (hipstr::prepare_batch(batch, dev->prep, err, budget, seed_base)){ g_err = err; hipstr::recycle_prepared(dev->prep); delete dev; return NULL; }
  dev->t_prepare = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_prep0).count();
  if (getenv("HIPSTR_TIMING")) fprintf(stderr, "hipstr_hmm_upload: prepare_batch %.3f ms\n", 1e3*dev->t_prepare);
  hipstr::Prepared& P = dev->prep;
  hs_dev_t& h = dev->h;
  memset(&h, 0, sizeof h);
  // ---- one device block for everything the host fills, one pinned block to stage it, one copy
  const auto t_stage0 = std::chrono::steady_clock::now();
  struct Piece { const void* src; size_t bytes, off; };
  std::vector<Piece> pieces;        // what is copied where; a pool gathered from fragments contributes one piece per fragment
  size_t total = 0;
  auto place = [&](const void* src, size_t bytes){ total = (total + 255) & ~(size_t)255; pieces.push_back(Piece{src, bytes, total}); total += bytes ? bytes : 1; return pieces.size() - 1; };
  // a large pool: the batch's own vector (single-threaded preparation) followed by the fragments' (threaded), back to back
  // (tail_bytes: room behind the pool that the host does not fill — the generated part of the f64 pool)
  auto place_pool = [&](const void* own, size_t own_bytes, auto frag_ptr, size_t elem, size_t tail_bytes){
    total = (total + 255) & ~(size_t)255;
    const size_t first = pieces.size();
    pieces.push_back(Piece{own, own_bytes, total}); total += own_bytes;
    for (const hipstr::Prepared& f : P.frags){ const auto& v = f.*frag_ptr; pieces.push_back(Piece{v.data(), v.size()*elem, total}); total += v.size()*elem; }
    total += tail_bytes + 1;
    return first;
  };
  dev->n_lead_items = (int)P.lead_items.size();
  dev->n_trail_items = (int)P.trail_items.size();
#define PL(vec) place((vec).data(), (vec).size()*sizeof((vec)[0]))
  const size_t i_loci = PL(P.loci), i_alleles = PL(P.alleles), i_stropts = PL(P.stropts), i_rowsets = PL(P.rowsets),
    i_rows = place_pool(P.rows.data(), P.rows.size()*sizeof(hs_row_t), &hipstr::Prepared::rows, sizeof(hs_row_t), 0),
    i_visits = place_pool(P.visits.data(), P.visits.size()*sizeof(hs_visit_t), &hipstr::Prepared::visits, sizeof(hs_visit_t), 0),
    i_f64 = place_pool(P.f64pool.data(), P.f64pool.size()*sizeof(double), &hipstr::Prepared::f64pool, sizeof(double), sizeof(double)*(size_t)P.gen_f64),
    i_chars = place_pool(P.chars.data(), P.chars.size(), &hipstr::Prepared::chars, 1, 0),
    i_recd = PL(P.rec_descs), i_pmf = PL(P.pmf13),
    i_reads = PL(P.reads), i_active = PL(P.active),
    i_ws = PL(P.ws), i_tg = PL(P.tgroups), i_tm = PL(P.tmembers), i_tp = PL(P.tpack), i_ord = PL(P.str_order), i_ndr = PL(P.nd_rows);
#undef PL
  // the work items of the three phases, one array on the device: lead | trail | STR
  total = (total + 255) & ~(size_t)255;
  const size_t i_items = pieces.size();
  pieces.push_back(Piece{P.lead_items.data(), P.lead_items.size()*sizeof(hs_item_t), total}); total += P.lead_items.size()*sizeof(hs_item_t);
  pieces.push_back(Piece{P.trail_items.data(), P.trail_items.size()*sizeof(hs_item_t), total}); total += P.trail_items.size()*sizeof(hs_item_t);
  pieces.push_back(Piece{P.str_items.data(), P.str_items.size()*sizeof(hs_item_t), total}); total += P.str_items.size()*sizeof(hs_item_t) + 1;
  const size_t i_args = place(&h, sizeof h);
  // the reads' bases and qualities come last: a caller whose arrays are pinned (the stream's batches) has them copied from where they lie,
  // without a pass through the staging block
  const size_t n_bases = P.reads.empty() ? 0 : (size_t)batch->base_off[P.reads.size()];
  const size_t packed_total = reads_pinned ? ((total + 255) & ~(size_t)255) : 0;
  const size_t i_bases = place(reads_pinned ? NULL : batch->bases, n_bases), i_quals = place(reads_pinned ? NULL : batch->quals, n_bases);
  const size_t stage_total = reads_pinned ? packed_total : total;
  const bool up_prof = hipstr::api_profile_on();
  double up_blocks = 0, up_t = up_prof ? hipstr::ApiTimer::now() : 0;
  char* dblk = (char*)ctx->dev_cache.get(total);
  if (!dblk){ hipstr_hmm_free(dev); return NULL; }
  dev->dev_blocks.push_back(dblk);
  char* stage = (char*)ctx->pin_cache.get(stage_total);
  if (!stage){ hipstr_hmm_free(dev); return NULL; }
  dev->pin_blocks.push_back(stage);
  if (up_prof) up_blocks += hipstr::ApiTimer::now() - up_t;
  auto at = [&](size_t i){ return dblk + pieces[i].off; };
  h.loci = (const hs_locus_t*)at(i_loci); h.alleles = (const hs_allele_t*)at(i_alleles); h.stropts = (const hs_stropt_t*)at(i_stropts);
  h.rowsets = (const hs_rowset_t*)at(i_rowsets); h.rows = (const hs_row_t*)at(i_rows); h.visits = (const hs_visit_t*)at(i_visits);
  h.f64pool = (const double*)at(i_f64); h.chars = (const char*)at(i_chars); h.reads = (const hs_read_t*)at(i_reads);
  h.active = (const int32_t*)at(i_active); h.items = (const hs_item_t*)at(i_items); h.ws = (const hs_ws_t*)at(i_ws);
  h.tgroups = (const hs_tgroup_t*)at(i_tg); h.tmembers = (const int32_t*)at(i_tm); h.tpack = (const int32_t*)at(i_tp);
  h.str_order = (const int32_t*)at(i_ord); h.rec_descs = (const hs_recdesc_t*)at(i_recd); h.pmf13 = (const double*)at(i_pmf); h.nd_rows = (const hs_ndrow_t*)at(i_ndr); h.bases = at(i_bases); h.quals = at(i_quals);
  dev->d_args = (hs_dev_t*)at(i_args);
  // ---- output + workspaces (device only)
  auto dalloc = [&](size_t bytes) -> void* { void* p = ctx->dev_cache.get(bytes ? bytes : 1); if (p) dev->dev_blocks.push_back(p); return p; };
  if (up_prof) up_t = hipstr::ApiTimer::now();
  const size_t out_bytes = (size_t)(P.n_out ? P.n_out : 1) * sizeof(double);
  h.aln_probs = (double*)dalloc(out_bytes);
  h.ws_mr = (double*)dalloc(sizeof(double)*(size_t)P.ws_mr_size); h.ws_lt = (double*)dalloc(sizeof(double)*(size_t)P.ws_lt_size);
  h.ws_lead = (double*)dalloc(sizeof(double)*(size_t)P.ws_lead_size); h.ws_col = (double*)dalloc(sizeof(double)*(size_t)P.ws_col_size);
  h.ws_nd = (double*)dalloc(sizeof(double)*(size_t)P.ws_nd_size);
  h.grp_recs = (const int32_t*)dalloc(sizeof(int32_t)*HS_GRP_REC_DWORDS*P.rec_descs.size());        // assembled on the device (hs_expand_recs_kernel)
  h.n_stropts = (int32_t)P.stropts.size(); h.n_recs = (int32_t)P.rec_descs.size(); h.f64_gen_base = (int64_t)P.n_f64();
  // trailing-flank kernel: persistent wavefronts, each with two band-boundary rows of [max side columns][64 lanes][M,D]
  dev->facts = hipstr::launch_facts(P);
  h.band_cols = dev->facts.band_cols;
  dev->trail_waves = (int)std::min<size_t>(P.trail_items.size() ? P.trail_items.size() : 1, 256 * 16);
  h.ws_band = (double*)dalloc(sizeof(double)*(size_t)dev->trail_waves*h.band_cols*64*2);
  h.lts_rows = 1; h.ws_lts = NULL;          // (fields of the removed fused trailing-flank item: the argument block keeps its layout)
  h.n_active = (int32_t)P.active.size();
  // [n_active] re-do flags of hs_str_kernel | [2 x chunks] work counters of hs_lead_kernel and hs_trail_kernel
  h.redo = (int32_t*)dalloc(sizeof(int32_t)*((size_t)h.n_active + 2*P.chunks.size() + 2));
  if (!h.aln_probs || !h.ws_mr || !h.ws_lt || !h.ws_lead || !h.ws_col || !h.ws_nd || !h.ws_band || !h.redo || !h.grp_recs){ hipstr_hmm_free(dev); return NULL; }
  if (up_prof){ up_blocks += hipstr::ApiTimer::now() - up_t; hipstr::api_profile_add(hipstr::PB_UP_BLOCKS, up_blocks); }
  const hipstr::HostTables& T = hipstr::host_tables();
  h.int_log = ctx->int_log; h.qual_correct = ctx->qc; h.qual_error = ctx->qe; h.m2m = ctx->m2m; h.m2i = ctx->m2i;
  h.log_thresh = T.log_thresh; h.log_half = T.log_half;
  h.lds_len = P.max_read_len;
  h.debug_redo = getenv("HIPSTR_DEBUG_REDO") ? atoi(getenv("HIPSTR_DEBUG_REDO")) : 0;
  // Workgroups: one per (active read[, side]), times enough allele chunks to put >= ~8192 wavefronts on the 256 CUs
  int maxA = 1;
  for (const hs_locus_t& l : P.loci) maxA = l.n_alleles > maxA ? l.n_alleles : maxA;
  int gy = 1;
  if (h.n_active > 0 && h.n_active < 4096){ gy = (4096 + h.n_active - 1) / h.n_active; if (gy > maxA) gy = maxA; }
  h.allele_chunk = (maxA + gy - 1) / gy;
  dev->grid_y = (maxA + h.allele_chunk - 1) / h.allele_chunk;
  dev->max_alleles = maxA;
  h.max_B = P.max_B;
  dev->lds_bytes = hs_str_lds_bytes(h.lds_len, h.max_B);
  if (dev->lds_bytes > 160*1024){ g_err = "batch needs more than 160 KiB of LDS per workgroup"; hipstr_hmm_free(dev); return NULL; }
  h.grp_nd_cap = std::max(2, (P.grp_nd_cap + 1) & ~1);
  dev->grp_lds_bytes = hs_str_group_lds_bytes(h.max_B, h.grp_nd_cap, 0);
  dev->grp_pw_lds_bytes = hs_str_group_lds_bytes(h.max_B, h.grp_nd_cap, 1);
  if (dev->grp_pw_lds_bytes > 48*1024){
    HS_HIP_DEV(hipFuncSetAttribute((const void*)hs_str_group_kernel_pw, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dev->grp_pw_lds_bytes));
    HS_HIP_DEV(hipFuncSetAttribute((const void*)hs_str_group_kernel_rp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dev->grp_pw_lds_bytes));
  }
  if (getenv("HIPSTR_TIMING")) fprintf(stderr, "hipstr_hmm_upload: STR group kernel LDS %zu bytes (max block %d, read-end table %d doubles, %zu groups)\n", dev->grp_lds_bytes, h.max_B, h.grp_nd_cap, P.str_items.size());
  if (dev->grp_lds_bytes > 48*1024){
    HS_HIP_DEV(hipFuncSetAttribute((const void*)hs_str_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dev->grp_lds_bytes));
  }
  if (dev->lds_bytes > 48*1024){
    HS_HIP_DEV(hipFuncSetAttribute((const void*)hs_str_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dev->lds_bytes));
    HS_HIP_DEV(hipFuncSetAttribute((const void*)hs_str_kernel_generic, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dev->lds_bytes));
  }
  // ---- pack (large pieces cut into 4 MiB spans so that the copy is shared by the host threads) and send
  {
    struct Span { char* dst; const char* src; size_t n; };
    std::vector<Span> spans;
    for (const Piece& pc : pieces)
      for (size_t o = 0; pc.src && o < pc.bytes; o += (size_t)4 << 20)
        spans.push_back(Span{stage + pc.off + o, (const char*)pc.src + o, std::min<size_t>((size_t)4 << 20, pc.bytes - o)});
    hipstr::parallel_for((int)spans.size(), stage_total > ((size_t)8 << 20) ? hipstr::host_threads() : 1, [&](int i){ memcpy(spans[i].dst, spans[i].src, spans[i].n); });
  }
  { hipstr::Prepared only_frags; only_frags.frags.swap(P.frags); hipstr::recycle_prepared(only_frags); }      // the fragments' pools are packed: their storage can serve the next batch already
  dev->t_stage = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_stage0).count();
  if (up_prof) up_t = hipstr::ApiTimer::now();
  HS_HIP_DEV(hipMemcpyAsync(dblk, stage, stage_total, hipMemcpyHostToDevice, copy_stream));
  if (reads_pinned && n_bases){
    HS_HIP_DEV(hipMemcpyAsync(dblk + pieces[i_bases].off, batch->bases, n_bases, hipMemcpyHostToDevice, copy_stream));
    HS_HIP_DEV(hipMemcpyAsync(dblk + pieces[i_quals].off, batch->quals, n_bases, hipMemcpyHostToDevice, copy_stream));
  }
  if (up_prof){ const double n_ = hipstr::ApiTimer::now(); hipstr::api_profile_add(hipstr::PB_UP_MEMCPY, n_ - up_t); up_t = n_; }
  // what the device builds for itself (expand_kernels.hip), behind the copies on the same stream and in front of everything else
  // One-shot path (copies and kernels on ONE stream): aside, on the thread's second stream, beside the column tables and the leading flanks
  hipStream_t exp_stream = copy_stream;
  if (copy_stream == compute_stream && (P.gen_f64 > 0 || !P.rec_descs.empty()) && (dev->aux_stream = thread_aux_stream(ctx)) != NULL){
    hipEvent_t fork = ctx->get_event(false); dev->ev_expand = ctx->get_event(false);
    if (fork && dev->ev_expand && hipEventRecord(fork, copy_stream) == hipSuccess && hipStreamWaitEvent(dev->aux_stream, fork, 0) == hipSuccess) exp_stream = dev->aux_stream;
    else { ctx->put_event(dev->ev_expand, false); dev->ev_expand = NULL; }
    ctx->put_event(fork, false);          // (its wait is queued: the event may be recorded again by its next user)
  }
  if (P.gen_f64 > 0) hipLaunchKernelGGL(hs_expand_stropts_kernel, dim3((unsigned)((P.stropts.size() + 3)/4)), dim3(256), 0, exp_stream, (const hs_dev_t*)dev->d_args);
  if (!P.rec_descs.empty()) hipLaunchKernelGGL(hs_expand_recs_kernel, dim3((unsigned)((P.rec_descs.size()*HS_GRP_REC_DWORDS + 255)/256)), dim3(256), 0, exp_stream, (const hs_dev_t*)dev->d_args);
  HS_HIP_DEV(hipGetLastError());
  if (dev->ev_expand) HS_HIP_DEV(hipEventRecord(dev->ev_expand, dev->aux_stream));
  // entries no kernel writes (reads or alleles that are not realigned, reads without a seed) read as 0 for whoever takes the device pointer
  // (hipstr_hmm_dev_aln_probs); a batch where every read is active and every allele realigned — the usual one — has none: no fill launch
  bool all_written = P.active.size() == P.reads.size();
  for (size_t li = 0; all_written && li < P.loci.size(); li++) all_written = P.loci[li].n_re == P.loci[li].n_alleles;
  if (!all_written) HS_HIP_DEV(hipMemsetAsync(h.aln_probs, 0, out_bytes, copy_stream));
  if (up_prof){ const double n_ = hipstr::ApiTimer::now(); hipstr::api_profile_add(hipstr::PB_UP_EXPAND, n_ - up_t); up_t = n_; }
  dev->ev0 = ctx->get_event(true); dev->ev1 = ctx->get_event(true);
  // The stream's batches take tens of milliseconds and their collectors must not burn a core waiting: hipEventSynchronize spins at 100 %
  // of a CPU on this stack whatever the event's flags (tools/wait_probe.hip: 41.7 ms of thread CPU per 41.7 ms of waiting, also with
  // hipEventBlockingSync), a query + usleep loop costs 0.6 ms (results_wait).
  dev->sleepy_wait = reads_pinned;
  dev->ev_h2d = ctx->get_event(false); dev->ev_done = ctx->get_event(false); dev->ev_d2h = ctx->get_event(false);
  if (!dev->ev0 || !dev->ev1 || !dev->ev_h2d || !dev->ev_done || !dev->ev_d2h){ g_err = "hipEventCreate failed"; hipstr_hmm_free(dev); return NULL; }
  HS_HIP_DEV(hipEventRecord(dev->ev_h2d, copy_stream));
  if (up_prof) hipstr::api_profile_add(hipstr::PB_UP_EVENTS, hipstr::ApiTimer::now() - up_t);
  if (getenv("HIPSTR_TIMING"))
    fprintf(stderr, "hipstr_hmm_upload: total %.3f ms (prepare %.3f, blocks + staging %.3f), %zu B of tables, %lld alignments\n",
            1e3*std::chrono::duration<double>(std::chrono::steady_clock::now() - t_prep0).count(), 1e3*dev->t_prepare, 1e3*dev->t_stage, total, (long long)P.n_alignments);
  return dev;
}

// Pipelined fetch: the device-to-host copy of aln_probs queued on `copy_stream` behind the batch's last pass; results_wait blocks
// until it has landed in the batch's pinned buffer; scatter_loci then applies the reference's output contract for a range of loci.
// Waiting for an event without a core AND without a sleep's granularity where the wait is short (a one-locus batch of a latency-bound caller goes
// through three of these: upload, kernels, copy back): yield for the first 300 us, then sleep 100 us at a time.
static hipError_t event_wait_sleepy(hipEvent_t ev){
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e;
  for (unsigned n = 0; (e = hipEventQuery(ev)) == hipErrorNotReady; n++){
    if (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(300)) sched_yield(); else usleep(100);
  }
  return e;
}
int hipstr::fetch_begin(hipstr_dev_batch_t* dev, hipStream_t compute_stream, hipStream_t copy_stream){
  if (bind(dev->ctx)) return 1;
  const hipstr::Prepared& P = dev->prep;
  HS_HIP(hipEventRecord(dev->ev_done, compute_stream));
  if (P.n_out && !dev->host_out){
    dev->host_out = (double*)dev->ctx->pin_cache.get((size_t)P.n_out*sizeof(double));
    if (!dev->host_out) return 1;
    dev->pin_blocks.push_back(dev->host_out);
  }
  dev->d2h_stream = copy_stream;
  // Round 6: the copy back is NOT queued behind a hipStreamWaitEvent(copy_stream, ev_done).  A cross-stream wait for an event that tens of
  // milliseconds of kernels stand in front of is resolved by the HSA runtime's event thread ON THE CPU: it spins in the KFD's wait call until
  // the event fires (profiles/r06_runtime_thread_probe.txt: 2.65 s of CPU per 3 s of such waits, nothing for the same kernels without the wait) — with a
  // stream running that was a core in use for as long as the device was busy, a third of a rank's two-CPU allowance.  The copy is queued by
  // whoever finds ev_done fired first: a worker passing by (fetch_poll) or the collector that waits for the results (results_wait).
  std::lock_guard<std::mutex> lg(dev->d2h_m);
  dev->d2h_pending = true;
  return 0;
}
// ev_done has fired (the caller saw it): the copy back and its event, on the copy stream, with nothing to wait for
static int fetch_issue_locked(hipstr_dev_batch_t* dev){
  const hipstr::Prepared& P = dev->prep;
  if (P.n_out) HS_HIP(hipMemcpyAsync(dev->host_out, dev->h.aln_probs, (size_t)P.n_out*sizeof(double), hipMemcpyDeviceToHost, dev->d2h_stream));
  HS_HIP(hipEventRecord(dev->ev_d2h, dev->d2h_stream));
  dev->d2h_pending = false;
  return 0;
}
// a look without waiting: queues the copy back if the batch's kernels are done.  0 = nothing pending any more, 1 = still running, -1 = error
int hipstr::fetch_poll(hipstr_dev_batch_t* dev){
  std::unique_lock<std::mutex> lg(dev->d2h_m, std::try_to_lock);
  if (!lg.owns_lock()) return 1;
  if (!dev->d2h_pending) return 0;
  if (bind(dev->ctx)) return -1;
  const hipError_t e = hipEventQuery(dev->ev_done);
  if (e == hipErrorNotReady) return 1;
  if (e != hipSuccess){ g_err = std::string("hipEventQuery: ") + hipGetErrorString(e); return -1; }
  return fetch_issue_locked(dev) == 0 ? 0 : -1;
}
int hipstr::results_wait(hipstr_dev_batch_t* dev){
  if (bind(dev->ctx)) return 1;
  {
    std::lock_guard<std::mutex> lg(dev->d2h_m);
    if (dev->d2h_pending){
      if (dev->sleepy_wait){
        const hipError_t e = event_wait_sleepy(dev->ev_done);
        if (e != hipSuccess){ g_err = std::string("hipEventQuery: ") + hipGetErrorString(e); return 1; }
      } else HS_HIP(hipEventSynchronize(dev->ev_done));
      if (fetch_issue_locked(dev)) return 1;
    }
  }
  if (dev->sleepy_wait){
    const hipError_t e = event_wait_sleepy(dev->ev_d2h);
    if (e != hipSuccess){ g_err = std::string("hipEventQuery: ") + hipGetErrorString(e); return 1; }
    return 0;
  }
  HS_HIP(hipEventSynchronize(dev->ev_d2h));
  return 0;
}
void hipstr::scatter_loci(const hipstr_dev_batch_t* dev, int l0, int l1, double* aln_probs, int32_t* seeds, const double* from, bool whole){
  const hipstr::Prepared& P = dev->prep;
  if (l1 <= l0) return;
  if (!from) from = dev->host_out;
  const int64_t out0 = whole ? 0 : P.loci[l0].out_off; const int r0 = whole ? 0 : P.loci[l0].read_begin;
  for (int li = l0; li < l1; li++){
    const hs_locus_t& loc = P.loci[li];
    const int A = loc.n_alleles;
    const bool all_haps = loc.n_re == A;
    // the usual locus — every read realigned and seeded, every haplotype realigned — is one block in both layouts
    bool plain = all_haps;
    for (int i = 0; plain && i < loc.n_reads; i++) plain = P.realign_read[loc.read_begin + i] && P.seeds[loc.read_begin + i] >= 0;
    if (plain){
      memcpy(aln_probs + (loc.out_off - out0), from + loc.out_off, sizeof(double)*(size_t)loc.n_reads*(size_t)A);
      memcpy(seeds + (loc.read_begin - r0), P.seeds.data() + loc.read_begin, sizeof(int32_t)*(size_t)loc.n_reads);
      continue;
    }
    for (int i = 0; i < loc.n_reads; i++){
      const int r = loc.read_begin + i;
      if (!P.realign_read[r]) continue;                       // HapAligner.cpp:326-329
      seeds[r - r0] = P.seeds[r];
      double* dst = aln_probs + (loc.out_off - out0) + (int64_t)i*A;
      const double* src = from + loc.out_off + (int64_t)i*A;
      if (P.seeds[r] == -1){ for (int k = 0; k < A; k++) dst[k] = 0; continue; }   // HapAligner.cpp:333-337
      if (all_haps) memcpy(dst, src, sizeof(double)*(size_t)A);
      else for (int k = 0; k < A; k++) if (P.realign_hap[loc.hap_begin + k]) dst[k] = src[k];   // HapAligner.cpp:615-619
    }
  }
}
// Releases a batch whose results have landed on the host (its D2H event completed, hence every kernel that touched its blocks):
// the blocks can go back to the cache without synchronising the stream, which would stall the batches queued behind it.
void hipstr::free_landed(hipstr_dev_batch_t* dev, bool landed){
  if (!dev) return;
  if (landed && dev->ctx && bind(dev->ctx) == 0){
    for (void* p : dev->dev_blocks) dev->ctx->dev_cache.put(p);
    for (void* p : dev->pin_blocks) dev->ctx->pin_cache.put(p);
    dev->dev_blocks.clear(); dev->pin_blocks.clear();
  }
  hipstr_hmm_free(dev);
}
double hipstr::batch_prepare_seconds(const hipstr_dev_batch_t* dev){ return dev ? dev->t_prepare : 0.0; }
hipStream_t hipstr::ctx_stream(Ctx* c){ return c->stream; }
int hipstr::ctx_device(Ctx* c){ return c->device; }
hipStream_t hipstr::ctx_aux_stream(Ctx* c){ hipStream_t st = thread_aux_stream(c); if (!st) fail("hipStreamCreate failed"); return st; }
hipEvent_t hipstr::event_get(Ctx* c){ hipEvent_t e = c->get_event(false); if (!e) fail("hipEventCreate failed"); return e; }
void hipstr::event_put(Ctx* c, hipEvent_t e){ c->put_event(e, false); }
int hipstr::ctx_record_table(Ctx* c, size_t count, void (*fill)(double*), const double** out){
  std::lock_guard<std::mutex> lock(c->rec_m);
  if (!c->rec_table){
    std::vector<double> t(count);
    fill(t.data());
    if (bind(c)) return 1;
    double* p = NULL;
    if (upload_table(t, &p)){ if (p) hipFree(p); return 1; }
    c->rec_table = p;
  }
  *out = c->rec_table;
  return 0;
}

extern "C" {

int hipstr_hmm_align(hipstr_dev_batch_t* dev, void* hip_stream){
  if (!dev) return fail("null device batch");
  if (bind(dev->ctx)) return 1;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : dev->stream;
  if (hip_stream && (hipStream_t)hip_stream != dev->stream) dev->foreign_stream = true;
  dev->aligned = true;
  // the tables were sent on another stream.  Also with nothing to align: what follows on `st` (the copy back, the events that release the
  // batch's blocks to the cache) must come after the upload that is still writing into those blocks
  // (round 6, the stream's batches — the caller is a worker thread with a batch's time to spare: the two events a batch's kernels depend on, the
  //  upload and the table expansion, are waited for HERE, asleep, instead of by hipStreamWaitEvent on a stream that is busy with the previous
  //  batch: a cross-stream wait keeps the HSA runtime's event thread spinning on a CPU while it is pending, fetch_begin.  One-shot calls keep the
  //  device-side waits: theirs are microseconds long and a host round trip would be their latency.
  //  Measured with the two side by side, profiles/r06_host_side_dependencies.txt: the event thread's 0.65-1.04 s per second of streaming gone,
  //  p30 under a rank's two CPUs 8.0-8.5 -> 5.5-6.3 us of CPU per locus, NS 185 -> 80.)
  const bool host_deps = dev->sleepy_wait && !hip_stream;
  auto host_wait = [&](hipEvent_t ev) -> int {
    const hipError_t e = event_wait_sleepy(ev);
    if (e != hipSuccess) return fail(std::string("hipEventQuery: ") + hipGetErrorString(e));
    return 0;
  };
  if (dev->h2d_stream != st){ if (host_deps){ if (host_wait(dev->ev_h2d)) return 1; } else HS_HIP(hipStreamWaitEvent(st, dev->ev_h2d, 0)); }
  if (host_deps && dev->ev_expand && !dev->expand_joined){ if (host_wait(dev->ev_expand)) return 1; dev->expand_joined = true; dev->expand_joined_on = st; }
  if (dev->h.n_active == 0) return 0;
  const hs_dev_t* dp = dev->d_args;
  auto mark = [&]() -> int {
    if (!dev->profiling) return 0;
    if (dev->prof_used == dev->prof_pool.size()){ hipEvent_t e; HS_HIP(hipEventCreate(&e)); dev->prof_pool.push_back(e); }
    HS_HIP(hipEventRecord(dev->prof_pool[dev->prof_used++], st));
    return 0;
  };
  const int n_clear = (int)((size_t)dev->h.n_active + 2*dev->prep.chunks.size() + 2);        // re-do flags + item counters: cleared by hs_col_kernel
  int chunk_no = 0;
  for (const hipstr::Prepared::Chunk& ch : dev->prep.chunks){
    const unsigned nact = ch.active_end - ch.active_begin;
    if (mark()) return 1;
    // leading flanks: persistent wavefronts striding over (locus side, distinct flank, 64 reads) items
    hs_launch_lead2(nact, (unsigned)std::max(1, std::min(dev->trail_waves, ch.lead_end - ch.lead_begin)), st, dp, ch.active_begin, ch.lead_begin, ch.lead_end, 2*chunk_no, dev->h.band_cols, n_clear);
    if (mark()) return 1;
    // (once per stream: a later pass on ANOTHER stream of the caller's is not ordered behind the first one's wait)
    if (dev->ev_expand && (!dev->expand_joined || dev->expand_joined_on != st)){ HS_HIP(hipStreamWaitEvent(st, dev->ev_expand, 0)); dev->expand_joined = true; dev->expand_joined_on = st; }
    // tabulated alleles: reads of a locus side packed into workgroups (HIPSTR_STR_GROUP=0: one workgroup per read, for comparison)
    const hipstr::StrLaunch sl = hipstr::str_launch(dev->prep, ch, dev->facts);
    if (sl.per_read) hipLaunchKernelGGL(hs_str_kernel, dim3(nact, dev->grid_y), dim3(128), dev->lds_bytes, st, dp, ch.active_begin, 0);
    else {
      // A call of a locus or two: the interrupted alleles' kernels beside the tabulated alleles' (different alleles of the same reads: disjoint
      // outputs; the re-do marks both may set are the same value) on the thread's second stream — 18 us of a 180 us call
      hipStream_t st_pw = st; hipEvent_t ev_pw = NULL, ev_fork = NULL;
      if (sl.side_stream){
        hipStream_t aux = thread_aux_stream(dev->ctx);
        ev_fork = aux ? dev->ctx->get_event(false) : NULL;
        ev_pw = ev_fork ? dev->ctx->get_event(false) : NULL;
        if (ev_pw) st_pw = aux; else { dev->ctx->put_event(ev_fork, false); ev_fork = NULL; }
      }
      if (sl.nd)       // read-end deletion sums of the tabulated alleles, every (row, column) a lane
        hipLaunchKernelGGL(hs_nd_kernel, dim3(nact, 2), dim3(256), 0, st, dp, ch.active_begin);
      if (ev_pw){      // (back to the pool once its wait is queued: the next user records it again)
        const bool ok = hipEventRecord(ev_fork, st) == hipSuccess && hipStreamWaitEvent(st_pw, ev_fork, 0) == hipSuccess;
        dev->ctx->put_event(ev_fork, false);
        if (!ok){ dev->ctx->put_event(ev_pw, false); return fail("hipEventRecord / hipStreamWaitEvent failed"); }      // (nothing launched on the side stream yet)
      }
      if (sl.group_p) hipLaunchKernelGGL(hs_str_group_kernel_p, dim3(ch.str_end - ch.str_begin, dev->grid_y), dim3(HS_GRP_COLS), hs_str_group_p_lds_bytes(), st, dp,
                                         dev->n_lead_items + dev->n_trail_items + ch.str_begin);
      if (sl.group)      // periods above HS_GRP_MAXP only (hs_str_group_kernel_p takes the others)
        hipLaunchKernelGGL(hs_str_group_kernel, dim3(ch.str_end - ch.str_begin, dev->grid_y), dim3(HS_GRP_COLS), dev->grp_lds_bytes, st, dp,
                           dev->n_lead_items + dev->n_trail_items + ch.str_begin, 1);
      if (sl.pw)       // interrupted repeats: the piecewise simple lists' closed forms, grouped like the tabulated ones
        hipLaunchKernelGGL(hs_str_group_kernel_pw, dim3(ch.str_end - ch.str_begin, dev->grid_y), dim3(HS_GRP_COLS), dev->grp_pw_lds_bytes, st_pw, dp,
                           dev->n_lead_items + dev->n_trail_items + ch.str_begin);
      if (sl.rp)       // three and more interruptions: lists without a closed form, replayed in the grouped layout
        hipLaunchKernelGGL(hs_str_group_kernel_rp, dim3(ch.str_end - ch.str_begin, dev->grid_y), dim3(HS_GRP_COLS), dev->grp_pw_lds_bytes, st_pw, dp,
                           dev->n_lead_items + dev->n_trail_items + ch.str_begin);
      if (ev_pw){
        // the join: whatever happens the event goes back to the pool, and a join that could not be queued waits for the side stream here —
        // its kernels read and write this batch's blocks, which the caller is about to return to the cache
        dev->aux_pw_stream = st_pw;
        const bool ok = hipEventRecord(ev_pw, st_pw) == hipSuccess && hipStreamWaitEvent(st, ev_pw, 0) == hipSuccess;
        dev->ctx->put_event(ev_pw, false);
        if (!ok){ hipStreamSynchronize(st_pw); return fail("hipEventRecord / hipStreamWaitEvent failed (side stream of the interrupted alleles' kernels)"); }
      }
      if (sl.long_sides)        // sides with more columns than a group holds: one workgroup per read as before
        hipLaunchKernelGGL(hs_str_kernel, dim3(nact, dev->grid_y), dim3(128), dev->lds_bytes, st, dp, ch.active_begin, 1);
    }
    // alleles without a tabulated closed form (interrupted repeats, very long blocks) and whatever hs_str_kernel marked HS_REDO
    hipLaunchKernelGGL(hs_str_kernel_generic, dim3(nact, dev->grid_y), dim3(128), dev->lds_bytes, st, dp, ch.active_begin, sl.per_read ? 0 : 1);
    if (mark()) return 1;
    if (ch.trail_end > ch.trail_begin)     // trailing flanks: persistent wavefronts striding over (read side, allele group) items
      hs_launch_trail((unsigned)std::min(dev->trail_waves, ch.trail_end - ch.trail_begin), st, dp,
                      dev->n_lead_items + ch.trail_begin, dev->n_lead_items + ch.trail_end, 2*chunk_no + 1, dev->h.band_cols, dev->facts.max_rows);
    if (mark()) return 1;
    hipLaunchKernelGGL(hs_combine_kernel, dim3(nact), dim3(64*hs_combine_waves()), 0, st, dp, ch.active_begin);       // compute_aln_logprob
    if (mark()) return 1;
    HS_HIP(hipGetLastError());
    chunk_no++;
  }
  return 0;
}

int hipstr_hmm_profile(hipstr_dev_batch_t* dev, int enable){
  if (!dev) return fail("null device batch");
  dev->profiling = enable != 0;
  return 0;
}

// ms[4*i + {0,1,2,3}] = {leading flanks, STR block, trailing flanks, combine} of pass i (summed over chunks)
int hipstr_hmm_profile_read(hipstr_dev_batch_t* dev, float* ms, int cap){
  if (!dev || !ms) return -1;
  const size_t per_pass = 5 * dev->prep.chunks.size();
  if (per_pass == 0) return 0;
  int n = 0;
  for (size_t base = 0; base + per_pass <= dev->prof_used && n < cap; base += per_pass, n++){
    float acc[4] = {0, 0, 0, 0};
    for (size_t c = 0; c < dev->prep.chunks.size(); c++)
      for (int ph = 0; ph < 4; ph++){
        hipEvent_t a = dev->prof_pool[base + 5*c + ph], b = dev->prof_pool[base + 5*c + ph + 1];
        float t = 0;
        if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&t, a, b) != hipSuccess) return -1;
        acc[ph] += t;
      }
    for (int ph = 0; ph < 4; ph++) ms[4*n + ph] = acc[ph];
  }
  dev->prof_used = 0;
  return n;
}

int hipstr_hmm_workload(hipstr_dev_batch_t* dev, int64_t* n_alignments, int64_t* algorithmic_bytes, int64_t* dp_cells){
  if (!dev) return fail("null device batch");
  if (n_alignments) *n_alignments = dev->prep.n_alignments;
  if (dev->algo_bytes == 0 && dev->dp_cells == 0) workload_of(dev);
  if (algorithmic_bytes) *algorithmic_bytes = dev->algo_bytes;
  if (dp_cells) *dp_cells = dev->dp_cells;
  return 0;
}

int hipstr_hmm_align_timed(hipstr_dev_batch_t* dev, int reps, float* ms_total, float* ms_kernel){
  if (!dev || reps < 1 || !ms_total) return fail("bad argument");
  if (bind(dev->ctx)) return 1;
  hipStream_t st = dev->stream;
  HS_HIP(hipEventRecord(dev->ev0, st));
  for (int i = 0; i < reps; i++) if (hipstr_hmm_align(dev, st)) return 1;
  HS_HIP(hipEventRecord(dev->ev1, st));
  HS_HIP(hipEventSynchronize(dev->ev1));
  HS_HIP(hipEventElapsedTime(ms_total, dev->ev0, dev->ev1));
  if (ms_kernel) *ms_kernel = *ms_total;
  return 0;
}

double* hipstr_hmm_dev_aln_probs(hipstr_dev_batch_t* dev){ return dev ? dev->h.aln_probs : NULL; }

int hipstr_hmm_fetch(hipstr_dev_batch_t* dev, double* aln_probs, int32_t* seeds){
  if (!dev || !aln_probs || !seeds) return fail("null argument");
  if (bind(dev->ctx)) return 1;
  const hipstr::Prepared& P = dev->prep;
  Ctx* ctx = dev->ctx;
  if (dev->foreign_stream) HS_HIP(hipDeviceSynchronize());         // a pass was launched on a stream of the caller's
  hipstr::ScratchBufs S; S.ctx = ctx; S.runs_on(dev->stream);
  double* tmp = NULL;
  if (P.n_out){
    if (S.alloc_pinned(&tmp, (size_t)P.n_out)) return 1;
    if (hipMemcpyAsync(tmp, dev->h.aln_probs, (size_t)P.n_out*sizeof(double), hipMemcpyDeviceToHost, dev->stream) != hipSuccess)
      return fail("hipMemcpyAsync (device to host) failed");
  }
  if (hipstr::wait_stream(dev->stream) != hipSuccess) return fail("hipStreamSynchronize failed");
  // the reference's output contract, locus by locus (loci are independent: shared among the host threads)
  hipstr::parallel_for((int)P.loci.size(), P.n_out > (1 << 20) ? hipstr::host_threads() : 1,
                       [&](int li){ hipstr::scatter_loci(dev, li, li + 1, aln_probs, seeds, tmp, true); });
  S.release(tmp);
  return 0;
}

int hipstr_hmm_process_reads(const hipstr_batch_t* batch, double* aln_probs, int32_t* seeds){
  return hipstr_hmm_process_reads_seeded(batch, NULL, aln_probs, seeds);
}

int hipstr_hmm_process_reads_seeded(const hipstr_batch_t* batch, const int32_t* seed_base, double* aln_probs, int32_t* seeds){
  hipstr::ApiTimer whole(hipstr::PB_PROCESS_READS);
  const bool prof = hipstr::api_profile_on();
  const double t0 = prof ? hipstr::ApiTimer::now() : 0;
  hipstr_dev_batch_t* dev = hipstr_hmm_upload_seeded(batch, seed_base);
  if (!dev) return 1;
  const double t1 = prof ? hipstr::ApiTimer::now() : 0;
  int rc = hipstr_hmm_align(dev, NULL);
  const double t2 = prof ? hipstr::ApiTimer::now() : 0;
  if (!rc) rc = hipstr_hmm_fetch(dev, aln_probs, seeds);
  const double t3 = prof ? hipstr::ApiTimer::now() : 0;
  if (prof){
    hipstr::api_profile_add(hipstr::PB_PR_PREPARE, dev->t_prepare); hipstr::api_profile_add(hipstr::PB_PR_STAGE, dev->t_stage);
    hipstr::api_profile_add(hipstr::PB_PR_UPLOAD_REST, (t1 - t0) - dev->t_prepare - dev->t_stage);
    hipstr::api_profile_add(hipstr::PB_PR_LAUNCH, t2 - t1); hipstr::api_profile_add(hipstr::PB_PR_FETCH, t3 - t2);
  }
  hipstr_hmm_free(dev);
  if (prof) hipstr::api_profile_add(hipstr::PB_PR_FREE, hipstr::ApiTimer::now() - t3);
  return rc;
}

// ---- hipstr_debug_api_profile
extern "C++" {
namespace hipstr {
static std::atomic<bool> g_prof_on(false);
static std::atomic<int64_t> g_prof_ns[PB_COUNT], g_prof_calls[PB_COUNT];
bool api_profile_on(){ return g_prof_on.load(std::memory_order_relaxed); }
void api_profile_add(int bucket, double seconds, int calls){
  g_prof_ns[bucket].fetch_add((int64_t)(seconds*1e9), std::memory_order_relaxed); g_prof_calls[bucket].fetch_add(calls, std::memory_order_relaxed);
}
double ApiTimer::now(){ return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}
}
#ifndef HIPSTR_NO_DEBUG_ABI      // diagnostics (include/hipstr_hmm_debug.h): tests, fuzzers, bench.py — not the drop-in ABI
int64_t hipstr_debug_driver_allocs(void){ return g_driver_allocs.load(); }
namespace {
// the result of a debug primitive: the launch's stream waited for, then one synchronous copy (up to 1 GiB: not through the pinned cache)
int prim_fetch(hipStream_t st, void* dst, const void* src, size_t bytes){
  return hipstr::wait_stream(st) == hipSuccess && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
}
int hipstr_debug_cr_math(int which, const double* x, double* y, int64_t n){
  if (!x || !y || n < 0) return fail("null argument");
  if (n == 0) return 0;
  Ctx* c = current_ctx();
  if (!c || bind(c)) return 1;
  hipstr::ScratchBufs S; S.ctx = c; S.runs_on(c->stream);
  double *dx, *dy;
  int rc = S.put(&dx, x, (size_t)n) || S.alloc(&dy, (size_t)n);
  if (!rc){
    const auto t0 = std::chrono::steady_clock::now();
    const int reps = getenv("HIPSTR_TIMING") ? 10 : 1;
    for (int r = 0; r < reps; r++)
      hipLaunchKernelGGL(hs_cr_math_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, c->stream, which, (const double*)dx, dy, n);
    if (reps > 1 && hipstr::wait_stream(c->stream) == hipSuccess)
      fprintf(stderr, "hipstr_debug_cr_math: %s of %lld arguments x %d launches: %.3f ms per launch\n", which ? "log" : "exp", (long long)n, reps,
              1e3*std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()/reps);
    rc = prim_fetch(c->stream, y, dy, (size_t)n*8);
  }
  return rc ? fail("hipstr_debug_cr_math: device call failed") : 0;
}
// float_lse.h on the device and, the _host forms, on the host (tests/test_float_lse_gpu.py, tests/test_float_lse.py)
namespace {
const int64_t FLOAT_FN_MAX = (int64_t)1 << 28;       // results of one call: 1 GiB
int float_fn_args(int which, uint32_t bits_lo, int64_t count, const uint32_t* out, int n_modes){
  if (!out || count < 0) return fail("null argument");
  if (which < 0 || which >= n_modes) return fail("hipstr_debug_float_fn: no such function");
  if (count > FLOAT_FN_MAX || (uint64_t)bits_lo + (uint64_t)count > ((uint64_t)1 << 32)) return fail("hipstr_debug_float_fn: range too long");
  return 0;
}
// rows of at least one value each, offsets ascending from 0
int lse_vec_args(const double* v, const int64_t* row_off, const double* out, int64_t n_rows){
  if (!v || !row_off || !out || n_rows < 0) return fail("null argument");
  if (n_rows && row_off[0] != 0) return fail("hipstr_debug_fast_lse_vec: row_off[0] != 0");
  for (int64_t r = 0; r < n_rows; r++) if (row_off[r+1] <= row_off[r]) return fail("hipstr_debug_fast_lse_vec: empty row");
  return 0;
}
}
int hipstr_debug_float_fn(int which, uint32_t bits_lo, int64_t count, uint32_t* out_bits){
  if (float_fn_args(which, bits_lo, count, out_bits, 9)) return 1;
  if (count == 0) return 0;
  Ctx* c = current_ctx();
  if (!c || bind(c)) return 1;
  hipstr::ScratchBufs S; S.ctx = c; S.runs_on(c->stream);
  uint32_t* d;
  int rc = S.alloc(&d, (size_t)count);
  if (!rc){
    hipLaunchKernelGGL(hs_float_fn_kernel, dim3((unsigned)((count + 255)/256)), dim3(256), 0, c->stream, which, bits_lo, count, d);
    rc = prim_fetch(c->stream, out_bits, d, (size_t)count*4);
  }
  return rc ? fail("hipstr_debug_float_fn: device call failed") : 0;
}
int hipstr_debug_float_fn_host(int which, uint32_t bits_lo, int64_t count, uint32_t* out_bits){
  if (float_fn_args(which, bits_lo, count, out_bits, 7)) return 1;        // the controls are the device's reciprocal: no host form
  for (int64_t i = 0; i < count; i++){
    const float x = f_from_bits(bits_lo + (uint32_t)i);
    float r;
    switch (which){
      case 0: r = f_fasterexp(x); break;
      case 1: r = f_fasterlog(x); break;
      case 2: r = f_fastexp(x); break;
      case 3: r = f_fastlog(x); break;
      case 4: r = f_lse2_term(x); break;
      case 5: r = f_div_tab(27.7280233f, x); break;
      default: r = f_div_tab(1.72587999f, x); break;
    }
    out_bits[i] = f_to_bits(r);
  }
  return 0;
}
int hipstr_debug_fast_lse2(const double* a, const double* b, double* out, int64_t n){
  if (!a || !b || !out || n < 0) return fail("null argument");
  if (n == 0) return 0;
  Ctx* c = current_ctx();
  if (!c || bind(c)) return 1;
  hipstr::ScratchBufs S; S.ctx = c; S.runs_on(c->stream);
  double *da, *db, *dy;
  int rc = S.put(&da, a, (size_t)n) || S.put(&db, b, (size_t)n) || S.alloc(&dy, (size_t)n);
  if (!rc){
    hipLaunchKernelGGL(hs_fast_lse2_kernel, dim3((unsigned)((n + 255)/256)), dim3(256), 0, c->stream, (const double*)da, (const double*)db, dy, n, hipstr::host_tables().log_thresh);
    rc = prim_fetch(c->stream, out, dy, (size_t)n*8);
  }
  return rc ? fail("hipstr_debug_fast_lse2: device call failed") : 0;
}
int hipstr_debug_fast_lse2_host(const double* a, const double* b, double* out, int64_t n){
  if (!a || !b || !out || n < 0) return fail("null argument");
  const double thr = hipstr::host_tables().log_thresh;
  for (int64_t i = 0; i < n; i++) out[i] = fast_lse2(a[i], b[i], thr);
  return 0;
}
int hipstr_debug_fast_lse_vec(const double* v, const int64_t* row_off, double* out, int64_t n_rows){
  if (lse_vec_args(v, row_off, out, n_rows)) return 1;
  if (n_rows == 0) return 0;
  Ctx* c = current_ctx();
  if (!c || bind(c)) return 1;
  const size_t nv = (size_t)row_off[n_rows];
  hipstr::ScratchBufs S; S.ctx = c; S.runs_on(c->stream);
  double *dv, *dy; int64_t* dr;
  int rc = S.put(&dv, v, nv) || S.put(&dr, row_off, (size_t)n_rows + 1) || S.alloc(&dy, (size_t)n_rows);
  if (!rc){
    hipLaunchKernelGGL(hs_fast_lse_vec_kernel, dim3((unsigned)((n_rows + 63)/64)), dim3(64), 0, c->stream, (const double*)dv, (const int64_t*)dr, dy, n_rows, hipstr::host_tables().log_thresh);
    rc = prim_fetch(c->stream, out, dy, (size_t)n_rows*8);
  }
  return rc ? fail("hipstr_debug_fast_lse_vec: device call failed") : 0;
}
int hipstr_debug_fast_lse_vec_host(const double* v, const int64_t* row_off, double* out, int64_t n_rows){
  if (lse_vec_args(v, row_off, out, n_rows)) return 1;
  const double thr = hipstr::host_tables().log_thresh;
  for (int64_t r = 0; r < n_rows; r++){
    Lse lse;
    for (int pass = 0; pass < 2; pass++){
      lse.start(pass, v[row_off[r]]);
      for (int64_t i = row_off[r]; i < row_off[r+1]; i++) lse.push(pass, v[i], thr);
    }
    out[r] = lse.finish();
  }
  return 0;
}
void* hipstr_debug_cache_get(int64_t bytes){ Ctx* c = current_ctx(); if (!c || bind(c) || bytes < 0) return NULL; return c->dev_cache.get((size_t)bytes); }
void hipstr_debug_cache_put(void* p){ Ctx* c = current_ctx(); if (c && p) c->dev_cache.put(p); }
// Every byte of the calling thread's context's caches that the next get() may hand out — the free blocks and each chunk's not yet carved
// tail — set to `byte`; a block that is out is never touched.  The device is idle first: a block goes back to the cache while the last
// copy out of it may still be queued.
int64_t hipstr_debug_cache_poison(int byte){
  Ctx* c = current_ctx();
  if (!c || bind(c)) return -1;
  if (hipDeviceSynchronize() != hipSuccess){ fail("hipstr_debug_cache_poison: hipDeviceSynchronize failed"); return -1; }
  int64_t filled = 0;
  BlockCache* bc[2] = { &c->dev_cache, &c->pin_cache };
  for (int k = 0; k < 2; k++){
    std::lock_guard<std::mutex> g(bc[k]->m);
    auto fill = [&](void* p, size_t n) -> bool {
      if (n == 0) return true;
      if (bc[k]->pinned) memset(p, byte, n);
      else if (hipMemset(p, byte, n) != hipSuccess) return false;
      filled += (int64_t)n;
      return true;
    };
    for (const auto& fb : bc[k]->free_) if (!fill(fb.second, fb.first)){ fail("hipstr_debug_cache_poison: hipMemset failed"); return -1; }
    for (const BlockCache::Chunk& ch : bc[k]->chunks)
      if (!fill(ch.base + ch.used, ch.size - ch.used)){ fail("hipstr_debug_cache_poison: hipMemset failed"); return -1; }
  }
  if (hipDeviceSynchronize() != hipSuccess){ fail("hipstr_debug_cache_poison: hipDeviceSynchronize failed"); return -1; }
  return filled;
}
int hipstr_debug_cache_stats(int64_t out[12]){
  Ctx* c = current_ctx();
  if (!c) return 1;
  BlockCache* bc[2] = { &c->dev_cache, &c->pin_cache };
  for (int k = 0; k < 2; k++){
    std::lock_guard<std::mutex> g(bc[k]->m);
    size_t held = 0; for (const BlockCache::Chunk& ch : bc[k]->chunks) held += ch.size;
    out[4*k] = (int64_t)held; out[4*k + 1] = (int64_t)bc[k]->cached; out[4*k + 2] = (int64_t)bc[k]->in_use; out[4*k + 3] = (int64_t)bc[k]->cap;
    out[8 + 2*k] = bc[k]->n_fallback; out[9 + 2*k] = bc[k]->n_trim_retry;
  }
  return 0;
}

// Diagnostics: how the (realigned allele, side) pairs of a batch split over the STR kernels — counts[1]: every visiting list tabulated
// (periodic blocks: hs_str_group_kernel_p), counts[2]: simple or piecewise-simple lists (one or two interruptions: hs_str_group_kernel_pw),
// counts[3]: at least one list replayed inside the grouped layout (three and more interruptions: hs_str_group_kernel_rp),
// counts[0]: anything else (hs_str_kernel_generic).
int hipstr_debug_allele_kinds(hipstr_dev_batch_t* dev, int64_t counts[4]){
  if (!dev || !counts) return fail("null argument");
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  const hipstr::Prepared& P = dev->prep;
  for (const hs_allele_t& al : P.alleles)
    if (al.realign) for (int side = 0; side < 2; side++){ const int k = P.stropts[al.str_opt[side]].kind; if (k >= 0 && k <= 3) counts[k]++; }
  return 0;
}

// Diagnostics (tests): a non-blocking HIP stream of the calling thread's context, as a caller of its own would create one, and its release.
void* hipstr_debug_stream_create(void){
  Ctx* ctx = hipstr::api_current_ctx();
  if (!ctx) return NULL;
  hipStream_t st = NULL;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess){ fail("hipStreamCreate failed"); return NULL; }
  return (void*)st;
}
void hipstr_debug_stream_destroy(void* st){ if (st){ hipStreamSynchronize((hipStream_t)st); hipStreamDestroy((hipStream_t)st); } }

// Diagnostics (tests/test_expand_gpu.py): the device's copy of a batch's option records (what = 0), f64 pool with its generated part (1)
// or per-allele records (2), after everything queued by the upload has run.  Returns the bytes the table has (-1 on failure); copies at most cap.
int64_t hipstr_debug_fetch_table(hipstr_dev_batch_t* dev, int what, void* buf, int64_t cap){
  if (!dev || bind(dev->ctx)) return -1;
  const hipstr::Prepared& P = dev->prep;
  const void* src = NULL; int64_t n = 0;
  if (what == 0){ src = dev->h.stropts; n = (int64_t)P.stropts.size()*sizeof(hs_stropt_t); }
  else if (what == 1){ src = dev->h.f64pool; n = (int64_t)(dev->h.f64_gen_base + P.gen_f64)*sizeof(double); }
  else if (what == 2){ src = dev->h.grp_recs; n = (int64_t)P.rec_descs.size()*HS_GRP_REC_DWORDS*sizeof(int32_t); }
  else { fail("unknown table"); return -1; }
  if (hipStreamSynchronize(dev->h2d_stream ? dev->h2d_stream : dev->stream) != hipSuccess){ fail("hipStreamSynchronize failed"); return -1; }
  if (dev->ev_expand && hipStreamSynchronize(dev->aux_stream) != hipSuccess){ fail("hipStreamSynchronize failed"); return -1; }
  const int64_t m = std::min(n, cap);
  if (m > 0 && buf && hipMemcpy(buf, src, (size_t)m, hipMemcpyDeviceToHost) != hipSuccess){ fail("hipMemcpy failed"); return -1; }
  return n;
}

int hipstr_debug_api_profile(int mode, int cap, const char** names, double* seconds, int64_t* calls){
  static const char* const kNames[hipstr::PB_COUNT] = {
    "hipstr_hmm_process_reads[_seeded]", "  prepare_batch", "  pack staging buffer", "  blocks + H2D enqueue", "  kernel launches", "  wait + D2H + scatter", "  release",
    "hipstr_hmm_trace[_seeded]", "  replay + string work (host)", "hipstr_post_run", "hipstr_post_extract", "hipstr_em_train", "hipstr_nw_align",
    "hipstr_stream_submit", "hipstr_stream_take", "hipstr_calc_seed_bases",
    "    upload: device + pinned blocks from the caches", "    upload: hipMemcpyAsync (tables, reads)", "    upload: expansion kernels + output memset", "    upload: events" };
  if (mode == 1){ for (int i = 0; i < hipstr::PB_COUNT; i++){ hipstr::g_prof_ns[i] = 0; hipstr::g_prof_calls[i] = 0; } hipstr::g_prof_on = true; }
  else if (mode == 0) hipstr::g_prof_on = false;
  for (int i = 0; i < hipstr::PB_COUNT && i < cap; i++){
    if (names) names[i] = kNames[i];
    if (seconds) seconds[i] = 1e-9*(double)hipstr::g_prof_ns[i].load();
    if (calls) calls[i] = hipstr::g_prof_calls[i].load();
  }
  return hipstr::PB_COUNT;
}

// Diagnostics for the host preparation (no device needed): the haplotype rows, as the flank sweeps
// consume them, of allele k / side / block (0 = leading flank, 1 = trailing flank) of a ONE-locus batch.
int hipstr_debug_rows(const hipstr_batch_t* batch, int k, int side, int which, uint32_t* rows, int cap){
  hipstr::Prepared P; std::string err;
  if (hipstr::prepare_batch(batch, P, err)){ g_err = err; return -1; }
  if (k < 0 || k >= (int)P.alleles.size() || side < 0 || side > 1) return -1;
  const hs_allele_t& al = P.alleles[k];
  if (!al.realign) return 0;
  const hs_rowset_t rs = P.rowsets[which ? al.trail_rows[side] : al.lead_rows[side]];
  for (int i = 0; i < rs.len && i < cap; i++) rows[i] = P.rows[rs.off + i];
  return rs.len;
}

// Diagnostics (host only): runs the host preparation of a batch with `threads` host threads (0 = default) and returns its wall time
// and a digest of everything it produced — the digest must not depend on the thread count.
int hipstr_debug_prepare(const hipstr_batch_t* batch, int threads, double* seconds, uint64_t* digest){
  hipstr::Prepared P; std::string err;
  hipstr::set_host_threads(threads);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = hipstr::prepare_batch(batch, P, err);
  const auto t1 = std::chrono::steady_clock::now();
  hipstr::set_host_threads(0);
  if (rc){ g_err = err; return 1; }
  if (seconds) *seconds = std::chrono::duration<double>(t1 - t0).count();
  hipstr::prep_profile_print();
  if (digest){
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n){ const uint8_t* q = (const uint8_t*)p; for (size_t i = 0; i < n; i++){ h ^= q[i]; h *= 1099511628211ull; } };
#define HS_MIX(v) mix((v).data(), (v).size()*sizeof((v)[0]))
    HS_MIX(P.loci); HS_MIX(P.alleles); HS_MIX(P.stropts); HS_MIX(P.rowsets);
    HS_MIX(P.rows); for (const hipstr::Prepared& f : P.frags) HS_MIX(f.rows);
    HS_MIX(P.visits); for (const hipstr::Prepared& f : P.frags) HS_MIX(f.visits);
    HS_MIX(P.f64pool); for (const hipstr::Prepared& f : P.frags) HS_MIX(f.f64pool);
    HS_MIX(P.chars); for (const hipstr::Prepared& f : P.frags) HS_MIX(f.chars);
    HS_MIX(P.rec_descs); HS_MIX(P.pmf13);
    HS_MIX(P.reads); HS_MIX(P.active); HS_MIX(P.seeds); HS_MIX(P.realign_read); HS_MIX(P.realign_hap); HS_MIX(P.ws); HS_MIX(P.lead_items);
    HS_MIX(P.trail_items); HS_MIX(P.str_items); HS_MIX(P.tpack); HS_MIX(P.str_order); HS_MIX(P.tgroups); HS_MIX(P.tmembers); HS_MIX(P.chunks); HS_MIX(P.nd_rows);
#undef HS_MIX
    const int64_t tail[9] = { P.ws_mr_size, P.ws_lt_size, P.ws_lead_size, P.ws_col_size, P.max_side_len, P.max_B, P.n_out, P.n_alignments, P.gen_f64 };
    mix(tail, sizeof tail);
    *digest = h;
  }
  return 0;
}

int hipstr_debug_str_groups(const hipstr_batch_t* batch, int32_t* side, int32_t* columns, int32_t* read_off, int cap_groups,
                            int32_t* reads, int cap_reads, int32_t* max_columns){
  if (!batch || !side || !columns || !read_off || !reads) return -1;
  hipstr::Prepared P; std::string err;
  if (hipstr::prepare_batch(batch, P, err)){ g_err = err; return -1; }
  if (max_columns) *max_columns = HS_GRP_COLS;
  const int ng = (int)P.str_items.size();
  if (ng > cap_groups) return -1;
  int nr = 0;
  read_off[0] = 0;
  for (int g = 0; g < ng; g++){
    const hs_item_t& it = P.str_items[g];
    side[g] = it.side; columns[g] = it.rowset;
    if (nr + it.slot > cap_reads) return -1;
    for (int k = 0; k < it.slot; k++) reads[nr++] = P.active[P.tpack[it.active + k]];
    read_off[g + 1] = nr;
  }
  return ng;
}

// Diagnostics (host only): the launch plan of a batch as hipstr_hmm_align would run it, from the same decisions (hs_flank_route, str_launch,
// hs_coop_bands, hs_combine_tier), as one JSON object.  Route names (the "routes" list of every chunk draws from kRoutes):
static const char* const kRoutes[] = {
  "lead_systolic", "lead_latency", "lead_default", "trail_systolic", "trail_latency", "trail_short", "trail_default",
  "hs_str_group_kernel_p", "hs_str_group_kernel", "hs_str_group_kernel_pw", "hs_str_group_kernel_rp", "hs_str_kernel_long", "hs_str_kernel",
  "hs_str_kernel_generic", "str_side_stream", "str_chunk_stream", "rp_list_closed_form", "rp_list_replay", "combine_one", "combine_1", "combine_2", "combine_3", "combine_4",
  "plan_one_chunk", "plan_chunks" };
int hipstr_debug_launch_plan(const hipstr_batch_t* batch, double ws_gib, char* json, int cap){
  if (!batch) return fail("null batch");
  hipstr::Prepared P; std::string err;
  if (hipstr::prepare_batch(batch, P, err, hipstr::ws_budget(ws_gib))){ g_err = err; return -1; }
  const hipstr::LaunchFacts f = hipstr::launch_facts(P);
  int32_t lim[5]; hs_flank_limits(lim);
  std::string o; char b[256];
  auto put = [&](const char* fmt, auto... a){ snprintf(b, sizeof b, fmt, a...); o += b; };
  auto shape = [&](const char* name, int trail, int route){ int R, W; hs_flank_shape(trail, route, &R, &W); put("\"%s\": [%d, %d], ", name, R, W); };
  put("{\"thresholds\": {\"HS_SYS_ITEMS\": %d, \"HS_LAT_ITEMS\": %d, \"HS_SYS_MAXCOLS\": %d, \"HS_SHORT_TRAIL_ROWS\": %d, ", lim[0], lim[1], lim[2], lim[3]);
  put("\"HS_GRP_MAXP\": %d, \"HS_GRP_MAX_BLOCK\": %d, \"HS_MAX_SIDE_LEN\": %d, \"HS_GRP_COLS\": %d, \"HS_PWK_MAX\": %d, \"HS_SIDE_STREAM_ITEMS\": %d, \"HS_CMB_MAX_FLANK\": %d, ",
      HS_GRP_MAXP, HS_GRP_MAX_BLOCK, HS_MAX_SIDE_LEN, HS_GRP_COLS, HS_PWK_MAX, HS_SIDE_STREAM_ITEMS, 64*lim[4]);
  o += "\"shapes\": {";
  shape("lead_systolic", 0, HS_FLANK_SYSTOLIC); shape("lead_latency", 0, HS_FLANK_LATENCY); shape("lead_default", 0, HS_FLANK_DEFAULT);
  shape("trail_systolic", 1, HS_FLANK_SYSTOLIC); shape("trail_latency", 1, HS_FLANK_LATENCY); shape("trail_short", 1, HS_FLANK_SHORT); shape("trail_default", 1, HS_FLANK_DEFAULT);
  o.resize(o.size() - 2); o += "}}, \"routes\": [";
  for (const char* r : kRoutes){ put("\"%s\", ", r); }
  o.resize(o.size() - 2);
  put("], \"max_cols\": %d, \"max_rows\": %d, \"chunks\": [", f.band_cols, f.max_rows);
  static const char* const kLead[] = { "lead_systolic", "lead_latency", "", "lead_default" };
  static const char* const kTrail[] = { "trail_systolic", "trail_latency", "trail_short", "trail_default" };
  for (size_t ci = 0; ci < P.chunks.size(); ci++){
    const hipstr::Prepared::Chunk& ch = P.chunks[ci];
    std::vector<std::string> hit;
    hit.push_back(P.chunks.size() == 1 ? "plan_one_chunk" : "plan_chunks");
    put("%s{\"n_active\": %d, ", ci ? ", " : "", ch.active_end - ch.active_begin);
    // flanks: the route of the launch and, per item in launch order, [rows after the first, rounds, bands of the last round, band heights]
    // (systolic: [rows after the first, bands of 64 rows])
    for (int trail = 0; trail < 2; trail++){
      const int i0 = trail ? ch.trail_begin : ch.lead_begin, i1 = trail ? ch.trail_end : ch.lead_end;
      const int route = hs_flank_route(trail, i1 - i0, f.band_cols, trail ? f.max_rows : 0);
      const char* name = i1 > i0 ? (trail ? kTrail : kLead)[route] : "none";
      if (i1 > i0) hit.push_back(name);
      int R, W; hs_flank_shape(trail, route, &R, &W);
      put("\"%s\": {\"route\": \"%s\", \"items\": %d, \"R\": %d, \"W\": %d, \"bands\": [", trail ? "trail" : "lead", name, i1 - i0, R, W);
      for (int i = i0; i < i1; i++){
        const hs_item_t& it = trail ? P.trail_items[i] : P.lead_items[i];
        const int n_rows = P.rowsets[trail ? P.tgroups[it.slot].rowset : it.rowset].len - 1;
        if (i > i0) o += ", ";
        if (route == HS_FLANK_SYSTOLIC){ put("[%d, %d]", n_rows, (n_rows + 63) / 64); continue; }
        if (n_rows == 0){ o += "[0, 0, 0, []]"; continue; }
        const hs_coop_bands_t cb = hs_coop_bands(n_rows, R, W);
        put("[%d, %d, %d, [%d", n_rows, cb.rounds, cb.nbands - (cb.rounds - 1)*W, cb.nr_rem < cb.nbands ? cb.nr_base : cb.nr_base + 1);
        if (cb.nr_rem > 0 && cb.nr_rem < cb.nbands) put(", %d", cb.nr_base + 1);
        o += "]]";
      }
      o += "]}, ";
    }
    // STR block: which kernels launch, and (active read side, realigned allele) pairs by the kernel that computes them
    const hipstr::StrLaunch sl = hipstr::str_launch(P, ch, f);
    int64_t n_p = 0, n_g = 0, n_pw = 0, n_rp = 0, n_long = 0, n_pr = 0, n_gen = 0;
    // combine: (active read, realigned allele) pairs by form
    int64_t tiers[5] = {0, 0, 0, 0, 0};
    // visiting lists of the chunk's loci' realigned (allele, side) options by the form prep gave them (hs_stropt_t::shape): tabulated
    // simple, piecewise (one or two interruptions), the K-level closed form (three to HS_PWK_MAX breaks), replayed entry by entry
    int64_t lists[4] = {0, 0, 0, 0};
    int last_locus = -1;
    for (int a = ch.active_begin; a < ch.active_end; a++){
      const hs_read_t& rd = P.reads[P.active[a]];
      const hs_locus_t& loc = P.loci[rd.locus];
      if (rd.locus != last_locus){
        last_locus = rd.locus;
        for (int k = 0; k < loc.n_alleles; k++){
          const hs_allele_t& al = P.alleles[loc.hap_begin + k];
          if (!al.realign) continue;
          for (int side = 0; side < 2; side++){
            const hs_stropt_t& so = P.stropts[al.str_opt[side]];
            if (so.kind == 0) continue;
            for (int q = 0; q <= HS_MAXREP; q++){
              if ((q == HS_MAXREP ? so.B : so.B - (q+1)*so.period) < 0) continue;        // a deletion size that is never evaluated
              const int sh = so.shape[q];
              lists[sh >= 0 ? 0 : sh == HS_SHAPE_PIECEWISE ? 1 : sh == HS_SHAPE_PWK ? 2 : 3]++;
            }
          }
        }
      }
      for (int side = 0; side < 2; side++){
        const int n = side ? rd.len - rd.seed - 1 : rd.seed;
        if (n <= 0) continue;
        if (sl.per_read){ n_pr += loc.n_tab[side]; n_gen += loc.n_re - loc.n_tab[side]; continue; }
        if (n > HS_GRP_COLS){ n_long += loc.n_tab[side]; n_gen += loc.n_re - loc.n_tab[side]; continue; }
        n_g += loc.n_short[side]; n_p += loc.n_tab[side] - loc.n_short[side];
        n_pw += loc.n_pw[side] - loc.n_tab[side]; n_rp += loc.n_rp[side] - loc.n_pw[side]; n_gen += loc.n_re - loc.n_rp[side];
      }
      for (int k = 0; k < loc.n_alleles; k++){
        const hs_allele_t& al = P.alleles[loc.hap_begin + k];
        if (al.realign) tiers[hs_combine_tier(al.n_flank, P.rowsets[al.lead_rows[0]].len, lim[4])]++;
      }
    }
    const struct { const char* name; bool launched; int64_t pairs; } ks[] = {
      { "hs_str_group_kernel_p", sl.group_p, n_p }, { "hs_str_group_kernel", sl.group, n_g }, { "hs_str_group_kernel_pw", sl.pw, n_pw },
      { "hs_str_group_kernel_rp", sl.rp, n_rp }, { "hs_str_kernel_long", sl.long_sides, n_long }, { "hs_str_kernel", sl.per_read, n_pr },
      { "hs_str_kernel_generic", true, n_gen } };
    o += "\"str\": {\"launch\": [";
    bool first = true;
    if (sl.nd){ o += "\"hs_nd_kernel\""; first = false; }
    for (const auto& k : ks) if (k.launched){ put("%s\"%s\"", first ? "" : ", ", k.name); first = false; }
    o += "], \"pairs\": {";
    for (size_t i = 0; i < sizeof ks / sizeof ks[0]; i++){
      put("%s\"%s\": %lld", i ? ", " : "", ks[i].name, (long long)ks[i].pairs);
      if (ks[i].launched && ks[i].pairs > 0) hit.push_back(ks[i].name);
    }
    const bool interrupted = sl.pw || sl.rp;
    if (interrupted) hit.push_back(sl.side_stream ? "str_side_stream" : "str_chunk_stream");
    if (sl.rp && n_rp > 0 && lists[2] > 0) hit.push_back("rp_list_closed_form");
    if (sl.rp && n_rp > 0 && lists[3] > 0) hit.push_back("rp_list_replay");
    put("}, \"lists\": {\"simple\": %lld, \"piecewise\": %lld, \"pwk\": %lld, \"replay\": %lld}, ", (long long)lists[0], (long long)lists[1], (long long)lists[2], (long long)lists[3]);
    // the groups of hs_str_group_kernel*: per item [side, columns, reads]
    o += "\"groups\": [";
    for (int i = ch.str_begin; i < ch.str_end; i++) put("%s[%d, %d, %d]", i > ch.str_begin ? ", " : "", P.str_items[i].side, P.str_items[i].rowset, P.str_items[i].slot);
    put("], \"items\": %d, \"side_stream\": %s, \"n_long_sides\": %d}, ", ch.str_end - ch.str_begin, sl.side_stream ? "true" : "false", ch.n_long_sides);
    put("\"combine\": [%lld, %lld, %lld, %lld, %lld], \"routes\": [", (long long)tiers[0], (long long)tiers[1], (long long)tiers[2], (long long)tiers[3], (long long)tiers[4]);
    static const char* const kCmb[] = { "combine_one", "combine_1", "combine_2", "combine_3", "combine_4" };
    for (int t = 0; t < 5; t++) if (tiers[t] > 0) hit.push_back(kCmb[t]);
    for (size_t i = 0; i < hit.size(); i++) put("%s\"%s\"", i ? ", " : "", hit[i].c_str());
    o += "]}";
  }
  o += "]}";
  if (json && cap > 0){ const size_t m = std::min(o.size(), (size_t)cap - 1); memcpy(json, o.data(), m); json[m] = 0; }
  return (int)o.size();
}

int hipstr_debug_simple_table(int bound, int U0, int tail, double entry[3]){
  if (!entry || bound < 0 || U0 < 0 || tail < 0 || tail >= 10000 || U0 >= 10000) return fail("bad argument");
  hipstr::debug_simple_table(bound, U0, tail, entry);
  return 0;
}
#endif  // HIPSTR_NO_DEBUG_ABI

// ----------------------------------------------------------------------------- posteriors
int hipstr_post_offsets(const hipstr_post_batch_t* pb, int64_t* post_off, int64_t* samp_off){
  if (!pb || !post_off || !samp_off) return fail("null argument");
  int64_t po = 0, so = 0;
  for (int l = 0; l < pb->n_loci; l++){
    post_off[l] = po; samp_off[l] = so;
    po += (int64_t)pb->n_samples[l]*pb->n_alleles[l]*pb->n_alleles[l];
    so += pb->n_samples[l];
  }
  post_off[pb->n_loci] = po; samp_off[pb->n_loci] = so;
  return 0;
}

namespace {
// `ll` is a resident read matrix (hipstr_rm_*) whose last scatter / remap was queued on another stream than `st`: `st` waits for it
int rm_order_behind(const double* ll, hipStream_t st);
struct PostRun {
  Ctx* ctx = NULL;
  hipStream_t stream = NULL;        // the creating thread's stream
  std::vector<hs_post_unit_t> units;
  hipstr::ScratchBufs blocks;       // the run's blocks of the context's caches: back when the run goes, behind `stream`
  hs_post_dev_t h;
  hs_post_dev_t* d_args = NULL;
  int64_t n_post = 0, n_samp = 0, n_ll = 0;
  int n_reads = 0;
  // small runs (a locus or a few: everything under 4 MiB): inputs and argument block travel in ONE pinned block with one copy, the three
  // results sit next to each other in the same device block and come back with one copy of res_bytes from log_post on
  size_t res_bytes = 0;
  hipEvent_t ev_up = NULL;          // small runs: recorded on `stream` behind the asynchronous upload; a launch on another stream waits for it
  ~PostRun(){ if (ctx){ ctx->put_event(ev_up, false); bind(ctx); } }
};

// The (locus, sample) units of a posterior batch and the totals of its arrays (host only: hipstr_debug_post_plan builds the same units).
int post_units(const hipstr_post_batch_t* pb, std::vector<hs_post_unit_t>& units, int64_t& n_post, int64_t& n_samp, int64_t& n_ll){
  const hipstr::HostTables& T = hipstr::host_tables();
  int64_t po = 0, so = 0, lo = 0;
  for (int l = 0; l < pb->n_loci; l++){
    const int A = pb->n_alleles[l], S = pb->n_samples[l];
    const int r0 = pb->read_off[l], r1 = pb->read_off[l+1];
    if (A < 1 || A+1 >= 10000) return fail("allele count out of range");
    const bool hap = pb->haploid && pb->haploid[l];
    const double hom = hap ? -T.int_log[A] : T.int_log[2] - T.int_log[A] - T.int_log[A+1];     // genotyper.cpp:20-25
    const double het = hap ? -DBL_MAX/2 : -T.int_log[A] - T.int_log[A+1];                     // genotyper.cpp:27-32
    int r = r0;
    for (int s = 0; s < S; s++){
      hs_post_unit_t u;
      u.post_off = u.prior_off = po + (int64_t)s*A*A; u.n_alleles = A; u.samp_index = (int32_t)(so + s);
      u.log_hom_prior = hom; u.log_het_prior = het;
      u.read_begin = r; u.ll_off = lo + (int64_t)(r-r0)*A;
      while (r < r1 && pb->sample_label[r] == s) r++;
      u.n_reads = r - u.read_begin;
      units.push_back(u);
    }
    if (r != r1) return fail("reads of a locus must be grouped by ascending sample label (genotyper.h:112-119)");
    po += (int64_t)S*A*A; so += S; lo += (int64_t)(r1-r0)*A;
  }
  n_post = po; n_samp = so; n_ll = lo;
  return 0;
}

// The launch of a run's units: the largest unit decides for all (hs_post_split, post_layout.h).
struct PostLaunch { size_t n_units; int max_nd, split; };
PostLaunch post_launch_of(const std::vector<hs_post_unit_t>& units){
  PostLaunch L; L.n_units = units.size(); L.max_nd = 1;
  for (const hs_post_unit_t& u : units) L.max_nd = std::max(L.max_nd, u.n_alleles*u.n_alleles);
  L.split = units.empty() ? 1 : hs_post_split(L.max_nd, L.n_units);          // (no units: nothing is launched)
  return L;
}

int post_setup(const hipstr_post_batch_t* pb, const double* dev_ll, PostRun& R){
  const hipstr::HostTables& T = hipstr::host_tables();
  Ctx* ctx = R.ctx;
  if (post_units(pb, R.units, R.n_post, R.n_samp, R.n_ll)) return 1;
  R.n_reads = pb->n_loci ? pb->read_off[pb->n_loci] : 0;
  memset(&R.h, 0, sizeof R.h);
  if (!dev_ll && !pb->log_aln_probs) return fail("no log_aln_probs given");
  R.h.log_aln_probs = dev_ll; R.h.log_thresh = T.log_thresh; R.h.log_half = T.log_half;
  R.blocks.ctx = ctx; R.blocks.runs_on(R.stream);
  // The run's pieces, once: what the kernels read — the argument block last, it holds the addresses of all the others — then what they
  // write.  at[i] is the pointer that receives piece i's device address.  The two forms differ only in where a piece lives and how it travels.
  hipstr::HostPieces lay; std::vector<void**> at;
  auto piece = [&](auto* where, const void* src, size_t bytes){ at.push_back((void**)where); lay.add(src, bytes); };
  piece(&R.h.units, R.units.data(), R.units.size()*sizeof(hs_post_unit_t));
  piece(&R.h.log_p1, pb->log_p1, sizeof(double)*R.n_reads);
  piece(&R.h.log_p2, pb->log_p2, sizeof(double)*R.n_reads);
  piece(&R.h.read_weight, pb->read_weight, sizeof(int32_t)*R.n_reads);
  if (pb->log_prior) piece(&R.h.log_prior, pb->log_prior, sizeof(double)*R.n_post);
  if (!dev_ll) piece(&R.h.log_aln_probs, pb->log_aln_probs, sizeof(double)*R.n_ll);
  piece(&R.d_args, &R.h, sizeof R.h);
  const size_t in_total = lay.total;
  piece(&R.h.log_post, NULL, sizeof(double)*R.n_post);
  piece(&R.h.sample_total, NULL, sizeof(double)*R.n_samp);
  piece(&R.h.map_gt, NULL, sizeof(int32_t)*2*R.n_samp);
  if (lay.total < ((size_t)4 << 20)){
    // small form: a piece is an offset in the one device block; the inputs are staged in one pinned block and sent with one copy
    char *dblk, *pin;
    if (R.blocks.alloc(&dblk, lay.total) || R.blocks.alloc_pinned(&pin, in_total)) return 1;
    for (size_t i = 0; i < at.size(); i++) *at[i] = dblk + lay.pieces[i].off;
    lay.pack(pin);
    HS_HIP(hipMemcpyAsync(dblk, pin, in_total, hipMemcpyHostToDevice, R.stream));
    R.ev_up = ctx->get_event(false);
    if (!R.ev_up) return fail("hipEventCreate failed");
    HS_HIP(hipEventRecord(R.ev_up, R.stream));
    R.res_bytes = lay.total - in_total;
    return 0;
  }
  // large form: a piece is a block of its own, copied from the caller's array
  for (size_t i = 0; i < at.size(); i++) if (R.blocks.alloc((char**)at[i], lay.pieces[i].bytes)) return 1;
  for (size_t i = 0; i < at.size(); i++){
    const hipstr::HostPieces::Piece& pc = lay.pieces[i];
    if (pc.src && pc.bytes && hipMemcpyAsync(*at[i], pc.src, pc.bytes, hipMemcpyHostToDevice, R.stream) != hipSuccess) return fail("hipMemcpy failed");
  }
  HS_HIP(hipstr::wait_stream(R.stream));       // the sources are the caller's (pageable) arrays: done with them before returning
  return 0;
}
}  // namespace

struct hipstr_post_dev { PostRun R; std::vector<int32_t> n_samples, n_alleles; std::vector<uint8_t> haploid; bool foreign_stream = false; bool launched = false; };

hipstr_post_dev_t* hipstr_post_upload(const hipstr_post_batch_t* pb, const double* dev_log_aln_probs){
  if (!pb){ g_err = "null argument"; return NULL; }
  Ctx* ctx = hipstr::api_current_ctx();
  if (!ctx) return NULL;
  hipstr_post_dev_t* pd = new hipstr_post_dev_t();
  pd->R.ctx = ctx;
  pd->R.stream = thread_stream(ctx);
  if (post_setup(pb, dev_log_aln_probs, pd->R)){ delete pd; return NULL; }
  pd->n_samples.assign(pb->n_samples, pb->n_samples + pb->n_loci);
  pd->n_alleles.assign(pb->n_alleles, pb->n_alleles + pb->n_loci);
  pd->haploid.assign(pb->n_loci, 0);
  if (pb->haploid) pd->haploid.assign(pb->haploid, pb->haploid + pb->n_loci);
  return pd;
}

int hipstr_post_launch(hipstr_post_dev_t* pd, void* hip_stream){
  if (!pd) return fail("null argument");
  if (pd->R.units.empty()){ pd->launched = true; return 0; }
  if (bind(pd->R.ctx)) return 1;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : pd->R.stream;
  if (hip_stream && st != pd->R.stream) pd->foreign_stream = true;
  // a small run's inputs and argument block were sent asynchronously on the run's own stream: a launch elsewhere comes after them
  if (st != pd->R.stream && pd->R.ev_up) HS_HIP(hipStreamWaitEvent(st, pd->R.ev_up, 0));
  if (rm_order_behind(pd->R.h.log_aln_probs, st)) return 1;
  // HIPSTR_DEBUG_HOST_LIBM=1 (tests/test_genotypes_gpu.py): the three places where the device's exp / log enter — the per-sample
  // log-sum-exp over the diplotypes, the streaming log-sum-exps per genotype and the exact pair log-sum-exp of the unphased posterior —
  // are evaluated on the host with its libm, in the reference's order, on the device's accumulated values.  It shows where the
  // one-float-step differences of GL / GLDIFF / PL against the reference come from (they vanish); it is not a way to run the path.
  const bool host_libm = getenv("HIPSTR_DEBUG_HOST_LIBM") && atoi(getenv("HIPSTR_DEBUG_HOST_LIBM")) != 0;
  if (host_libm != (pd->R.h.raw != 0)){
    pd->R.h.raw = host_libm ? 1 : 0;
    HS_HIP(hipMemcpy(pd->R.d_args, &pd->R.h, sizeof pd->R.h, hipMemcpyHostToDevice));
  }
  {
    // few units with many diplotypes each (one sample per locus, 128 haplotypes): the accumulation of a unit is shared by several
    // workgroups, to ~2048 in all (post_kernels.hip; bit-identical either way)
    const PostLaunch L = post_launch_of(pd->R.units);
    const size_t n_units = L.n_units;
    const int split = L.split;
    if (split > 1){
      hipLaunchKernelGGL(hs_posterior_accumulate_kernel, dim3((unsigned)n_units, (unsigned)split), dim3(HS_POST_THREADS), 0, st, (const hs_post_dev_t*)pd->R.d_args);
      hipLaunchKernelGGL(hs_posterior_finish_kernel, dim3((unsigned)n_units), dim3(HS_POST_THREADS), 0, st, (const hs_post_dev_t*)pd->R.d_args);
    } else
      hipLaunchKernelGGL(hs_posterior_kernel, dim3((unsigned)n_units), dim3(HS_POST_THREADS), 0, st, (const hs_post_dev_t*)pd->R.d_args);
  }
  HS_HIP(hipGetLastError());
  pd->launched = true;
  if (host_libm){
    PostRun& R = pd->R;
    HS_HIP(hipstr::wait_stream(st));
    std::vector<double> post((size_t)R.n_post), total((size_t)R.n_samp, 0.0);
    std::vector<int32_t> mapgt(2*(size_t)R.n_samp, -1);
    HS_HIP(hipMemcpy(post.data(), R.h.log_post, sizeof(double)*R.n_post, hipMemcpyDeviceToHost));
    for (const hs_post_unit_t& u : R.units){
      double* v = post.data() + u.post_off;
      const int nd = u.n_alleles*u.n_alleles;
      double mx = v[0];                                   // log_sum_exp (mathops.cpp:44-50)
      for (int i = 1; i < nd; i++) mx = std::max(mx, v[i]);
      double tot = 0.0;
      for (int i = 0; i < nd; i++) tot += exp(v[i] - mx);
      const double lse = mx + log(tot);
      double bv = -1.7976931348623157e308; int bi = -1;   // first maximum, a1-major (genotyper.cpp:88-95)
      for (int i = 0; i < nd; i++){ v[i] -= lse; if (v[i] > bv){ bv = v[i]; bi = i; } }
      total[u.samp_index] = lse;
      if (bi >= 0){ mapgt[2*u.samp_index] = bi / u.n_alleles; mapgt[2*u.samp_index+1] = bi % u.n_alleles; }
    }
    HS_HIP(hipMemcpy(R.h.log_post, post.data(), sizeof(double)*R.n_post, hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(R.h.sample_total, total.data(), sizeof(double)*R.n_samp, hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(R.h.map_gt, mapgt.data(), sizeof(int32_t)*2*R.n_samp, hipMemcpyHostToDevice));
  }
  return 0;
}

#ifndef HIPSTR_NO_DEBUG_ABI
// Diagnostics (host only): the launch hipstr_post_launch would make for a posterior batch, from the same decisions (post_units,
// post_launch_of, hs_post_in_registers, hs_post_reads_per_tile), as one JSON object.
static const char* const kPostRoutes[] = {
  "hs_posterior_kernel", "hs_posterior_accumulate_kernel+hs_posterior_finish_kernel", "post_registers", "post_chunked",
  "post_one_tile", "post_many_tiles", "post_no_reads", "post_one_echunk", "post_many_echunks", "post_empty_share" };
int hipstr_debug_post_plan(const hipstr_post_batch_t* pb, char* json, int cap){
  if (!pb) return fail("null argument"), -1;
  std::vector<hs_post_unit_t> units; int64_t n_post, n_samp, n_ll;
  if (post_units(pb, units, n_post, n_samp, n_ll)) return -1;
  const PostLaunch L = post_launch_of(units);
  std::string o; char b[256];
  auto put = [&](const char* fmt, auto... a){ snprintf(b, sizeof b, fmt, a...); o += b; };
  put("{\"thresholds\": {\"HS_POST_THREADS\": %d, \"HS_POST_ECHUNK\": %d, \"HS_POST_REGS\": %d, \"HS_POST_SPLIT_WGS\": %d, \"HS_POST_SPLIT_MAX_UNITS\": %d}, \"routes\": [",
      HS_POST_THREADS, HS_POST_ECHUNK, HS_POST_REGS, HS_POST_SPLIT_WGS, HS_POST_SPLIT_MAX_UNITS);
  for (const char* r : kPostRoutes) put("\"%s\", ", r);
  o.resize(o.size() - 2);
  const bool split = !units.empty() && L.split > 1;
  put("], \"n_units\": %d, \"max_nd\": %d, \"split\": %d, \"launch\": [", (int)L.n_units, L.max_nd, units.empty() ? 0 : L.split);
  if (split) put("[\"hs_posterior_accumulate_kernel\", %d], [\"hs_posterior_finish_kernel\", %d]", (int)L.n_units*L.split, (int)L.n_units);
  else if (!units.empty()) put("[\"hs_posterior_kernel\", %d]", (int)L.n_units);
  // per unit: [alleles, reads, path (0 registers, 1 chunked), reads per tile (registers), tiles, chunks of exponentials (chunked),
  // workgroups of a split launch whose share of the unit's diplotypes is empty]
  o += "], \"units\": [";
  bool hit[10] = {false};
  if (!units.empty()) hit[split ? 1 : 0] = true;
  for (size_t i = 0; i < units.size(); i++){
    const hs_post_unit_t& u = units[i];
    const int A = u.n_alleles, nd = A*A;
    const bool regs = !split && hs_post_in_registers(nd);
    const int rt = regs ? hs_post_reads_per_tile(A, u.n_reads) : 0, tiles = regs ? (u.n_reads + rt - 1)/rt : 0;
    const int echunks = regs ? 0 : (nd + HS_POST_ECHUNK - 1)/HS_POST_ECHUNK;
    const int used = (nd + HS_POST_THREADS - 1)/HS_POST_THREADS, empty = split ? std::max(0, L.split - used) : 0;
    hit[regs ? 2 : 3] = true;
    if (regs) hit[tiles == 0 ? 6 : tiles == 1 ? 4 : 5] = true; else hit[echunks > 1 ? 8 : 7] = true;
    if (empty > 0) hit[9] = true;
    put("%s[%d, %d, %d, %d, %d, %d, %d]", i ? ", " : "", A, u.n_reads, regs ? 0 : 1, rt, tiles, echunks, empty);
  }
  o += "], \"routes_hit\": [";
  bool first = true;
  for (int i = 0; i < 10; i++) if (hit[i]){ put("%s\"%s\"", first ? "" : ", ", kPostRoutes[i]); first = false; }
  o += "]}";
  if (json && cap > 0){ const size_t m = std::min(o.size(), (size_t)cap - 1); memcpy(json, o.data(), m); json[m] = 0; }
  return (int)o.size();
}
#endif  // HIPSTR_NO_DEBUG_ABI

int hipstr_post_fetch(hipstr_post_dev_t* pd, double* log_post, double* sample_total_ll, int32_t* map_gt, double* locus_total_ll){
  if (!pd || !log_post || !sample_total_ll || !map_gt || !locus_total_ll) return fail("null argument");
  PostRun& R = pd->R;
  if (bind(R.ctx)) return 1;
  if (pd->foreign_stream) HS_HIP(hipDeviceSynchronize());
  if (!(R.res_bytes && !pd->foreign_stream)) HS_HIP(hipstr::wait_stream(R.stream));      // (the small form's one copy is ordered behind the kernel on the same stream)
  if (!R.units.empty() && R.res_bytes){
    char* pin;
    if (R.blocks.alloc_pinned(&pin, R.res_bytes)) return 1;
    if (hipMemcpyAsync(pin, R.h.log_post, R.res_bytes, hipMemcpyDeviceToHost, R.stream) != hipSuccess || hipstr::wait_stream(R.stream) != hipSuccess)
      return fail("device-to-host copy failed");          // (the block goes back with the run, behind the stream)
    const char* base = (const char*)R.h.log_post;
    memcpy(log_post, pin, sizeof(double)*R.n_post); memcpy(sample_total_ll, pin + ((const char*)R.h.sample_total - base), sizeof(double)*R.n_samp);
    memcpy(map_gt, pin + ((const char*)R.h.map_gt - base), sizeof(int32_t)*2*R.n_samp);
    R.blocks.release(pin);
  } else if (!R.units.empty()){
    if (fetch_array(R.ctx, R.stream, log_post, R.h.log_post, sizeof(double)*R.n_post) ||
        fetch_array(R.ctx, R.stream, sample_total_ll, R.h.sample_total, sizeof(double)*R.n_samp) ||
        fetch_array(R.ctx, R.stream, map_gt, R.h.map_gt, sizeof(int32_t)*2*R.n_samp)) return 1;
  }
  int64_t so = 0;
  for (size_t l = 0; l < pd->n_samples.size(); l++){     // sum(sample_total_LLs_) in sample order (genotyper.cpp:75)
    double tot = 0.0;
    for (int s = 0; s < pd->n_samples[l]; s++) tot += sample_total_ll[so+s];
    locus_total_ll[l] = tot;
    so += pd->n_samples[l];
  }
  return 0;
}

void hipstr_post_free(hipstr_post_dev_t* pd){ delete pd; }

// what hipstr_em_train_dev (em_input.hip) reads of a run
extern "C++" {
void hipstr::post_view(const hipstr_post_dev* pd, PostView* v){
  const PostRun& R = pd->R;
  v->ctx = R.ctx; v->stream = R.stream; v->ev_up = R.ev_up; v->d_units = R.h.units; v->units = R.units.data(); v->n_units = R.units.size();
  v->n_loci = pd->n_samples.size(); v->log_p1 = R.h.log_p1; v->log_p2 = R.h.log_p2; v->n_reads = R.n_reads; v->n_samp = R.n_samp;
  v->n_samples = pd->n_samples.data(); v->haploid = pd->haploid.data();
  v->n_alleles = pd->n_alleles.data(); v->map_gt = R.h.map_gt; v->launched = pd->launched; v->foreign_stream = pd->foreign_stream;
}
void hipstr::PostView::locus_tables(std::vector<int32_t>& read_off, std::vector<int32_t>& unit_off) const {
  read_off.assign(n_loci + 1, 0); unit_off.assign(n_loci + 1, 0);
  size_t ui = 0; int rend = 0;
  for (size_t l = 0; l < n_loci; l++){
    read_off[l] = rend;
    for (int s = 0; s < n_samples[l]; s++, ui++){
      if (s == 0) read_off[l] = units[ui].read_begin;
      rend = units[ui].read_begin + units[ui].n_reads;
    }
    read_off[l+1] = rend; unit_off[l+1] = (int32_t)ui;
  }
}
int hipstr::api_tables_of(Ctx* c, ApiTables* t){
  if (!c || bind(c)) return 1;
  t->int_log = c->int_log; t->qual_correct = c->qc; t->qual_error = c->qe; t->m2m = c->m2m; t->m2i = c->m2i;
  t->stream = thread_stream(c); t->ctx = c;
  return 0;
}
}  // extern "C++"

int hipstr_gt_offsets(const hipstr_post_batch_t* pb, const hipstr_gt_request_t* rq, int64_t* gl_off, int64_t* pgl_off){
  if (!pb || !rq || !gl_off || !pgl_off) return fail("null argument");
  int64_t g = 0, pg = 0, so = 0;
  for (int l = 0; l < pb->n_loci; l++){
    const int64_t V = rq->n_variants[l];
    const bool hap = pb->haploid && pb->haploid[l];
    for (int s = 0; s < pb->n_samples[l]; s++, so++){
      gl_off[so] = g; pgl_off[so] = pg;
      g += hap ? V : V*(V+1)/2; pg += hap ? V : V*V;
    }
  }
  gl_off[so] = g; pgl_off[so] = pg;
  return 0;
}

// hipstr_post_extract (order == NULL) and hipstr_post_extract_vcf: the same units, launch and fetches; with an order, hs_gt_permute_kernel
// runs behind the genotype kernel and the fetches read its pieces.
static int post_extract_run(hipstr_post_dev_t* pd, const hipstr_gt_request_t* rq, const hipstr_gt_vcf_order_t* order, hipstr_gt_out_t* out){
  hipstr::ApiTimer prof_t(hipstr::PB_POST_EXTRACT);
  if (!pd || !rq || !out || !rq->n_variants || !rq->hap_to_allele) return fail("null argument");
  if (!out->best_hap || !out->best_gt || !out->log_phased_post || !out->log_unphased_post || !out->hap_log_phased_post || !out->hap_log_unphased_post)
    return fail("null output array");
  const bool any = rq->calc_gls || rq->calc_pls || rq->calc_phased_gls;
  if (any && !out->gl_diff) return fail("gl_diff output missing");
  if ((rq->calc_gls && !out->gls) || (rq->calc_pls && !out->pls) || (rq->calc_phased_gls && !out->phased_gls)) return fail("requested output array missing");
  PostRun& R = pd->R;
  const hipstr::HostTables& T = hipstr::host_tables();
  const size_t n_loci = pd->n_samples.size();
  const bool timing = getenv("HIPSTR_TIMING") != NULL;
  auto t_lap = std::chrono::steady_clock::now();
  auto lap = [&](const char* what){ if (timing){ const auto t2 = std::chrono::steady_clock::now(); fprintf(stderr, "hipstr_post_extract: %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t2 - t_lap).count()); t_lap = t2; } };
  std::vector<hs_gt_unit_t> units;
  std::vector<int32_t> gmem, goff;
  int64_t po = 0, tot = 0, g = 0, pg = 0; int so = 0, map_off = 0;
  for (size_t l = 0; l < n_loci; l++){
    const int A = pd->n_alleles[l], S = pd->n_samples[l], V = rq->n_variants[l];
    const bool hap = pd->haploid[l] != 0;
    if (V < 1 || V > A) return fail("n_variants must be in [1, n_alleles]");
    const int32_t* h2a = rq->hap_to_allele + map_off;
    std::vector<int> count(V, 0);
    for (int a = 0; a < A; a++){ if (h2a[a] < 0 || h2a[a] >= V) return fail("hap_to_allele entry out of range"); count[h2a[a]]++; }
    const int goff_off = (int)goff.size();
    int run = 0;
    for (int v = 0; v < V; v++){ if (count[v] == 0) return fail("every variant must be carried by a haplotype"); goff.push_back(run); run += count[v]; }
    goff.push_back(run);
    for (int v = 0; v < V; v++) for (int a = 0; a < A; a++) if (h2a[a] == v) gmem.push_back(a);
    const double hom = hap ? -T.int_log[A] : T.int_log[2] - T.int_log[A] - T.int_log[A+1];
    const double het = hap ? 0.0 : -T.int_log[A] - T.int_log[A+1];                           // genotyper.cpp:198
    const double gl_ncfg  = hap ? T.int_log[2] + T.int_log[A] - T.int_log[V] : T.int_log[2] + 2*(T.int_log[A] - T.int_log[V]);
    const double pgl_ncfg = hap ? T.int_log[A] - T.int_log[V] : 2*(T.int_log[A] - T.int_log[V]);
    for (int s = 0; s < S; s++, so++){
      hs_gt_unit_t u; memset(&u, 0, sizeof u);
      u.post_off = po + (int64_t)s*A*A; u.tot_off = tot; tot += (int64_t)V*V;
      u.gl_off = g; u.pgl_off = pg; g += hap ? V : (int64_t)V*(V+1)/2; pg += hap ? V : (int64_t)V*V;
      u.n_alleles = A; u.n_variants = V; u.samp_index = so; u.haploid = hap ? 1 : 0;
      u.map_off = map_off; u.goff_off = goff_off;
      u.hom_corr = hom; u.het_corr = het; u.gl_ncfg = gl_ncfg; u.pgl_ncfg = pgl_ncfg;
      units.push_back(u);
    }
    po += (int64_t)S*A*A; map_off += A;
  }
  // the VCF order: per locus a permutation with the reference allele first and its inverse; per unit where its locus' entries begin
  std::vector<int32_t> unit_var, n2o_abs;
  size_t n_var = 0;
  if (order){
    if (!order->new_to_old || !order->old_to_new) return fail("null argument");
    if ((order->allele_bp_diff && !order->bp_diffs) || (order->allele_count && !order->ac)) return fail("requested output array missing");
    unit_var.reserve(units.size());
    for (size_t l = 0; l < n_loci; l++){
      const int V = rq->n_variants[l];
      const int32_t* n2o = order->new_to_old + n_var; const int32_t* o2n = order->old_to_new + n_var;
      if (n2o[0] != 0) return fail("hipstr_post_extract_vcf: new_to_old[0] must be 0 (the reference allele stays first)");
      for (int i = 0; i < V; i++){
        if (n2o[i] < 0 || n2o[i] >= V || o2n[n2o[i]] != i) return fail("hipstr_post_extract_vcf: new_to_old is not a permutation with old_to_new its inverse");
        n2o_abs.push_back((int32_t)n_var + n2o[i]);
      }
      for (int s = 0; s < pd->n_samples[l]; s++) unit_var.push_back((int32_t)n_var);
      n_var += (size_t)V;
    }
  }
  if (units.empty()){
    if (order) for (size_t v = 0; v < n_var; v++){
      if (order->allele_bp_diff) order->bp_diffs[v] = order->allele_bp_diff[n2o_abs[v]];
      if (order->allele_count) order->ac[v] = order->allele_count[n2o_abs[v]];
    }
    return 0;
  }
  lap("units");
  if (bind(R.ctx)) return 1;
  Ctx* ctx = R.ctx;
  hs_gt_dev_t h; memset(&h, 0, sizeof h);
  hs_gt_perm_dev_t hp; memset(&hp, 0, sizeof hp);
  hipstr::HostArena ar;
  const size_t o_units = ar.add(units.data(), units.size()*sizeof(hs_gt_unit_t)), o_h2a = ar.add(rq->hap_to_allele, (size_t)map_off*4),
               o_gmem = ar.add(gmem.data(), gmem.size()*4), o_goff = ar.add(goff.data(), goff.size()*4), o_args = ar.add(&h, sizeof h);
  size_t o_uvar = 0, o_n2o = 0, o_o2n = 0, o_abs = 0, o_bp = 0, o_ac = 0, o_pargs = 0;
  if (order){
    o_uvar = ar.add(unit_var.data(), unit_var.size()*4); o_n2o = ar.add(order->new_to_old, n_var*4); o_o2n = ar.add(order->old_to_new, n_var*4);
    o_abs = ar.add(n2o_abs.data(), n_var*4);
    if (order->allele_bp_diff) o_bp = ar.add(order->allele_bp_diff, n_var*4);
    if (order->allele_count) o_ac = ar.add(order->allele_count, n_var*4);
    o_pargs = ar.add(&hp, sizeof hp);
  }
  if (ar.reserve(ctx)) return 1;
  // the per-sample results, back to back (one copy home); then the variant pairs' totals and the optional outputs, which can be large
  hipstr::ResultBlocks B;
  const size_t r_hap = B.take((size_t)so*2*4), r_gt = B.take((size_t)so*2*4), r_five = B.take((size_t)so*5*8);
  const size_t r_bp = order && order->allele_bp_diff ? B.take(n_var*4) : 0, r_ac = order && order->allele_count ? B.take(n_var*4) : 0;
  B.end_results();
  const size_t d_tot = B.take((size_t)tot*8), d_gls = any ? B.take((size_t)g*8) : 0, d_pls = rq->calc_pls ? B.take((size_t)g*4) : 0,
               d_pgls = rq->calc_phased_gls ? B.take((size_t)pg*8) : 0;
  // the same three in the VCF order (only what is asked for travels)
  const size_t v_gls = order && rq->calc_gls ? B.take((size_t)g*8) : 0, v_pls = order && rq->calc_pls ? B.take((size_t)g*4) : 0,
               v_pgls = order && rq->calc_phased_gls ? B.take((size_t)pg*8) : 0;
  if (B.reserve(ctx, R.stream)) return 1;
  h.units = ar.at<hs_gt_unit_t>(o_units); h.h2a = ar.at<int32_t>(o_h2a); h.gmem = ar.at<int32_t>(o_gmem); h.goff = ar.at<int32_t>(o_goff);
  h.log_post = R.h.log_post; h.sample_total = R.h.sample_total; h.map_gt = R.h.map_gt;
  h.tot = B.dev<double>(d_tot); h.best_gt = B.dev<int32_t>(r_gt);
  double* five = B.dev<double>(r_five);
  h.log_phased = five; h.log_unphased = five + so; h.hap_log_phased = five + 2*(size_t)so; h.hap_log_unphased = five + 3*(size_t)so; h.gl_diff = five + 4*(size_t)so;
  if (any) h.gls = B.dev<double>(d_gls);
  if (rq->calc_pls) h.pls = B.dev<int32_t>(d_pls);
  if (rq->calc_phased_gls) h.pgls = B.dev<double>(d_pgls);
  h.calc_any = any; h.calc_gls = rq->calc_gls; h.calc_pls = rq->calc_pls; h.calc_pgls = rq->calc_phased_gls;
  h.log_thresh = T.log_thresh;
  const bool host_libm = getenv("HIPSTR_DEBUG_HOST_LIBM") && atoi(getenv("HIPSTR_DEBUG_HOST_LIBM")) != 0;      // see hipstr_post_launch
  std::vector<double> h_tot;
  if (host_libm){
    HS_HIP(hipDeviceSynchronize());
    std::vector<double> post((size_t)R.n_post);
    HS_HIP(hipMemcpy(post.data(), R.h.log_post, sizeof(double)*R.n_post, hipMemcpyDeviceToHost));
    h_tot.resize((size_t)tot);
    for (const hs_gt_unit_t& u : units){                  // total_log_phased_posteriors, streamed as genotyper.cpp:148-170 does (mathops.cpp:72-80)
      const int A = u.n_alleles, V = u.n_variants;
      const int32_t* gm = gmem.data() + u.map_off; const int32_t* go = goff.data() + u.goff_off;
      for (int v1 = 0; v1 < V; v1++) for (int v2 = 0; v2 < V; v2++){
        double mx = -1.7976931348623157e308/2, t = 0.0;
        for (int x = go[v1]; x < go[v1+1]; x++) for (int y = go[v2]; y < go[v2+1]; y++){
          const double lv = post[u.post_off + (int64_t)gm[x]*A + gm[y]];
          if (lv <= mx) t += exp(lv - mx); else { t *= exp(mx - lv); t += 1.0; mx = lv; }
        }
        h_tot[u.tot_off + (int64_t)v1*V + v2] = mx + log(t);
      }
    }
    HS_HIP(hipMemcpy(h.tot, h_tot.data(), sizeof(double)*(size_t)tot, hipMemcpyHostToDevice));
    h.tot_given = 1;
  }
  if (order){
    hp.units = h.units; hp.unit_var = ar.at<int32_t>(o_uvar); hp.new_to_old = ar.at<int32_t>(o_n2o); hp.old_to_new = ar.at<int32_t>(o_o2n);
    hp.n2o_abs = ar.at<int32_t>(o_abs); hp.n_var = (int32_t)n_var;
    hp.gls = h.gls; hp.pls = h.pls; hp.pgls = h.pgls; hp.best_gt = h.best_gt;
    if (rq->calc_gls) hp.gls_out = B.dev<double>(v_gls);
    if (rq->calc_pls) hp.pls_out = B.dev<int32_t>(v_pls);
    if (rq->calc_phased_gls) hp.pgls_out = B.dev<double>(v_pgls);
    if (order->allele_bp_diff){ hp.bp_in = ar.at<int32_t>(o_bp); hp.bp_out = B.dev<int32_t>(r_bp); }
    if (order->allele_count){ hp.ac_in = ar.at<int32_t>(o_ac); hp.ac_out = B.dev<int32_t>(r_ac); }
  }
  if (pd->foreign_stream) HS_HIP(hipDeviceSynchronize());          // the posterior kernel may still be running on a stream of the caller's
  if (ar.send(R.stream)) return 1;                                 // (the argument block is complete by now)
  hipLaunchKernelGGL(hs_genotype_kernel, dim3((unsigned)units.size()), dim3(256), 0, R.stream, (const hs_gt_dev_t*)ar.at<hs_gt_dev_t>(o_args));
  HS_HIP(hipGetLastError());
  if (order){
    hipLaunchKernelGGL(hs_gt_permute_kernel, dim3((unsigned)units.size()), dim3(256), 0, R.stream, (const hs_gt_perm_dev_t*)ar.at<hs_gt_perm_dev_t>(o_pargs));
    HS_HIP(hipGetLastError());
    if (order->allele_bp_diff || order->allele_count){
      hipLaunchKernelGGL(hs_gt_gather_kernel, dim3((unsigned)((n_var + 255)/256)), dim3(256), 0, R.stream, (const hs_gt_perm_dev_t*)ar.at<hs_gt_perm_dev_t>(o_pargs));
      HS_HIP(hipGetLastError());
    }
  }
  HS_HIP(hipMemcpyAsync(B.dev<char>(r_hap), R.h.map_gt, (size_t)so*2*4, hipMemcpyDeviceToDevice, R.stream));       // best_hap travels with the rest
  lap("setup");
  if (B.fetch()) return 1;
  lap("kernel");
  const double* hf = B.host<double>(r_five);
  memcpy(out->best_hap, B.host<char>(r_hap), (size_t)so*2*4); memcpy(out->best_gt, B.host<char>(r_gt), (size_t)so*2*4);
  memcpy(out->log_phased_post, hf, (size_t)so*8); memcpy(out->log_unphased_post, hf + so, (size_t)so*8);
  if (host_libm)                                          // the exact pair log_sum_exp of the two phasings (mathops.cpp:52-57) with the host libm
    for (const hs_gt_unit_t& u : units){
      int ga = out->best_gt[2*u.samp_index], gb = out->best_gt[2*u.samp_index+1];
      if (ga < 0 || gb < 0 || ga == gb) continue;
      if (order){ const int32_t* n2o = order->new_to_old + unit_var[u.samp_index]; ga = n2o[ga]; gb = n2o[gb]; }       // h_tot is in block-option order
      const double lp = h_tot[u.tot_off + (int64_t)u.n_variants*ga + gb], alt = h_tot[u.tot_off + (int64_t)u.n_variants*gb + ga];
      out->log_unphased_post[u.samp_index] = (lp > alt) ? lp + log(1 + exp(alt - lp)) : alt + log(1 + exp(lp - alt));
    }
  memcpy(out->hap_log_phased_post, hf + 2*(size_t)so, (size_t)so*8); memcpy(out->hap_log_unphased_post, hf + 3*(size_t)so, (size_t)so*8);
  if (any) memcpy(out->gl_diff, hf + 4*(size_t)so, (size_t)so*8);
  if (order && order->allele_bp_diff) memcpy(order->bp_diffs, B.host<char>(r_bp), n_var*4);
  if (order && order->allele_count) memcpy(order->ac, B.host<char>(r_ac), n_var*4);
  if (rq->calc_gls && fetch_array(ctx, R.stream, out->gls, order ? hp.gls_out : h.gls, (size_t)g*8)) return 1;
  if (rq->calc_pls && fetch_array(ctx, R.stream, out->pls, order ? hp.pls_out : h.pls, (size_t)g*4)) return 1;
  if (rq->calc_phased_gls && fetch_array(ctx, R.stream, out->phased_gls, order ? hp.pgls_out : h.pgls, (size_t)pg*8)) return 1;
  lap("fetch");
  return 0;
}

int hipstr_post_extract(hipstr_post_dev_t* pd, const hipstr_gt_request_t* rq, hipstr_gt_out_t* out){ return post_extract_run(pd, rq, NULL, out); }
int hipstr_post_extract_vcf(hipstr_post_dev_t* pd, const hipstr_gt_request_t* rq, const hipstr_gt_vcf_order_t* order, hipstr_gt_out_t* out){
  if (!order) return fail("null argument");
  return post_extract_run(pd, rq, order, out);
}

// ----------------------------------------------------------------------------- read assignment
namespace {
// The loci of an assignment and its launch, from the posterior run's units (host only).
struct AssignPlan { std::vector<hs_assign_locus_t> loci; std::vector<int32_t> unit_locus; int64_t tab_ints = 0; int max_unit_reads = 0, waves = 1; };
int assign_plan(const hipstr_post_dev_t* pd, const hipstr_assign_request_t* rq, AssignPlan& P){
  const PostRun& R = pd->R;
  const size_t n_loci = pd->n_samples.size();
  P.loci.resize(n_loci); P.unit_locus.resize(R.units.size());
  size_t ui = 0; int rend = 0;
  for (size_t l = 0; l < n_loci; l++){
    hs_assign_locus_t& L = P.loci[l]; memset(&L, 0, sizeof L);
    L.read_begin = rend; L.n_alleles = pd->n_alleles[l];
    for (int s = 0; s < pd->n_samples[l]; s++, ui++){
      const hs_post_unit_t& u = R.units[ui];
      if (s == 0) L.read_begin = u.read_begin;
      rend = u.read_begin + u.n_reads;
      P.unit_locus[ui] = (int32_t)(l << 1) | (pd->haploid[l] ? 1 : 0);
      P.max_unit_reads = std::max(P.max_unit_reads, u.n_reads);
    }
    L.n_reads = rend - L.read_begin;
    if (rq->pool_index){
      const int64_t np = (int64_t)rq->pool_off[l+1] - rq->pool_off[l];
      if (np < 0) return fail("pool_off must not decrease");
      const int64_t n_keys = np*L.n_alleles;
      if (n_keys >= HS_ASSIGN_EMPTY) return fail("too many (pool, haplotype) pairs in a locus");
      for (int r = L.read_begin; r < rend; r++)
        if (rq->pool_index[r] < 0 || rq->pool_index[r] >= np) return fail("pool_index outside the pools of its locus");
      int hashed = 0;
      const int64_t slots = L.n_reads ? hs_assign_table_slots(n_keys, L.n_reads, &hashed) : 0;
      if (slots >= HS_ASSIGN_EMPTY) return fail("too many reads in a locus");
      L.slots = (int32_t)slots; L.hashed = hashed; L.pool_off = rq->pool_off[l];
      L.tab_off = P.tab_ints; P.tab_ints += slots*(hashed ? 3 : 2);
    }
  }
  P.waves = hs_assign_waves_per_unit(P.max_unit_reads);
  return 0;
}
}  // namespace

int hipstr_post_assign(hipstr_post_dev_t* pd, const hipstr_assign_request_t* rq, hipstr_assign_out_t* out){
  if (!pd || !rq || !out || !rq->seed) return fail("null argument");
  if (!out->best_hap || !out->read_strand || !out->log_phase_one || !out->n_aligned || !out->n_snp || !out->n_strand_one || !out->n_strand_two ||
      !out->uniq_one || !out->uniq_two || !out->rv_uniq_one || !out->rv_uniq_two || !out->phase1_reads || !out->phase2_reads) return fail("null output array");
  if (rq->rule != HIPSTR_ASSIGN_VCF && rq->rule != HIPSTR_ASSIGN_RETRACE) return fail("unknown assignment rule");
  if (rq->pool_index && !rq->pool_off) return fail("pool_index given without pool_off");
  if (rq->pool_index && (!out->n_req || !out->req_read || !out->req_allele || !out->read_req || out->cap_req < 0)) return fail("request-list output missing");
  if (!(rq->strand_tolerance >= 0)) return fail("strand_tolerance must not be negative");
  if (!pd->launched) return fail("hipstr_post_assign needs the posteriors: call hipstr_post_launch first");
  PostRun& R = pd->R;
  const hipstr::HostTables& T = hipstr::host_tables();
  const bool req = rq->pool_index != NULL;
  if (R.n_reads >= HS_ASSIGN_EMPTY) return fail("too many reads");
  AssignPlan P;
  if (assign_plan(pd, rq, P)) return 1;
  if (req) *out->n_req = 0;
  if (R.units.empty()) return 0;
  if (bind(R.ctx)) return 1;
  Ctx* ctx = R.ctx;
  const size_t n = (size_t)R.n_reads, ns = (size_t)R.n_samp, nl = P.loci.size();
  const size_t cap = req ? std::min((size_t)out->cap_req, n) : 0;          // (a read makes at most one request)

  hipstr::HostArena ar;
  const size_t o_loci = ar.add(P.loci.data(), nl*sizeof(hs_assign_locus_t)), o_ul = ar.add(P.unit_locus.data(), P.unit_locus.size()*4),
               o_seed = ar.add(rq->seed, n*4), o_rev = rq->reverse ? ar.add(rq->reverse, n) : 0, o_pool = req ? ar.add(rq->pool_index, n*4) : 0;
  hs_assign_dev_t h; memset(&h, 0, sizeof h);
  const size_t o_args = ar.add(&h, sizeof h);
  if (ar.reserve(ctx)) return 1;
  // results, back to back (one copy home), then what stays on the device: counts and bases per locus, the first-occurrence tables
  hipstr::ResultBlocks B;
  const size_t r_nreq = B.take(4), r_best = B.take(n*4), r_strand = B.take(n*4), r_rreq = B.take(n*4), r_lpo = B.take(n*8), r_cnt = B.take(8*ns*4),
               r_ph1 = B.take(ns*8), r_ph2 = B.take(ns*8), r_rr = B.take(cap*4), r_ra = B.take(cap*4);
  B.end_results();
  const size_t d_count = B.take(nl*4), d_base = B.take(nl*4), d_tab = B.take((size_t)P.tab_ints*4);
  if (B.reserve(ctx, R.stream)) return 1;
  h.units = R.h.units; h.log_aln_probs = R.h.log_aln_probs; h.log_p1 = R.h.log_p1; h.log_p2 = R.h.log_p2; h.map_gt = R.h.map_gt;
  h.unit_locus = ar.at<int32_t>(o_ul); h.loci = ar.at<hs_assign_locus_t>(o_loci); h.seed = ar.at<int32_t>(o_seed);
  h.reverse = rq->reverse ? ar.at<uint8_t>(o_rev) : NULL; h.pool_index = req ? ar.at<int32_t>(o_pool) : NULL;
  h.n_units = (int32_t)R.units.size(); h.n_loci = (int32_t)nl; h.rule = rq->rule; h.cap_req = (int32_t)cap;
  h.log_half = T.log_half; h.strand_tolerance = rq->strand_tolerance == 0 ? 0.1 : rq->strand_tolerance;       // seq_stutter_genotyper.h:157
  h.best_hap = B.dev<int32_t>(r_best); h.read_strand = B.dev<int32_t>(r_strand); h.read_req = B.dev<int32_t>(r_rreq);
  h.log_phase_one = B.dev<double>(r_lpo); h.counters = B.dev<int32_t>(r_cnt); h.n_samp = (int32_t)ns;
  h.phase1 = B.dev<double>(r_ph1); h.phase2 = B.dev<double>(r_ph2);
  h.tab = B.dev<int32_t>(d_tab); h.locus_count = B.dev<int32_t>(d_count); h.locus_base = B.dev<int32_t>(d_base);
  h.n_req = B.dev<int32_t>(r_nreq); h.req_read = B.dev<int32_t>(r_rr); h.req_allele = B.dev<int32_t>(r_ra);
  if (pd->foreign_stream) HS_HIP(hipDeviceSynchronize());          // the posterior kernel may still be running on a stream of the caller's
  hipStream_t st = R.stream;
  if (rm_order_behind(R.h.log_aln_probs, st)) return 1;
  if (ar.send(st)) return 1;
  const hs_assign_dev_t* d_args = ar.at<hs_assign_dev_t>(o_args);
  if (req){
    HS_HIP(hipMemsetAsync(B.dev<char>(d_count), 0, nl*4, st));
    if (P.tab_ints) HS_HIP(hipMemsetAsync(B.dev<char>(d_tab), 0x7f, (size_t)P.tab_ints*4, st));
  }
  const unsigned wgs = (unsigned)hs_assign_workgroups((int64_t)R.units.size(), P.waves);
  if (P.waves == 1) hipLaunchKernelGGL(hs_assign_kernel, dim3(wgs), dim3(HS_ASSIGN_THREADS), 0, st, d_args);
  else hipLaunchKernelGGL(hs_assign_kernel_wg, dim3(wgs), dim3(HS_ASSIGN_THREADS), 0, st, d_args);
  if (req){
    hipLaunchKernelGGL(hs_assign_scan_kernel, dim3(1), dim3(HS_ASSIGN_THREADS), 0, st, d_args);
    hipLaunchKernelGGL(hs_assign_requests_kernel, dim3((unsigned)nl), dim3(HS_ASSIGN_THREADS), 0, st, d_args);
  }
  HS_HIP(hipGetLastError());
  if (B.fetch()) return 1;
  const int32_t* bh = B.host<int32_t>(r_best);
  if (req){
    const int32_t n_req = *B.host<int32_t>(r_nreq);
    *out->n_req = n_req;
    if (n_req > out->cap_req){ fail("request arrays too small: *n_req holds the number needed"); return 3; }
    memcpy(out->req_read, B.host<char>(r_rr), (size_t)n_req*4); memcpy(out->req_allele, B.host<char>(r_ra), (size_t)n_req*4);
    memcpy(out->read_req, B.host<char>(r_rreq), n*4);
  }
  memcpy(out->best_hap, bh, n*4); memcpy(out->read_strand, B.host<char>(r_strand), n*4);
  const double* lpo = B.host<double>(r_lpo);
  for (size_t r = 0; r < n; r++) if (bh[r] >= 0) out->log_phase_one[r] = lpo[r];        // (skipped reads: untouched)
  int32_t* const cnt[8] = { out->n_aligned, out->n_snp, out->n_strand_one, out->n_strand_two, out->uniq_one, out->uniq_two, out->rv_uniq_one, out->rv_uniq_two };
  for (int k = 0; k < 8; k++) memcpy(cnt[k], B.host<char>(r_cnt) + (size_t)k*ns*4, ns*4);
  memcpy(out->phase1_reads, B.host<char>(r_ph1), ns*8); memcpy(out->phase2_reads, B.host<char>(r_ph2), ns*8);
  return 0;
}

#ifndef HIPSTR_NO_DEBUG_ABI
// Diagnostics (host only): the launch hipstr_post_assign would make for a posterior batch whose largest unit has max_unit_reads reads
// and a locus of n_keys = pools x haplotypes keys and n_reads reads: out[0] wavefronts per unit, out[1] workgroups, out[2] table slots, out[3] hashed.
int hipstr_debug_assign_plan(int32_t max_unit_reads, int64_t n_units, int64_t n_keys, int64_t n_reads, int64_t out[4]){
  if (!out || max_unit_reads < 0 || n_units < 0 || n_keys < 0 || n_reads < 0) return fail("bad argument");
  int hashed = 0;
  out[0] = hs_assign_waves_per_unit(max_unit_reads); out[1] = hs_assign_workgroups(n_units, (int)out[0]);
  out[2] = hs_assign_table_slots(n_keys, n_reads, &hashed); out[3] = hashed;
  return 0;
}
#endif

// ----------------------------------------------------------------------------- allele census
namespace {
// The loci of a census, their routes and everything the host derives for the device (host only); every refusal of hipstr_post_census.
struct CensusPlan {
  std::vector<hs_census_locus_t> loci;
  std::vector<int32_t> list[3], read_samp, req_locus, o1_off;
  std::string o1_seq;
  int64_t ws_ints = 0, n_opts = 0, n_haps = 0;
};
// tr: the trace's host arrays, or NULL when they lie on the device (hipstr_post_census_dev: the checks of their values run there)
int census_plan(const hipstr_post_dev_t* pd, const hipstr_census_request_t* rq, const hipstr_trace_out_t* tr, CensusPlan& P){
  const PostRun& R = pd->R;
  const hipstr_batch_t* b = rq->pooled;
  const size_t nl = pd->n_samples.size();
  if ((size_t)b->n_loci != nl) return fail("hipstr_post_census: pooled->n_loci differs from the posterior batch's");
  const int32_t nq_all = rq->n_req;
  // requests: grouped by locus, in locus order
  P.req_locus.resize((size_t)nq_all);
  std::vector<int32_t> req_begin(nl + 1, 0);
  {
    size_t l = 0;
    const int32_t n_pooled = nl ? b->read_off[nl] : 0;
    for (int32_t k = 0; k < nq_all; k++){
      const int32_t pr = rq->req_read[k];
      if (pr < 0 || pr >= n_pooled) return fail("hipstr_post_census: req_read outside the pooled reads");
      while (l < nl && pr >= b->read_off[l+1]){ l++; req_begin[l] = k; }
      if (pr < b->read_off[l]) return fail("hipstr_post_census: requests must be grouped by locus, in locus order");
      P.req_locus[k] = (int32_t)l;
    }
    for (l++; l <= nl; l++) req_begin[l] = nq_all;
    if (nq_all && tr){
      if (tr->str_seq_off[0] < 0) return fail("hipstr_post_census: str_seq_off must not be negative");
      for (int32_t k = 0; k < nq_all; k++) if (tr->str_seq_off[k+1] < tr->str_seq_off[k]) return fail("hipstr_post_census: str_seq_off must not decrease");
      if (tr->str_seq_off[nq_all] > 0 && !tr->str_seq) return fail("hipstr_post_census: trace output without str_seq");
    }
  }
  P.loci.resize(nl); P.read_samp.assign((size_t)R.n_reads, 0); P.o1_off.push_back(0);
  size_t ui = 0; int rend = 0; int64_t opt = 0;
  for (size_t l = 0; l < nl; l++){
    hs_census_locus_t& L = P.loci[l]; memset(&L, 0, sizeof L);
    const int A = pd->n_alleles[l];
    if ((int64_t)b->hap_off[l+1] - b->hap_off[l] != A) return fail("hipstr_post_census: pooled->hap_off disagrees with the posterior batch's allele counts");
    L.n_alleles = A; L.hap_begin = b->hap_off[l]; L.haploid = pd->haploid[l] ? 1 : 0;
    L.read_begin = rend; L.samp_begin = ui < R.units.size() ? R.units[ui].samp_index : (int32_t)R.n_samp; L.n_samp = pd->n_samples[l];
    for (int s = 0; s < pd->n_samples[l]; s++, ui++){
      const hs_post_unit_t& u = R.units[ui];
      if (s == 0){ L.read_begin = u.read_begin; L.ll_off = u.ll_off; }
      rend = u.read_begin + u.n_reads;
      for (int r = u.read_begin; r < rend; r++) P.read_samp[r] = u.samp_index;
    }
    L.n_reads = rend - L.read_begin;
    L.req_begin = req_begin[l]; L.n_req = req_begin[l+1] - req_begin[l];
    L.blk_start = b->blk_start[3*l + 1]; L.blk_end = b->blk_end[3*l + 1];
    for (int k = 0; k < 3; k++){
      const int no = b->blk_nopts[3*l + k];
      if (no < 1) return fail("hipstr_post_census: a block without options");
      for (int o = 0; o < no; o++) if (b->opt_off[opt + o + 1] < b->opt_off[opt + o]) return fail("hipstr_post_census: opt_off must not decrease");
      L.opt_begin[k] = (int32_t)opt; L.n_opts[k] = no;
      if (k == 1){
        L.o1_begin = (int32_t)P.o1_off.size() - 1;
        for (int o = 0; o < no; o++){
          P.o1_seq.append(b->seq + b->opt_off[opt + o], (size_t)(b->opt_off[opt + o + 1] - b->opt_off[opt + o]));
          P.o1_off.push_back((int32_t)P.o1_seq.size());
        }
      }
      opt += no;
      if (rq->hap_to_allele[k])
        for (int h = 0; h < A; h++){
          const int32_t v = rq->hap_to_allele[k][L.hap_begin + h];
          if (v < 0 || v >= no) return fail("hipstr_post_census: hap_to_allele entry outside its block's options");
        }
    }
    if ((int64_t)L.n_samp*std::max(L.n_req, 1) >= INT32_MAX) return fail("hipstr_post_census: too many (sample, request) pairs in a locus");
    for (int r = L.read_begin; r < rend; r++){
      const int32_t k = rq->read_req[r];
      if (k < -1 || k >= nq_all) return fail("hipstr_post_census: read_req outside [-1, n_req)");
      if (k < 0) continue;
      if (P.req_locus[k] != (int32_t)l) return fail("hipstr_post_census: a read's request belongs to another locus");
      if (tr && rq->seed[r] >= 0 && tr->aln_start[k] < L.blk_start && tr->aln_stop[k] > L.blk_end && tr->stutter_size[k] == HIPSTR_NO_STR_DATA)
        return fail("hipstr_post_census: a spanning request without STR data (AlignmentTrace::stutter_size asserts)");
    }
    const int route = hs_census_route(L.n_req, L.n_reads);
    if (route == HS_CENSUS_ROUTE_GLOBAL){ L.ws_off = P.ws_ints; P.ws_ints += hs_census_ws_stride(L.n_req, L.n_reads); }
    P.list[route].push_back((int32_t)l);
  }
  P.n_opts = opt; P.n_haps = nl ? b->hap_off[nl] : 0;
  return 0;
}
}  // namespace

namespace {
// hipstr_post_census (td == NULL: the five trace fields are rq->trace's host arrays) and hipstr_post_census_dev (dev: they lie in td): one
// plan, the same launches, one copy home.  Only the source of the five fields and of the candidates' bytes differs.
int census_call(hipstr_post_dev_t* pd, const hipstr_census_request_t* rq, const hipstr_trace_dev* td, bool dev, hipstr_census_out_t* out){
  if (dev && rq && rq->trace) return fail("hipstr_post_census_dev: rq->trace must be NULL (the trace fields are the handle's)");
  if (!pd || !rq || !out || (dev && !td) || !rq->pooled || !rq->seed || !rq->read_req) return fail("null argument");
  const hipstr_batch_t* b = rq->pooled;
  if (b->n_loci < 0 || (b->n_loci && (!b->blk_start || !b->blk_end || !b->blk_nopts || !b->opt_off || !b->seq || !b->hap_off || !b->read_off))) return fail("null argument");
  if (rq->n_req < 0) return fail("hipstr_post_census: negative n_req");
  if (dev && rq->n_req != td->n_req) return fail("hipstr_post_census_dev: rq->n_req differs from the trace handle's");
  if (rq->n_req && (!rq->req_read || (dev ? (!td->scal[3] || !td->scal[4] || !td->scal[0] || !td->off[1])
                                          : (!rq->trace || !rq->trace->aln_start || !rq->trace->aln_stop || !rq->trace->stutter_size || !rq->trace->str_seq_off))))
    return fail("hipstr_post_census: trace output without aln_start / aln_stop / stutter_size / str_seq_off");
  const bool any_h2a = rq->hap_to_allele[0] || rq->hap_to_allele[1] || rq->hap_to_allele[2];
  if (!out->cand_off || !out->cand_seq_off || !out->new_n_haps || !out->n_spanning || !out->n_span_stutter || out->cap_cand < 0 || out->cap_chars < 0 ||
      (out->cap_cand && !out->cand_req) || (out->cap_chars && !out->cand_seq) || (any_h2a && !out->called) || (rq->hap_to_allele[1] && !out->spanned))
    return fail("null output array");
  if (rq->min_reads < 0 || !(rq->min_frac >= 0)) return fail("hipstr_post_census: min_reads and min_frac must not be negative");
  if (!pd->launched) return fail("hipstr_post_census needs the posteriors: call hipstr_post_launch first");
  PostRun& R = pd->R;
  if (dev && td->ctx != R.ctx) return fail("hipstr_post_census_dev: the trace handle lives on another device than the posteriors");
  const hipstr_trace_out_t* tr = dev ? NULL : rq->trace;
  CensusPlan P;
  if (census_plan(pd, rq, tr, P)) return 1;
  const size_t nl = P.loci.size(), n = (size_t)R.n_reads, ns = (size_t)R.n_samp, nq = (size_t)rq->n_req, no = (size_t)P.n_opts, nh = (size_t)P.n_haps;
  if (bind(R.ctx)) return 1;
  Ctx* ctx = R.ctx;
  const size_t cap = std::min((size_t)out->cap_cand, nq);                 // (a request makes at most one candidate)

  hipstr::HostArena ar;
  const size_t o_loci = ar.add(P.loci.data(), nl*sizeof(hs_census_locus_t)),
               o_list[3] = { ar.add(P.list[0].data(), P.list[0].size()*4), ar.add(P.list[1].data(), P.list[1].size()*4), ar.add(P.list[2].data(), P.list[2].size()*4) },
               o_seed = ar.add(rq->seed, n*4), o_rreq = ar.add(rq->read_req, n*4), o_rsamp = ar.add(P.read_samp.data(), n*4),
               // the five trace fields travel only when they are the host's
               o_start = ar.add(nq && tr ? tr->aln_start : NULL, tr ? nq*4 : 0), o_stop = ar.add(nq && tr ? tr->aln_stop : NULL, tr ? nq*4 : 0),
               o_stut = ar.add(nq && tr ? tr->stutter_size : NULL, tr ? nq*4 : 0), o_soff = ar.add(nq && tr ? tr->str_seq_off : NULL, nq && tr ? (nq + 1)*4 : 0),
               o_sseq = ar.add(nq && tr ? tr->str_seq : NULL, nq && tr ? (size_t)tr->str_seq_off[nq] : 0),
               o_rloc = ar.add(P.req_locus.data(), nq*4), o_o1off = ar.add(P.o1_off.data(), P.o1_off.size()*4), o_o1seq = ar.add(P.o1_seq.data(), P.o1_seq.size()),
               o_h2a[3] = { ar.add(rq->hap_to_allele[0], rq->hap_to_allele[0] ? nh*4 : 0), ar.add(rq->hap_to_allele[1], rq->hap_to_allele[1] ? nh*4 : 0),
                            ar.add(rq->hap_to_allele[2], rq->hap_to_allele[2] ? nh*4 : 0) },
               o_unc = ar.add(rq->sample_uncallable, rq->sample_uncallable ? ns : 0);
  hs_census_dev_t h; memset(&h, 0, sizeof h);
  const size_t o_args = ar.add(&h, sizeof h);
  if (ar.reserve(ctx)) return 1;
  // results, back to back (one copy home), then what stays on the device
  hipstr::ResultBlocks B;
  const size_t r_coff = B.take((nl + 1)*4), r_creq = B.take(cap*4), r_nsp = B.take(ns*4), r_nss = B.take(ns*4), r_called = B.take(no), r_spanned = B.take(no);
  // (resident trace fields: what the check found, the candidates' offsets and byte count; their bytes last: only those in use come home)
  const size_t dev_chars = dev ? (size_t)std::min<int64_t>(out->cap_chars, td->totals[1]) : 0;
  const size_t r_check = dev ? B.take(8) : 0, r_cchars = dev ? B.take(8) : 0, r_csoff = dev ? B.take((cap + 1)*4) : 0;
  B.end_results();
  const size_t r_cseq = dev ? B.take(dev_chars) : 0;
  const size_t d_count = B.take(nl*4), d_has = B.take(ns), d_rank = B.take(nq*4), d_ws = B.take((size_t)P.ws_ints*4);
  if (B.reserve(ctx, R.stream)) return 1;
  h.loci = ar.at<hs_census_locus_t>(o_loci);
  for (int k = 0; k < 3; k++){
    h.list[k] = ar.at<int32_t>(o_list[k]); h.n_list[k] = (int32_t)P.list[k].size();
    h.h2a[k] = rq->hap_to_allele[k] ? ar.at<int32_t>(o_h2a[k]) : NULL;
  }
  h.n_loci = (int32_t)nl; h.n_req = (int32_t)nq; h.cap_cand = (int32_t)cap;
  h.log_aln_probs = R.h.log_aln_probs; h.log_p1 = R.h.log_p1; h.log_p2 = R.h.log_p2; h.map_gt = R.h.map_gt;
  h.seed = ar.at<int32_t>(o_seed); h.read_req = ar.at<int32_t>(o_rreq); h.read_samp = ar.at<int32_t>(o_rsamp);
  if (dev){
    h.aln_start = td->scal[3]; h.aln_stop = td->scal[4]; h.stutter_size = td->scal[0]; h.str_seq_off = td->off[1]; h.str_seq = td->arr[1];
    h.check = B.dev<int32_t>(r_check); h.n_reads = (int32_t)n; h.check_offsets = td->checked ? 0 : 1; h.str_total = td->totals[1];
    h.cand_seq_off = B.dev<int32_t>(r_csoff); h.cand_seq = B.dev<char>(r_cseq); h.cand_chars = B.dev<int64_t>(r_cchars); h.cap_chars = out->cap_chars;
  } else {
    h.aln_start = ar.at<int32_t>(o_start); h.aln_stop = ar.at<int32_t>(o_stop); h.stutter_size = ar.at<int32_t>(o_stut);
    h.str_seq_off = ar.at<int32_t>(o_soff); h.str_seq = ar.at<char>(o_sseq);
  }
  h.req_locus = ar.at<int32_t>(o_rloc);
  h.o1_off = ar.at<int32_t>(o_o1off); h.o1_seq = ar.at<char>(o_o1seq);
  h.uncallable = rq->sample_uncallable ? ar.at<uint8_t>(o_unc) : NULL;
  h.min_reads = rq->min_reads == 0 ? 2 : rq->min_reads; h.min_frac = rq->min_frac == 0 ? 0.15 : rq->min_frac;      // seq_stutter_genotyper.cpp:869
  h.cand_off = B.dev<int32_t>(r_coff); h.cand_req = B.dev<int32_t>(r_creq);
  h.n_spanning = B.dev<int32_t>(r_nsp); h.n_span_stutter = B.dev<int32_t>(r_nss);
  h.called = B.dev<uint8_t>(r_called); h.spanned = B.dev<uint8_t>(r_spanned);
  h.cand_count = B.dev<int32_t>(d_count); h.has_read = B.dev<uint8_t>(d_has); h.req_rank = B.dev<int32_t>(d_rank); h.ws = B.dev<int32_t>(d_ws);
  if (pd->foreign_stream) HS_HIP(hipDeviceSynchronize());          // the posterior kernel may still be running on a stream of the caller's
  hipStream_t st = R.stream;
  if (rm_order_behind(R.h.log_aln_probs, st)) return 1;
  if (ar.send(st)) return 1;
  const hs_census_dev_t* d_args = ar.at<hs_census_dev_t>(o_args);
  if (dev && nq){
    // the checks of the trace's values; offsets that are not known to ascend are judged before any kernel follows them into str_seq
    hipLaunchKernelGGL(hs_census_check_kernel, dim3(1), dim3(HS_CENSUS_THREADS), 0, st, d_args);
    if (h.check_offsets){
      HS_HIP(hipGetLastError());
      if (B.fetch(r_check, 8)) return 1;             // the check word alone, ahead of the results
      const int bad = *B.host<int32_t>(r_check);
      if (bad & HS_CENSUS_BAD_NEGATIVE) return fail("hipstr_post_census: str_seq_off must not be negative");
      if (bad & HS_CENSUS_BAD_DECREASE) return fail("hipstr_post_census: str_seq_off must not decrease");
    }
  }
  HS_HIP(hipMemsetAsync(B.dev<char>(r_nsp), 0, (dev ? r_check : B.res) - r_nsp, st));          // the counts and the marks
  HS_HIP(hipMemsetAsync(B.dev<char>(d_count), 0, d_rank - d_count, st));            // candidates per locus, the samples' flags
  if (!P.list[0].empty()) hipLaunchKernelGGL(hs_census_wave_kernel, dim3((unsigned)hs_census_workgroups(0, (int64_t)P.list[0].size())), dim3(HS_CENSUS_THREADS), 0, st, d_args);
  if (!P.list[1].empty()) hipLaunchKernelGGL(hs_census_lds_kernel, dim3((unsigned)P.list[1].size()), dim3(HS_CENSUS_THREADS), 0, st, d_args);
  if (!P.list[2].empty()) hipLaunchKernelGGL(hs_census_global_kernel, dim3((unsigned)P.list[2].size()), dim3(HS_CENSUS_THREADS), 0, st, d_args);
  hipLaunchKernelGGL(hs_census_scan_kernel, dim3(1), dim3(HS_CENSUS_THREADS), 0, st, d_args);
  if (nq) hipLaunchKernelGGL(hs_census_emit_kernel, dim3((unsigned)((nq + HS_CENSUS_THREADS - 1)/HS_CENSUS_THREADS)), dim3(HS_CENSUS_THREADS), 0, st, d_args);
  if (dev && nq) hipLaunchKernelGGL(hs_census_gather_kernel, dim3(1), dim3(HS_CENSUS_THREADS), 0, st, d_args);
  HS_HIP(hipGetLastError());
  if (B.fetch()) return 1;
  const int32_t* coff = B.host<int32_t>(r_coff);
  const int32_t* creq = B.host<int32_t>(r_creq);
  if (dev && nq && (*B.host<int32_t>(r_check) & HS_CENSUS_BAD_NO_STR))
    return fail("hipstr_post_census: a spanning request without STR data (AlignmentTrace::stutter_size asserts)");
  memcpy(out->cand_off, coff, (nl + 1)*4);
  const int32_t n_cand = coff[nl];
  if (n_cand > out->cap_cand){ fail("candidate arrays too small: cand_off[n_loci] holds the number needed"); return 3; }
  int64_t chars = 0;
  if (dev) chars = nq ? *B.host<int64_t>(r_cchars) : 0;
  else for (int32_t k = 0; k < n_cand; k++) chars += tr->str_seq_off[creq[k] + 1] - tr->str_seq_off[creq[k]];
  if (chars > out->cap_chars){ fail("candidate string pool too small: cap_chars of str_seq_off[n_req] always holds it"); return 3; }
  // the candidates' strings are the caller's own bytes: copied here from trace->str_seq in the order the device fixed
  if (dev){
    // ... or gathered on the device in that order: the bytes in use come home in a copy of their own
    out->cand_seq_off[0] = 0;
    if (nq) memcpy(out->cand_seq_off, B.host<char>(r_csoff), ((size_t)n_cand + 1)*4);
    if (n_cand) memcpy(out->cand_req, creq, (size_t)n_cand*4);
    if (hipstr::fetch_to_host(ctx, st, out->cand_seq, B.dev<char>(r_cseq), (size_t)chars)) return 1;
  } else {
  out->cand_seq_off[0] = 0;
  for (int32_t k = 0; k < n_cand; k++){
    const int32_t q = creq[k], len = tr->str_seq_off[q+1] - tr->str_seq_off[q];
    out->cand_req[k] = q;
    if (len) memcpy(out->cand_seq + out->cand_seq_off[k], tr->str_seq + tr->str_seq_off[q], (size_t)len);
    out->cand_seq_off[k+1] = out->cand_seq_off[k] + len;
  }
  }
  for (size_t l = 0; l < nl; l++){                                                // :583-584, integer division as written
    const int64_t n1 = P.loci[l].n_opts[1];
    out->new_n_haps[l] = (int64_t)P.loci[l].n_alleles / n1 * (n1 + (coff[l+1] - coff[l]));
  }
  memcpy(out->n_spanning, B.host<char>(r_nsp), ns*4); memcpy(out->n_span_stutter, B.host<char>(r_nss), ns*4);
  for (size_t l = 0; l < nl; l++)
    for (int k = 0; k < 3; k++)
      if (rq->hap_to_allele[k]){
        const hs_census_locus_t& L = P.loci[l];
        memcpy(out->called + L.opt_begin[k], B.host<char>(r_called) + L.opt_begin[k], (size_t)L.n_opts[k]);
        if (k == 1) memcpy(out->spanned + L.opt_begin[k], B.host<char>(r_spanned) + L.opt_begin[k], (size_t)L.n_opts[k]);
      }
  return 0;
}
}  // namespace

int hipstr_post_census(hipstr_post_dev_t* pd, const hipstr_census_request_t* rq, hipstr_census_out_t* out){
  return census_call(pd, rq, NULL, false, out);
}
int hipstr_post_census_dev(hipstr_post_dev_t* pd, const hipstr_census_request_t* rq, const hipstr_trace_dev_t* td, hipstr_census_out_t* out){
  return census_call(pd, rq, td, true, out);
}

#ifndef HIPSTR_NO_DEBUG_ABI
// Diagnostics (host only): the route hipstr_post_census gives a locus of n_req requests and n_reads un-pooled reads (census_layout.h).
int hipstr_debug_census_plan(int64_t n_req, int64_t n_reads, int64_t out[10]){
  if (!out || n_req < 0 || n_reads < 0) return fail("bad argument");
  const int route = hs_census_route(n_req, n_reads);
  out[0] = route; out[1] = hs_census_ws_ints(n_req, n_reads);
  out[2] = route == HS_CENSUS_ROUTE_WAVE ? 64 : HS_CENSUS_THREADS; out[3] = route == HS_CENSUS_ROUTE_WAVE ? HS_CENSUS_THREADS/64 : 1;
  out[4] = route == HS_CENSUS_ROUTE_GLOBAL ? hs_census_ws_stride(n_req, n_reads) : 0;
  out[5] = HS_CENSUS_WAVE_REQS; out[6] = HS_CENSUS_WAVE_READS; out[7] = HS_CENSUS_LDS_INTS; out[8] = HS_CENSUS_THREADS; out[9] = HS_CENSUS_REQ_INTS;
  return 0;
}
#endif

extern "C++" {
namespace {
// What both forms of hipstr_assign_trace_stats check, before anything is written or launched.  trace: the host's or the resident result;
// scalars: its five arrays are there.  each_read(l, r, so): what a form adds for a read that passed (nonzero: refused); so, ao, vo: the
// samples, haplotypes and variants in front of locus l, and of all loci on return.
template <typename F>
int trace_stats_check(const hipstr_post_batch_t* pb, const int32_t* read_req, const void* trace, bool scalars, const int32_t* best_hap, const int32_t* hap_to_allele,
                      const int32_t* allele_bp_diff, const int32_t* n_variants, const int32_t* region_start, const int32_t* region_stop,
                      const int32_t* n_stutter, const int32_t* n_flank_indel, const int32_t* ml_bp, int64_t& so, int64_t& ao, int64_t& vo, F each_read){
  if (!pb || !read_req || !trace || !best_hap || !hap_to_allele || !allele_bp_diff || !n_variants || !region_start || !region_stop ||
      !n_stutter || !n_flank_indel || !ml_bp) return fail("null argument");
  if (!scalars) return fail("trace output without stutter_size / flank_ins / flank_del / aln_start / aln_stop");
  if (pb->n_loci < 0 || (pb->n_loci && (!pb->n_alleles || !pb->n_samples || !pb->read_off || !pb->sample_label))) return fail("null argument");
  so = ao = vo = 0;
  for (int l = 0; l < pb->n_loci; l++){
    const int A = pb->n_alleles[l], S = pb->n_samples[l], V = n_variants[l];
    if (A < 1 || S < 0 || V < 1 || pb->read_off[l+1] < pb->read_off[l]) return fail("inconsistent locus tables");
    for (int a = 0; a < A; a++) if (hap_to_allele[ao + a] < 0 || hap_to_allele[ao + a] >= V) return fail("hap_to_allele entry out of range");
    for (int r = pb->read_off[l]; r < pb->read_off[l+1]; r++){
      if (pb->sample_label[r] < 0 || pb->sample_label[r] >= S) return fail("sample_label out of range");
      if (read_req[r] >= 0 && (best_hap[r] < 0 || best_hap[r] >= A)) return fail("best_hap out of range for a read with a request");
      if (each_read(l, r, so)) return 1;
    }
    so += S; ao += A; vo += V;
  }
  return 0;
}
}  // namespace
}  // extern "C++"

// Host only: the read counts that need the tracebacks (seq_stutter_genotyper.cpp:1124-1127, 1150-1154).
int hipstr_assign_trace_stats(const hipstr_post_batch_t* pb, const int32_t* read_req, const hipstr_trace_out_t* tr,
                              const int32_t* best_hap, const int32_t* hap_to_allele, const int32_t* allele_bp_diff,
                              const int32_t* n_variants, const int32_t* region_start, const int32_t* region_stop,
                              int32_t* n_stutter, int32_t* n_flank_indel, int32_t* ml_bp){
  int64_t so = 0, ao = 0, vo = 0;
  if (trace_stats_check(pb, read_req, tr, tr && tr->stutter_size && tr->flank_ins && tr->flank_del && tr->aln_start && tr->aln_stop, best_hap, hap_to_allele,
                        allele_bp_diff, n_variants, region_start, region_stop, n_stutter, n_flank_indel, ml_bp, so, ao, vo, [](int, int, int64_t){ return 0; })) return 1;
  const int n_reads = pb->n_loci ? pb->read_off[pb->n_loci] : 0;
  for (int64_t s = 0; s < so; s++){ n_stutter[s] = 0; n_flank_indel[s] = 0; }
  for (int r = 0; r < n_reads; r++) ml_bp[r] = HIPSTR_NO_ML_BP;
  so = ao = vo = 0;
  for (int l = 0; l < pb->n_loci; l++){
    const int start_bound = region_start[l] > 4 ? region_start[l] - 4 : 0;
    for (int r = pb->read_off[l]; r < pb->read_off[l+1]; r++){
      const int q = read_req[r];
      if (q < 0) continue;                                 // skipped read (:1080)
      const int64_t s = so + pb->sample_label[r];
      const bool str_data = tr->stutter_size[q] != HIPSTR_NO_STR_DATA;
      if (str_data && tr->stutter_size[q] != 0) n_stutter[s]++;                        // has_stutter(), AlignmentTraceback.h:79-85
      if (tr->flank_ins[q] != 0 || tr->flank_del[q] != 0) n_flank_indel[s]++;          // :1126
      if (tr->aln_start[q] < start_bound && tr->aln_stop[q] > region_stop[l] + 4)      // :1152-1154
        ml_bp[r] = allele_bp_diff[vo + hap_to_allele[ao + best_hap[r]]] + (str_data ? tr->stutter_size[q] : 0);
    }
    so += pb->n_samples[l]; ao += pb->n_alleles[l]; vo += n_variants[l];
  }
  return 0;
}

static_assert(HS_TSTAT_NO_STR_DATA == HIPSTR_NO_STR_DATA && HS_CENSUS_NO_STR_DATA == HIPSTR_NO_STR_DATA && HS_TSTAT_NO_ML_BP == HIPSTR_NO_ML_BP,
              "the kernels' copies of the public constants");
// The same counts with the five scalars read from a resident traceback result, on its device (assign.hip: hs_trace_stats_kernel).  The
// host's table checks are the same function's, before any launch; the units are the runs of reads of one sample.
int hipstr_assign_trace_stats_dev(const hipstr_post_batch_t* pb, const int32_t* read_req, const hipstr_trace_dev_t* td,
                                  const int32_t* best_hap, const int32_t* hap_to_allele, const int32_t* allele_bp_diff,
                                  const int32_t* n_variants, const int32_t* region_start, const int32_t* region_stop,
                                  int32_t* n_stutter, int32_t* n_flank_indel, int32_t* ml_bp){
  std::vector<hs_tstat_unit_t> units;
  int64_t so = 0, ao = 0, vo = 0;
  if (trace_stats_check(pb, read_req, td, td && td->scal[0] && td->scal[1] && td->scal[2] && td->scal[3] && td->scal[4], best_hap, hap_to_allele,
                        allele_bp_diff, n_variants, region_start, region_stop, n_stutter, n_flank_indel, ml_bp, so, ao, vo, [&](int l, int r, int64_t so_l){
        if (read_req[r] >= td->n_req) return fail("read_req outside the trace handle's requests");
        if (r > pb->read_off[l] && pb->sample_label[r] == pb->sample_label[r-1]) units.back().n_reads++;
        else units.push_back(hs_tstat_unit_t{r, 1, (int32_t)(so_l + pb->sample_label[r]), l});
        return 0;
      })) return 1;
  std::vector<hs_tstat_locus_t> loci((size_t)pb->n_loci);
  for (int64_t l = 0, a = 0, v = 0; l < pb->n_loci; a += pb->n_alleles[l], v += n_variants[l], l++){
    hs_tstat_locus_t& L = loci[l];
    L.hap_begin = a; L.var_begin = v;
    L.start_bound = region_start[l] > 4 ? region_start[l] - 4 : 0; L.stop_bound = region_stop[l] + 4;
  }
  const size_t n = pb->n_loci ? (size_t)pb->read_off[pb->n_loci] : 0, ns = (size_t)so;
  if (units.empty()){                                      // no read: nothing for the device to do
    for (size_t s = 0; s < ns; s++){ n_stutter[s] = 0; n_flank_indel[s] = 0; }
    return 0;
  }
  Ctx* ctx = td->ctx;
  if (bind(ctx)) return 1;
  hipStream_t st = td->stream;
  hipstr::HostArena ar;
  const size_t o_units = ar.add(units.data(), units.size()*sizeof(hs_tstat_unit_t)), o_loci = ar.add(loci.data(), loci.size()*sizeof(hs_tstat_locus_t)),
               o_rreq = ar.add(read_req, n*4), o_best = ar.add(best_hap, n*4), o_h2a = ar.add(hap_to_allele, (size_t)ao*4), o_bp = ar.add(allele_bp_diff, (size_t)vo*4);
  hs_tstat_dev_t h; memset(&h, 0, sizeof h);
  const size_t o_args = ar.add(&h, sizeof h);
  if (ar.reserve(ctx)) return 1;
  hipstr::ResultBlocks B;
  const size_t r_st = B.take(ns*4), r_fi = B.take(ns*4), r_ml = B.take(n*4);
  B.end_results();                                         // all of it comes home
  if (B.reserve(ctx, st)) return 1;
  h.units = ar.at<hs_tstat_unit_t>(o_units); h.loci = ar.at<hs_tstat_locus_t>(o_loci); h.n_units = (int32_t)units.size();
  h.read_req = ar.at<int32_t>(o_rreq); h.best_hap = ar.at<int32_t>(o_best); h.hap_to_allele = ar.at<int32_t>(o_h2a); h.allele_bp_diff = ar.at<int32_t>(o_bp);
  h.stutter_size = td->scal[0]; h.flank_ins = td->scal[1]; h.flank_del = td->scal[2]; h.aln_start = td->scal[3]; h.aln_stop = td->scal[4];
  h.n_stutter = B.dev<int32_t>(r_st); h.n_flank_indel = B.dev<int32_t>(r_fi); h.ml_bp = B.dev<int32_t>(r_ml);
  if (ar.send(st)) return 1;
  const hs_tstat_dev_t* d_args = ar.at<hs_tstat_dev_t>(o_args);
  HS_HIP(hipMemsetAsync(B.dev<char>(r_st), 0, r_ml - r_st, st));                       // the samples' counts
  hipLaunchKernelGGL(hs_trace_stats_kernel, dim3((unsigned)hs_assign_workgroups((int64_t)units.size(), 1)), dim3(HS_ASSIGN_THREADS), 0, st, d_args);
  HS_HIP(hipGetLastError());
  if (B.fetch()) return 1;
  memcpy(n_stutter, B.host<char>(r_st), ns*4); memcpy(n_flank_indel, B.host<char>(r_fi), ns*4); memcpy(ml_bp, B.host<char>(r_ml), n*4);
  return 0;
}

// ----------------------------------------------------------------------------- resident read x haplotype matrix
// log_aln_probs_ of a batch of loci kept on the device between the rounds of SeqStutterGenotyper::genotype (hipstr_hmm.h: hipstr_rm_*).
// The layout (reads per locus, pool of every read, mates) is fixed at creation: the mate groups and each read's pool go to the device once;
// the haplotype counts change with hipstr_rm_remap, and with them the wavefront list of the scatter (readmat_layout.h).
struct hipstr_read_matrix {
  Ctx* ctx = NULL;
  hipStream_t stream = NULL;                   // the creating thread's stream: every kernel and copy of the matrix is queued here
  int32_t n_loci = 0; int64_t n_reads = 0, n_ll = 0, n_groups = 0, n_waves = 0;
  std::vector<int32_t> n_alleles, read_off, pool_index, pool_max, group_off;      // pool_max: largest pool_index of a locus (-1: no reads)
  std::vector<int64_t> mat_off;
  hipstr::ScratchBufs blocks;                  // the five blocks below: back when the matrix goes, behind `stream`
  double* d_ll = NULL; int32_t* d_seeds = NULL;
  char* d_static = NULL; size_t o_groups = 0, o_pool = 0, o_waves = 0;            // mate groups | pool_index | wavefront list, device
  char* d_stage = NULL; char* pin_stage = NULL; size_t stage_bytes = 0;           // what a scatter sends: locus records | copy_read | realign_hap flags
  hipEvent_t ev_stage = NULL, ev_done = NULL;  // the staging block's last copy has left it / the matrix' last kernel has run
  bool stage_sent = false;
  ~hipstr_read_matrix(){ if (ctx){ ctx->put_event(ev_stage, false); ctx->put_event(ev_done, false); bind(ctx); } }
};

namespace {
std::mutex g_rm_m;
std::map<const double*, hipstr_read_matrix*> g_rm;       // by device pointer of the matrix (hipstr_rm_dev_log_aln_probs)

int rm_order_behind(const double* ll, hipStream_t st){
  std::lock_guard<std::mutex> g(g_rm_m);
  auto it = g_rm.find(ll);
  if (it == g_rm.end() || it->second->stream == st) return 0;
  HS_HIP(hipStreamWaitEvent(st, it->second->ev_done, 0));
  return 0;
}

int ilog2(int w){ int k = 0; while ((1 << k) < w) k++; return k; }

// the wavefront list of a launch whose locus l has count[l] work items of A[l] columns
void rm_waves(const std::vector<int32_t>& A, const int64_t* count, std::vector<hs_rm_wave_t>& out){
  out.clear();
  for (size_t l = 0; l < A.size(); l++){
    const int per = hs_rm_items_per_wave(A[l]);
    for (int64_t f = 0; f < count[l]; f += per) out.push_back(hs_rm_wave_t{(int32_t)l, (int32_t)f});
  }
}

size_t rm_stage_bytes(const hipstr_read_matrix* rm){
  size_t sumA = 0; for (int32_t a : rm->n_alleles) sumA += (size_t)a;
  return (((size_t)rm->n_loci*sizeof(hs_rm_locus_t) + 255) & ~(size_t)255) + (((size_t)rm->n_reads + 255) & ~(size_t)255) + sumA + 256;
}

// host arrays -> device through a pinned block of the cache, on the matrix' stream; returns when the copy has landed (a copy that failed
// may still be in flight: its block goes back with the matrix)
int rm_send(hipstr_read_matrix* rm, void* dst, const void* src, size_t bytes){
  if (!bytes) return 0;
  char* pin;
  if (rm->blocks.alloc_pinned(&pin, bytes)) return 1;
  memcpy(pin, src, bytes);
  if (hipMemcpyAsync(dst, pin, bytes, hipMemcpyHostToDevice, rm->stream) != hipSuccess || hipstr::wait_stream(rm->stream) != hipSuccess)
    return fail("host-to-device copy failed");
  rm->blocks.release(pin);
  return 0;
}

void rm_release(hipstr_read_matrix* rm){
  if (!rm) return;
  { std::lock_guard<std::mutex> g(g_rm_m); if (rm->d_ll) g_rm.erase(rm->d_ll); }
  delete rm;
}
}  // namespace

hipstr_read_matrix_t* hipstr_rm_create(const hipstr_read_layout_t* lay, const double* init_ll, const int32_t* init_seeds){
  if (!lay || lay->n_loci < 0 || (lay->n_loci > 0 && (!lay->n_alleles || !lay->read_off))){ g_err = "null argument or negative locus count"; return NULL; }
  const int nl = lay->n_loci;
  if (nl > 0 && lay->read_off[0] != 0){ g_err = "read_off must start at 0"; return NULL; }
  int64_t n_ll = 0;
  for (int l = 0; l < nl; l++){
    if (lay->n_alleles[l] < 1 || lay->n_alleles[l] + 1 >= 10000){ g_err = "allele count out of range"; return NULL; }
    if (lay->read_off[l+1] < lay->read_off[l]){ g_err = "read_off must be ascending (negative read count)"; return NULL; }
    n_ll += (int64_t)(lay->read_off[l+1] - lay->read_off[l])*lay->n_alleles[l];
  }
  const int64_t R = nl ? lay->read_off[nl] : 0;
  if (R > 0 && !lay->pool_index){ g_err = "null pool_index"; return NULL; }
  std::vector<uint32_t> groups; std::vector<int32_t> group_off(nl + 1, 0), pool_max(nl, -1);
  for (int l = 0; l < nl; l++){
    const int r0 = lay->read_off[l], r1 = lay->read_off[l+1];
    for (int i = r0; i < r1; i++){
      if (lay->pool_index[i] < 0){ g_err = "pool_index must not be negative"; return NULL; }
      pool_max[l] = std::max(pool_max[l], lay->pool_index[i]);
      if (lay->second_mate && lay->second_mate[i]){
        if (i == r0){ g_err = "second_mate set on the first read of a locus: its first mate would be a read of another locus"; return NULL; }
        if (lay->second_mate[i-1]){ g_err = "second_mate set on two consecutive reads"; return NULL; }
      }
    }
    for (int i = r0; i < r1; ){        // a read alone, or a first mate with the second mate behind it (seq_stutter_genotyper.cpp:555-556)
      const bool pair = lay->second_mate && i + 1 < r1 && lay->second_mate[i+1];
      groups.push_back((uint32_t)i | (pair ? HS_RM_PAIR : 0u));
      i += pair ? 2 : 1;
    }
    group_off[l+1] = (int32_t)groups.size();
  }
  Ctx* ctx = hipstr::api_current_ctx();
  if (!ctx) return NULL;
  hipstr_read_matrix_t* rm = new hipstr_read_matrix_t();
  rm->ctx = ctx; rm->stream = thread_stream(ctx);
  rm->n_loci = nl; rm->n_reads = R; rm->n_ll = n_ll; rm->n_groups = (int64_t)groups.size();
  rm->n_alleles.assign(lay->n_alleles, lay->n_alleles + nl); rm->read_off.assign(lay->read_off, lay->read_off + (nl ? nl + 1 : 0));
  if (!nl) rm->read_off.assign(1, 0);
  rm->pool_index.assign(lay->pool_index, lay->pool_index + R); rm->pool_max.swap(pool_max); rm->group_off.swap(group_off);
  rm->mat_off.assign(nl + 1, 0);
  for (int l = 0; l < nl; l++) rm->mat_off[l+1] = rm->mat_off[l] + (int64_t)(rm->read_off[l+1] - rm->read_off[l])*rm->n_alleles[l];
  std::vector<hs_rm_wave_t> waves;
  { std::vector<int64_t> cnt(nl); for (int l = 0; l < nl; l++) cnt[l] = rm->group_off[l+1] - rm->group_off[l]; rm_waves(rm->n_alleles, cnt.data(), waves); }
  rm->n_waves = (int64_t)waves.size();
  // mate groups | pool_index | wavefront list (room for one wavefront per group: what any later haplotype count can need)
  const size_t G = groups.size();
  rm->o_groups = 0; rm->o_pool = (G*4 + 255) & ~(size_t)255; rm->o_waves = (rm->o_pool + (size_t)R*4 + 255) & ~(size_t)255;
  const size_t static_bytes = rm->o_waves + G*sizeof(hs_rm_wave_t) + 256;
  rm->stage_bytes = rm_stage_bytes(rm);
  rm->blocks.ctx = ctx; rm->blocks.runs_on(rm->stream);
  bool ok = !(rm->blocks.alloc(&rm->d_ll, (size_t)n_ll) || rm->blocks.alloc(&rm->d_seeds, (size_t)R) || rm->blocks.alloc(&rm->d_static, static_bytes) ||
              rm->blocks.alloc(&rm->d_stage, rm->stage_bytes) || rm->blocks.alloc_pinned(&rm->pin_stage, rm->stage_bytes));
  rm->ev_stage = ctx->get_event(false); rm->ev_done = ctx->get_event(false);
  if (ok && (!rm->ev_stage || !rm->ev_done)){ ok = false; g_err = "hipEventCreate failed"; }
  if (ok){
    std::vector<char> img(static_bytes, 0);
    if (G) memcpy(img.data() + rm->o_groups, groups.data(), G*4);
    if (R) memcpy(img.data() + rm->o_pool, rm->pool_index.data(), (size_t)R*4);
    if (!waves.empty()) memcpy(img.data() + rm->o_waves, waves.data(), waves.size()*sizeof(hs_rm_wave_t));
    ok = rm_send(rm, rm->d_static, img.data(), static_bytes) == 0;
  }
  hipError_t e = hipSuccess;
  if (ok && n_ll){
    if (init_ll) e = hipMemcpyAsync(rm->d_ll, init_ll, (size_t)n_ll*sizeof(double), hipMemcpyHostToDevice, rm->stream);
    else {          // columns nobody has aligned yet (seq_stutter_genotyper.cpp:374)
      const unsigned wgs = (unsigned)std::min<int64_t>((n_ll + HS_RM_THREADS - 1)/HS_RM_THREADS, 2048);
      hipLaunchKernelGGL(hs_rm_fill_kernel, dim3(wgs), dim3(HS_RM_THREADS), 0, rm->stream, rm->d_ll, n_ll, HS_RM_UNALIGNED);
      e = hipGetLastError();
    }
  }
  if (ok && e == hipSuccess && R)
    e = init_seeds ? hipMemcpyAsync(rm->d_seeds, init_seeds, (size_t)R*sizeof(int32_t), hipMemcpyHostToDevice, rm->stream)
                   : hipMemsetAsync(rm->d_seeds, 0xff, (size_t)R*sizeof(int32_t), rm->stream);         // -1
  if (ok && e == hipSuccess) e = hipEventRecord(rm->ev_done, rm->stream);
  if (ok && e == hipSuccess) e = hipstr::wait_stream(rm->stream);      // the sources are the caller's arrays: done with them before returning
  if (ok && e != hipSuccess){ ok = false; g_err = std::string("hipstr_rm_create: ") + hipGetErrorString(e); }
  if (!ok){ rm_release(rm); return NULL; }
  { std::lock_guard<std::mutex> g(g_rm_m); g_rm[rm->d_ll] = rm; }
  return rm;
}

int hipstr_rm_scatter(hipstr_read_matrix_t* rm, hipstr_dev_batch_t* dev, const uint8_t* copy_read){
  if (!rm || !dev) return fail("null argument");
  if (rm->ctx != dev->ctx) return fail("the matrix and the batch belong to different devices");
  if (!dev->aligned) return fail("hipstr_rm_scatter needs a forward pass: call hipstr_hmm_align on the batch first");
  const hipstr::Prepared& P = dev->prep;
  static_assert(sizeof(hs_read_t) == 16, "hs_rm_scatter_kernel reads the seed as the third dword of a 16-byte record");
  if ((int64_t)P.loci.size() != rm->n_loci) return fail("n_loci of the matrix disagrees with the batch");
  bool all_pools = true;
  for (int l = 0; l < rm->n_loci; l++){
    const hs_locus_t& loc = P.loci[l];
    if (loc.n_alleles != rm->n_alleles[l]) return fail("n_alleles of locus " + std::to_string(l) + " disagrees with the batch");
    if (rm->pool_max[l] >= loc.n_reads) return fail("pool_index outside the pooled reads of locus " + std::to_string(l));
  }
  for (uint8_t f : P.realign_read) if (!f){ all_pools = false; break; }
  if (!all_pools)      // the reference would copy a row process_reads never wrote (seq_stutter_genotyper.cpp:526-542)
    for (int l = 0; l < rm->n_loci; l++)
      for (int i = rm->read_off[l]; i < rm->read_off[l+1]; i++)
        if ((!copy_read || copy_read[i]) && !P.realign_read[P.loci[l].read_begin + rm->pool_index[i]])
          return fail("copy_read set for read " + std::to_string(i) + " whose pool was not realigned");
  if (bind(rm->ctx)) return 1;
  Ctx* ctx = rm->ctx;
  hipStream_t st = rm->stream;
  // ---- what this scatter sends: locus records | copy_read | realign_hap flags of the loci with a partial mask
  if (rm->stage_sent) HS_HIP(hipEventSynchronize(rm->ev_stage));      // the previous scatter's copy has left the pinned block
  const size_t o_copy = ((size_t)rm->n_loci*sizeof(hs_rm_locus_t) + 255) & ~(size_t)255, o_mask = o_copy + (((size_t)rm->n_reads + 255) & ~(size_t)255);
  hs_rm_locus_t* lr = (hs_rm_locus_t*)rm->pin_stage;
  size_t mask_used = 0;
  for (int l = 0; l < rm->n_loci; l++){
    const hs_locus_t& loc = P.loci[l];
    hs_rm_locus_t& o = lr[l];
    o.mat_off = rm->mat_off[l]; o.src_off = loc.out_off; o.n_alleles = loc.n_alleles; o.lanes_log2 = ilog2(hs_rm_item_lanes(loc.n_alleles));
    o.read_begin = rm->read_off[l]; o.pool_begin = loc.read_begin; o.group_begin = rm->group_off[l]; o.n_groups = rm->group_off[l+1] - rm->group_off[l];
    o.mask_off = -1; o.pad = 0;
    if (loc.n_re != loc.n_alleles){
      o.mask_off = (int32_t)mask_used;
      memcpy(rm->pin_stage + o_mask + mask_used, P.realign_hap.data() + loc.hap_begin, (size_t)loc.n_alleles);
      mask_used += (size_t)loc.n_alleles;
    }
  }
  if (copy_read && rm->n_reads) memcpy(rm->pin_stage + o_copy, copy_read, (size_t)rm->n_reads);
  // ---- behind the batch's last pass
  if (dev->foreign_stream) HS_HIP(hipDeviceSynchronize());            // a pass was launched on a stream of the caller's
  else if (dev->stream != st){
    hipEvent_t ev = ctx->get_event(false);
    if (!ev) return fail("hipEventCreate failed");
    const bool ok = hipEventRecord(ev, dev->stream) == hipSuccess && hipStreamWaitEvent(st, ev, 0) == hipSuccess;
    ctx->put_event(ev, false);          // (its wait is queued: the event may be recorded again by its next user)
    if (!ok) return fail("hipEventRecord / hipStreamWaitEvent failed");
  }
  HS_HIP(hipMemcpyAsync(rm->d_stage, rm->pin_stage, o_mask + mask_used + 1, hipMemcpyHostToDevice, st));
  HS_HIP(hipEventRecord(rm->ev_stage, st));
  rm->stage_sent = true;
  if (rm->n_waves > 0){
    hs_rm_scatter_t a; memset(&a, 0, sizeof a);
    a.waves = (const hs_rm_wave_t*)(rm->d_static + rm->o_waves); a.loci = (const hs_rm_locus_t*)rm->d_stage;
    a.groups = (const uint32_t*)(rm->d_static + rm->o_groups); a.pool_index = (const int32_t*)(rm->d_static + rm->o_pool);
    a.copy_read = copy_read ? (const uint8_t*)(rm->d_stage + o_copy) : NULL; a.mask = (const uint8_t*)(rm->d_stage + o_mask);
    a.src = dev->h.aln_probs; a.pool_reads = (const int32_t*)dev->h.reads; a.ll = rm->d_ll; a.seeds = rm->d_seeds; a.n_waves = rm->n_waves;
    hipLaunchKernelGGL(hs_rm_scatter_kernel, dim3((unsigned)((rm->n_waves + HS_RM_THREADS/64 - 1)/(HS_RM_THREADS/64))), dim3(HS_RM_THREADS), 0, st, a);
    HS_HIP(hipGetLastError());
  }
  HS_HIP(hipEventRecord(rm->ev_done, st));
  // the batch's blocks are read by a kernel on the matrix' stream: hipstr_hmm_free waits for the batch's own stream only
  if (!dev->foreign_stream && dev->stream != st) HS_HIP(hipStreamWaitEvent(dev->stream, rm->ev_done, 0));
  return 0;
}

int hipstr_rm_remap(hipstr_read_matrix_t* rm, const int32_t* new_n_alleles, const int32_t* allele_mapping){
  if (!rm || (rm->n_loci > 0 && (!new_n_alleles || !allele_mapping))) return fail("null argument");
  const int nl = rm->n_loci;
  std::vector<int32_t> newA(new_n_alleles, new_n_alleles + nl), inv;
  std::vector<hs_rm_remap_locus_t> loci(nl);
  std::vector<int64_t> new_off(nl + 1, 0), rows(nl);
  size_t old_base = 0;
  for (int l = 0; l < nl; l++){
    if (newA[l] < 1 || newA[l] + 1 >= 10000) return fail("allele count out of range");
    const size_t ib = inv.size();
    inv.resize(ib + (size_t)newA[l], -1);
    for (int j = 0; j < rm->n_alleles[l]; j++){
      const int m = allele_mapping[old_base + j];
      if (m == -1) continue;
      if (m < 0 || m >= newA[l]) return fail("allele_mapping entry out of range at locus " + std::to_string(l));
      if (inv[ib + m] != -1) return fail("two old columns mapped to one new column at locus " + std::to_string(l));
      inv[ib + m] = j;
    }
    rows[l] = rm->read_off[l+1] - rm->read_off[l];
    new_off[l+1] = new_off[l] + rows[l]*newA[l];
    hs_rm_remap_locus_t& o = loci[l];
    o.old_off = rm->mat_off[l]; o.new_off = new_off[l]; o.old_A = rm->n_alleles[l]; o.new_A = newA[l];
    o.lanes_log2 = ilog2(hs_rm_item_lanes(newA[l])); o.n_reads = (int32_t)rows[l]; o.inv_off = (int32_t)ib; o.pad = 0;
    old_base += (size_t)rm->n_alleles[l];
  }
  if (bind(rm->ctx)) return 1;
  Ctx* ctx = rm->ctx;
  hipStream_t st = rm->stream;
  std::vector<hs_rm_wave_t> waves, swaves;          // of this launch (rows), of the scatters to come (mate groups under the new counts)
  rm_waves(newA, rows.data(), waves);
  { std::vector<int64_t> cnt(nl); for (int l = 0; l < nl; l++) cnt[l] = rm->group_off[l+1] - rm->group_off[l]; rm_waves(newA, cnt.data(), swaves); }
  const int64_t n_new = new_off[nl];
  double* nll;
  if (rm->blocks.alloc(&nll, (size_t)n_new)) return 1;
  bool ok;
  {
    hipstr::HostArena ar;             // (waits for the stream when it goes)
    const size_t o_loci = ar.add(loci.data(), loci.size()*sizeof(hs_rm_remap_locus_t)), o_inv = ar.add(inv.data(), inv.size()*4),
                 o_w = ar.add(waves.data(), waves.size()*sizeof(hs_rm_wave_t)), o_sw = ar.add(swaves.data(), swaves.size()*sizeof(hs_rm_wave_t));
    ok = ar.reserve(ctx) == 0 && ar.send(st) == 0;
    if (ok && !waves.empty()){
      hs_rm_remap_t a; memset(&a, 0, sizeof a);
      a.waves = ar.at<hs_rm_wave_t>(o_w); a.loci = ar.at<hs_rm_remap_locus_t>(o_loci); a.inv = ar.at<int32_t>(o_inv);
      a.old_ll = rm->d_ll; a.new_ll = nll; a.n_waves = (int64_t)waves.size();
      hipLaunchKernelGGL(hs_rm_remap_kernel, dim3((unsigned)((waves.size() + HS_RM_THREADS/64 - 1)/(HS_RM_THREADS/64))), dim3(HS_RM_THREADS), 0, st, a);
      ok = hipGetLastError() == hipSuccess;
    }
    if (ok && !swaves.empty())
      ok = hipMemcpyAsync(rm->d_static + rm->o_waves, ar.at<char>(o_sw), swaves.size()*sizeof(hs_rm_wave_t), hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (ok) ok = hipEventRecord(rm->ev_done, st) == hipSuccess && hipstr::wait_stream(st) == hipSuccess;
  }
  if (!ok){ rm->blocks.release(nll); return g_err.empty() ? fail("hipstr_rm_remap: launch failed") : 1; }
  { std::lock_guard<std::mutex> g(g_rm_m); g_rm.erase(rm->d_ll); g_rm[nll] = rm; }
  rm->blocks.replace(&rm->d_ll, nll);    // (the stream is idle: nothing reads the old matrix any more)
  rm->n_ll = n_new; rm->n_alleles.swap(newA); rm->mat_off.swap(new_off); rm->n_waves = (int64_t)swaves.size();
  const size_t need = rm_stage_bytes(rm);
  if (need > rm->stage_bytes){           // more haplotype flags than the staging blocks hold
    char *d, *p;
    if (rm->blocks.alloc(&d, need) || rm->blocks.alloc_pinned(&p, need)) return 1;      // (a block already taken goes back with the matrix)
    rm->blocks.replace(&rm->d_stage, d); rm->blocks.replace(&rm->pin_stage, p);
    rm->stage_bytes = need; rm->stage_sent = false;
  }
  return 0;
}

const double* hipstr_rm_dev_log_aln_probs(hipstr_read_matrix_t* rm){ return rm ? rm->d_ll : NULL; }

int hipstr_rm_fetch(hipstr_read_matrix_t* rm, double* ll, int32_t* seeds){
  if (!rm) return fail("null argument");
  if (bind(rm->ctx)) return 1;
  HS_HIP(hipstr::wait_stream(rm->stream));
  if (ll && fetch_array(rm->ctx, rm->stream, ll, rm->d_ll, (size_t)rm->n_ll*sizeof(double))) return 1;
  if (seeds && fetch_array(rm->ctx, rm->stream, seeds, rm->d_seeds, (size_t)rm->n_reads*sizeof(int32_t))) return 1;
  return 0;
}

void hipstr_rm_free(hipstr_read_matrix_t* rm){ rm_release(rm); }

#ifndef HIPSTR_NO_DEBUG_ABI
// Diagnostics (host only): the route the matrix kernels give a locus of n_alleles haplotypes and n_items work items (mate groups of a
// scatter, rows of a remap), from readmat_layout.h's functions.
int hipstr_debug_rm_plan(int32_t n_alleles, int64_t n_items, int64_t out[5]){
  if (!out || n_alleles < 1 || n_items < 0) return fail("bad argument");
  out[0] = n_alleles > HS_RM_NARROW_MAX ? 1 : 0; out[1] = hs_rm_item_lanes(n_alleles); out[2] = hs_rm_items_per_wave(n_alleles);
  out[3] = hs_rm_waves(n_alleles, n_items); out[4] = hs_rm_column_steps(n_alleles);
  return 0;
}
#endif

int hipstr_post_run(const hipstr_post_batch_t* pb, const double* dev_log_aln_probs,
                    double* log_post, double* sample_total_ll, int32_t* map_gt, double* locus_total_ll){
  hipstr::ApiTimer prof_t(hipstr::PB_POST_RUN);
  if (!pb || !log_post || !sample_total_ll || !map_gt || !locus_total_ll) return fail("null argument");
  hipstr_post_dev_t* pd = hipstr_post_upload(pb, dev_log_aln_probs);
  if (!pd) return 1;
  int rc = hipstr_post_launch(pd, NULL);
  if (!rc) rc = hipstr_post_fetch(pd, log_post, sample_total_ll, map_gt, locus_total_ll);
  hipstr_post_free(pd);
  return rc;
}

}  // extern "C"
