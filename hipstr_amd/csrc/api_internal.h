// api_internal.h — state of api.hip shared with the other translation units of libhipstr_hmm.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include "block_pieces.h"

namespace hipstr {

// One context per device the process uses: constant tables, the library's stream, and two block caches (device memory and pinned
// host memory).  hipstr_hmm_init(d) makes device d the calling thread's current context; every object created afterwards
// (device batches, posterior runs) belongs to that context and may be used from any thread.
struct Ctx;
Ctx* api_current_ctx();                       // the calling thread's context; initialises device 0 on first use; NULL + last error on failure
int  api_bind(Ctx* ctx);                      // hipSetDevice(ctx's device) for the calling thread

struct ApiTables {                 // device copies of HostTables, owned by the context
  const double *int_log, *qual_correct, *qual_error, *m2m, *m2i;
  hipStream_t stream;
  Ctx* ctx;
};
int api_device_tables(ApiTables* t);          // tables of the calling thread's current context; 1 + hipstr_last_error() on failure
int api_fail(const std::string& message);     // records hipstr_last_error(); returns 1
// a HIP call of an entry point: on failure "<the call as written>: <the driver's words>" is the last error and the function returns 1
#define HS_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return ::hipstr::api_fail(std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// Cached blocks: a freed block goes back to its context's free list instead of hipFree / hipHostFree (both synchronise the
// device and cost 0.1-10 ms); a request is served from the list when a block of at most 1.25x the size is there.
// Waiting for a stream from a host thread.  hipStreamSynchronize / hipEventSynchronize spin at 100 % of a core on this stack (tools/wait_probe.hip),
// which is the fastest way to learn that a 0.2 ms call is done as long as every waiting thread has a core of its own — and the worst one
// when the caller runs more host threads than cores to keep the device busy (the reference's genotype() over the adapter: 16 threads on 16
// cores 755 loci/s, 64 threads 291): the waiters keep the cores from the threads that have host work.  wait_stream polls hipStreamQuery and
// yields the core between polls (sched_yield returns at once when nothing else is runnable: the single-thread latency stays what it was),
// sleeping 50 us per poll once a wait has lasted 2 ms.  HIPSTR_WAIT=spin: the driver's own wait; =sleep: sleep from the first poll.
hipError_t wait_stream(hipStream_t st);
hipError_t wait_event(hipEvent_t ev);         // the same policy for an event the caller recorded

void* dev_alloc(Ctx* ctx, size_t bytes);      // NULL + last error on failure
void  dev_free(Ctx* ctx, void* p);
void* pin_alloc(Ctx* ctx, size_t bytes);
void  pin_free(Ctx* ctx, void* p);


// Host arrays that travel together: packed into ONE pinned block and sent with ONE asynchronous copy (a synchronous hipMemcpy from
// pageable memory costs 10-20 us each; the traceback and Needleman-Wunsch calls of a locus had ten of them).  add() (the list of
// pieces and its arithmetic: HostPieces, block_pieces.h) returns a piece's offset; after send() the piece sits at dev + offset.  Both blocks go back to the context's caches when the arena dies; the caches serve other
// host threads, so the arena first waits for the stream its copy went to (an error path may leave while the copy is in flight; on the
// normal path the results were fetched already and the wait costs a few microseconds).
struct HostArena : HostPieces {
  Ctx* ctx = NULL; char* pin = NULL; char* dev = NULL;
  hipStream_t sent_on = NULL; bool sent = false;
  ~HostArena(){ if (ctx){ if (sent) hipStreamSynchronize(sent_on); if (pin) pin_free(ctx, pin); if (dev) dev_free(ctx, dev); } }
  int reserve(Ctx* c){        // blocks only (the caller still has pointers into `dev` to fill in before the pieces are packed)
    ctx = c; pin = (char*)pin_alloc(ctx, total ? total : 256); dev = (char*)dev_alloc(ctx, total ? total : 256);
    return (pin && dev) ? 0 : 1;
  }
  int send(hipStream_t st){   // pack and copy
    pack(pin);
    sent_on = st; sent = true;
    return (total && hipMemcpyAsync(dev, pin, total, hipMemcpyHostToDevice, st) != hipSuccess) ? api_fail("hipMemcpyAsync (host to device) failed") : 0;
  }
  template <typename T> T* at(size_t off) const { return (T*)(dev + off); }
};

// ---- blocks of the caches on the result side.  One rule, stated in the destructors below and nowhere else: the caches serve other host
// threads, so a block goes back only after the stream that may still be working on it has been waited for, whichever way the call leaves.
// On the normal path the results were fetched through wait_stream already and that wait costs a few microseconds; hipStreamSynchronize
// is the backstop of the error paths.

// Cache blocks with one owner — the device scratch arrays of a chunked call (traceback, Needleman-Wunsch), the blocks of a
// resident handle (a posterior run, a read matrix): one cache block each, device or pinned, all of them back when the owner goes, behind
// every stream it was told about.  release() gives one back earlier — the caller has waited for whatever used it — and replace() puts a
// new block in its place; an owner that holds nothing any more has nothing to wait for.
struct ScratchBufs {
  std::vector<void*> p, pin;        // device blocks, pinned blocks
  Ctx* ctx = NULL;                  // taken on first use: blocks come from (and return to) the context's cache, no hipMalloc / hipFree per call
  hipStream_t streams[3] = {NULL, NULL, NULL}; int n_streams = 0;
  void runs_on(hipStream_t st){ for (int i = 0; i < n_streams; i++) if (streams[i] == st) return; if (n_streams < 3) streams[n_streams++] = st; }
  ScratchBufs(){}
  ScratchBufs(const ScratchBufs&) = delete;
  ~ScratchBufs(){
    if (!ctx || (p.empty() && pin.empty())) return;
    for (int i = 0; i < n_streams; i++) hipStreamSynchronize(streams[i]);
    for (void* x : p) dev_free(ctx, x);
    for (void* x : pin) pin_free(ctx, x);
  }
  template <typename T> int alloc(T** out, size_t count, bool pinned = false){
    *out = NULL;
    if (!ctx) ctx = api_current_ctx();
    if (!ctx) return 1;
    const size_t bytes = (count ? count : 1)*sizeof(T);
    *out = (T*)(pinned ? pin_alloc(ctx, bytes) : dev_alloc(ctx, bytes));
    if (!*out) return 1;
    (pinned ? pin : p).push_back(*out);
    return 0;
  }
  template <typename T> int alloc_pinned(T** out, size_t count){ return alloc(out, count, true); }
  template <typename T> int put(T** out, const T* src, size_t count){
    if (alloc(out, count)) return 1;
    if (count) HS_HIP(hipMemcpy(*out, src, count*sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
  void release(void* x){
    auto it = std::find(p.begin(), p.end(), x);
    if (it != p.end()){ p.erase(it); dev_free(ctx, x); return; }
    it = std::find(pin.begin(), pin.end(), x);
    if (it != pin.end()){ pin.erase(it); pin_free(ctx, x); }
  }
  template <typename T> void replace(T** slot, T* fresh){ release(*slot); *slot = fresh; }
};

// The results of a one-shot call: the pieces that come home first, back to back (take, then end_results), then what stays on the device;
// one device block of the whole size and one pinned block of the results' size; one copy home.  Lives as long as the host reads the
// pinned pieces.
struct ResultBlocks : BlockPieces {
  Ctx* ctx = NULL; hipStream_t st = NULL; char* d = NULL; char* h = NULL;
  ResultBlocks(){}
  ResultBlocks(const ResultBlocks&) = delete;
  ~ResultBlocks(){ if (d || h) hipStreamSynchronize(st); if (d) dev_free(ctx, d); if (h) pin_free(ctx, h); }
  int reserve(Ctx* c, hipStream_t s){        // after the last take(): the blocks; everything the call queues on them goes to s
    ctx = c; st = s;
    d = (char*)dev_alloc(ctx, tot);
    if (!d) return 1;
    h = (char*)pin_alloc(ctx, res);
    return h ? 0 : 1;
  }
  template <typename T> T* dev(size_t off) const { return (T*)(d + off); }
  template <typename T> const T* host(size_t off) const { return (const T*)(h + off); }      // (a results' piece, after fetch)
  int fetch(size_t off, size_t bytes){       // part of the results home, at the same offset
    HS_HIP(hipMemcpyAsync(h + off, d + off, bytes, hipMemcpyDeviceToHost, st));
    HS_HIP(wait_stream(st));
    return 0;
  }
  int fetch(){ return fetch(0, res); }
};

// One chunk of a call that walks its loci in chunks (read pooling, allele generation): uploaded | workspace | results in one device block,
// the uploaded pieces packed in a pinned block, the results fetched into another.  `busy` from the first copy queued until the results are
// home: only then has the destructor a stream to wait for.  e0, e1: around the kernels, when the call is timed.
struct ChunkBlocks : BlockPieces {
  Ctx* ctx; hipStream_t st; char* dev = NULL; char* pin_up = NULL; char* pin_res = NULL; bool busy = false;
  hipEvent_t e0 = NULL, e1 = NULL;
  size_t up_bytes = 0, res0 = 0;             // where the uploaded pieces end and the results begin
  ChunkBlocks(Ctx* c, hipStream_t s) : ctx(c), st(s) {}
  ChunkBlocks(const ChunkBlocks&) = delete;
  ~ChunkBlocks(){
    if (busy) hipStreamSynchronize(st);
    if (dev) dev_free(ctx, dev);
    if (pin_up) pin_free(ctx, pin_up);
    if (pin_res) pin_free(ctx, pin_res);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
  }
  void end_upload(){ up_bytes = tot; }
  void begin_results(){ res0 = tot; }
  size_t res_bytes() const { return tot - res0; }
  int reserve(){
    dev = (char*)dev_alloc(ctx, tot);
    if (!dev) return 1;
    pin_up = (char*)pin_alloc(ctx, up_bytes);
    if (!pin_up) return 1;
    pin_res = (char*)pin_alloc(ctx, res_bytes());
    return pin_res ? 0 : 1;
  }
  template <typename T> T* up(size_t off) const { return (T*)(pin_up + off); }               // an uploaded piece, to be filled
  template <typename T> const T* host(size_t off) const { return (const T*)(pin_res + (off - res0)); }      // a results' piece, after fetch
  int upload(bool timing){                   // the uploaded pieces on their way, e0 behind them
    if (timing){ HS_HIP(hipEventCreate(&e0)); HS_HIP(hipEventCreate(&e1)); }
    busy = true;
    HS_HIP(hipMemcpyAsync(dev, pin_up, up_bytes, hipMemcpyHostToDevice, st));
    if (timing) HS_HIP(hipEventRecord(e0, st));
    return 0;
  }
  int fetch(bool timing, double* kernel_ms){ // e1 behind the kernels, the results home; the kernels' milliseconds are added when timed
    if (timing) HS_HIP(hipEventRecord(e1, st));
    HS_HIP(hipMemcpyAsync(pin_res, dev + res0, res_bytes(), hipMemcpyDeviceToHost, st));
    HS_HIP(wait_stream(st));
    busy = false;
    if (timing){ float ms = 0; HS_HIP(hipEventElapsedTime(&ms, e0, e1)); *kernel_ms += ms; }
    return 0;
  }
};
// the per-thread record of such a call (hipstr_debug_pool_last, hipstr_debug_hapgen_last): counts, and kernel ms | bytes up | bytes home | packing s
struct ChunkLast { int64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0}; double t[4] = {0, 0, 0, 0}; };
// a chunk's workspace in bytes: ws_mib when positive, else the variable `env` when it holds a positive number, else default_mib; at least
// 4 KiB, at most cap_bytes
inline int64_t chunk_budget(double ws_mib, const char* env, double default_mib, double cap_bytes){
  double mib = ws_mib > 0 ? ws_mib : default_mib;
  if (!(ws_mib > 0)) if (const char* e = getenv(env)){ const double v = atof(e); if (v > 0) mib = v; }
  return (int64_t)std::min(std::max(mib*1048576.0, 4096.0), cap_bytes);
}

// One device array into a (pageable) host array through a pinned block of the cache; returns when it has landed.  (The forward pass'
// large results: fetch_array, api.hip.)
inline int fetch_to_host(Ctx* ctx, hipStream_t st, void* dst, const void* src, size_t bytes){
  if (!bytes) return 0;
  char* p = (char*)pin_alloc(ctx, bytes);
  if (!p) return 1;
  const bool ok = hipMemcpyAsync(p, src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess && wait_stream(st) == hipSuccess;
  if (ok) memcpy(dst, p, bytes); else hipStreamSynchronize(st);
  pin_free(ctx, p);
  return ok ? 0 : api_fail("device-to-host copy failed");
}

// ---- where the host time of the entry points goes (hipstr_debug_api_profile, include/hipstr_hmm.h): wall-clock seconds and calls per
// bucket, summed over all threads while enabled.  Buckets nest: the indented ones are parts of the entry point above them.
enum ApiBucket { PB_PROCESS_READS, PB_PR_PREPARE, PB_PR_STAGE, PB_PR_UPLOAD_REST, PB_PR_LAUNCH, PB_PR_FETCH, PB_PR_FREE,
                 PB_TRACE, PB_TRACE_REPLAY, PB_POST_RUN, PB_POST_EXTRACT, PB_EM_TRAIN, PB_NW_ALIGN, PB_STREAM_SUBMIT, PB_STREAM_TAKE, PB_SEED_BASES,
                 PB_UP_BLOCKS, PB_UP_MEMCPY, PB_UP_EXPAND, PB_UP_EVENTS, PB_COUNT };        // (the last four: parts of "blocks + H2D enqueue")
bool api_profile_on();
void api_profile_add(int bucket, double seconds, int calls = 1);
struct ApiTimer {                  // adds its lifetime to a bucket
  int bucket; bool on; double t0;
  static double now();
  explicit ApiTimer(int b) : bucket(b), on(api_profile_on()), t0(on ? now() : 0.0) {}
  ~ApiTimer(){ if (on) api_profile_add(bucket, now() - t0); }
};

// ---- the pieces of hipstr_hmm_process_reads, split for pipelined use (stream.hip)
}  // namespace hipstr
struct hipstr_batch; struct hipstr_dev_batch;
namespace hipstr {
// reads_pinned: batch->bases / quals lie in pinned host memory that outlives the copy: they are sent from there, not through the staging block
hipstr_dev_batch* upload_on(Ctx* ctx, const hipstr_batch* batch, const int32_t* seed_base, hipStream_t copy_stream, hipStream_t compute_stream, bool reads_pinned = false);
int  fetch_begin(hipstr_dev_batch* dev, hipStream_t compute_stream, hipStream_t copy_stream);
int  fetch_poll(hipstr_dev_batch* dev);         // queues the copy back of a batch whose kernels are done (0 queued or nothing pending, 1 still running, -1 error)
int  results_wait(hipstr_dev_batch* dev);
double batch_prepare_seconds(const hipstr_dev_batch* dev);      // wall time of the batch's prepare_batch
// the reference's output contract for loci [l0, l1) of a batch whose results lie at `src` (NULL: where the batch's own copy back landed);
// aln_probs / seeds are based at locus l0, or at the batch's first locus when `whole`
void scatter_loci(const hipstr_dev_batch* dev, int l0, int l1, double* aln_probs, int32_t* seeds, const double* src = NULL, bool whole = false);
void free_landed(hipstr_dev_batch* dev, bool landed);
hipStream_t ctx_stream(Ctx* c);
int ctx_device(Ctx* c);
// the calling thread's second stream on c's device, for work beside its own stream (the forward pass' table expansion, the EM's
// allele-frequency scans): lives until the process ends; NULL + last error when it could not be made.  Whoever queues work on it joins
// that work into the stream of the call before the call returns.
hipStream_t ctx_aux_stream(Ctx* c);
// an untimed event of the context's pool (NULL + last error when the driver refuses a new one), and its way back
hipEvent_t event_get(Ctx* c);
void event_put(Ctx* c, hipEvent_t e);
// record.hip's constant table: `count` doubles written by `fill` and uploaded on the context's first request, the context's from then on
// (freed by hipstr_hmm_shutdown with its other tables); 1 + last error on failure
int ctx_record_table(Ctx* c, size_t count, void (*fill)(double*), const double** out);

}  // namespace hipstr

// ---- a resident traceback result (trace.hip: hipstr_hmm_trace_resident; read by hipstr_post_census_dev and hipstr_assign_trace_stats_dev
// in api.hip).  Every array is a piece of ONE block of the context's device cache, laid out by TraceDevLayout (trace.hip): the arrays of
// hipstr_trace_out_t, offsets with their leading 0, pools dense.  Read-only once the creating call has returned (it waits for its stream).
#define HS_TRACE_DEV_POOLS 7          // hap_aln, str_seq, flank_seq, indel, snp, cigar, aln_str: hipstr_trace_out_t's order
#define HS_TRACE_DEV_ARRAYS 10        // the pools' arrays: hap_aln, str_seq, flank_seq, indel_pos, indel_size, snp_pos, snp_base, cigar_op, cigar_len, aln_str
// the pool and the element size of every array, in that order: the one statement of it (trace.hip's host tables and trace_cache.hip's
// device tables are both initialised from these lists)
#define HS_TRACE_DEV_ARR_POOL_LIST {0, 1, 2, 3, 3, 4, 4, 5, 5, 6}
#define HS_TRACE_DEV_ARR_ESZ_LIST  {1, 1, 1, 4, 4, 4, 1, 1, 4, 1}
struct hipstr_trace_dev {
  hipstr::Ctx* ctx = NULL;
  hipStream_t stream = NULL;          // the creating thread's stream: fetches and the read counts are queued here
  int32_t n_req = 0;
  int64_t totals[HS_TRACE_DEV_POOLS] = {0, 0, 0, 0, 0, 0, 0};
  uint32_t groups = 0;                // HIPSTR_TRACE_F_* present (a handle of hipstr_debug_trace_dev_from_host may lack some)
  bool checked = false;               // made by hipstr_hmm_trace_resident: the offsets ascend by construction
  char* block = NULL;
  double* ll = NULL; int32_t* max_index = NULL;
  int32_t* scal[5] = {NULL, NULL, NULL, NULL, NULL};          // stutter_size, flank_ins, flank_del, aln_start, aln_stop
  int32_t* off[HS_TRACE_DEV_POOLS] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL};
  char* arr[HS_TRACE_DEV_ARRAYS] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL};
};
namespace hipstr {
// trace.hip, for trace_cache.hip: a handle of n requests and these pool totals on one fresh block of the context's device cache (groups and
// checked are the maker's to set; NULL + last error on failure), and its way back (the caller has waited for whatever used the block)
hipstr_trace_dev* trace_dev_make(Ctx* ctx, hipStream_t st, int32_t n, const int64_t tot[HS_TRACE_DEV_POOLS]);
void trace_dev_release(hipstr_trace_dev* td);
}  // namespace hipstr

// ---- what hipstr_em_train_dev (em_input.hip) needs of a posterior run (api.hip) and of the stutter EM (em.hip)
struct hs_post_unit_t; struct hipstr_post_dev; struct hipstr_em_batch;
namespace hipstr {
struct PostView {                    // a posterior run after hipstr_post_upload: what lies where (read-only)
  Ctx* ctx; hipStream_t stream;
  hipEvent_t ev_up;                  // recorded behind an asynchronous upload of the inputs, or NULL (they were waited for)
  const hs_post_unit_t* d_units;     // device: the (locus, sample) runs of reads, locus-major
  const hs_post_unit_t* units;       // the host's copy
  size_t n_units, n_loci;
  const double* log_p1, *log_p2;     // device, [n_reads]
  int n_reads; int64_t n_samp;
  const int32_t* n_samples;          // [n_loci]
  const uint8_t* haploid;            // [n_loci]
  const int32_t* n_alleles;          // [n_loci]
  const int32_t* map_gt;             // device, [2*n_samp]: the MAP pairs, once the run was launched
  bool launched, foreign_stream;     // hipstr_post_launch was called; on a stream of the caller's
  // per locus its reads [read_off[l], read_off[l+1]) and its units [unit_off[l], unit_off[l+1]), from the units (locus-major, one per sample)
  void locus_tables(std::vector<int32_t>& read_off, std::vector<int32_t>& unit_off) const;
};
void post_view(const hipstr_post_dev* pd, PostView* v);
int  api_tables_of(Ctx* c, ApiTables* t);     // api_device_tables for a given context (binds it)

int em_train_batch_on(const ApiTables& T, const hipstr_em_batch* eb, uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll);
// em_prepare's results for a batch (host only; its refusals): per locus the allele sizes (size_off), per read the allele index, per allele the initial log frequency
int em_prepare_host(const hipstr_em_batch* eb, std::vector<int32_t>& size_off, std::vector<int32_t>& sizes, std::vector<int32_t>& obs, std::vector<double>& log_freq);
struct EmLocusFacts { int32_t A, S, R, period, haploid, read_begin, bps_off; };
struct EmDeviceArrays { int32_t *bps, *obs, *sample_label, *weight; double *log_p1, *log_p2, *gtp; };      // the EM's seven per-read and per-allele arrays, device
// the EM loop on arrays prepared on the device: loci as em_prepare lays them out (reads_of_sample: [sum S], locus-major)
int em_train_prepared(const ApiTables& T, int n_loci, const EmLocusFacts* facts, const int32_t* reads_of_sample, const EmDeviceArrays& arr,
                      int max_iter, double min_abs_change, double min_frac_change, uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll);
}  // namespace hipstr
