// trace_cache.hip — the trace cache of SeqStutterGenotyper::retrace_alignments (seq_stutter_genotyper.cpp:805-841) for a batch of loci on
// gfx950, and the ragged gather of resident traceback records it is built on.  A round of genotype() asks for the (pool, haplotype) pairs
// its reads were assigned to; the reference traces only the pairs trace_cache_ does not hold yet and re-keys the cache when the allele set
// changes (:401-409).  Here the keys live in a host table (the request list is on the host anyway: the trace call's resolver runs there)
// and the records stay in the segments hipstr_hmm_trace_resident left them in, one per round that missed; what a round hands its
// consumers is ONE handle of the usual layout (api_internal.h: hipstr_trace_dev), gathered device-to-device:
//   hs_tc_lengths_kernel   a thread per output record: the length and the source position of each of its eight pieces, from the sources'
//                          offset arrays
//   hs_tc_scan_kernel      a wavefront per pool: running totals over the pieces (the flank pool has two per record), 64 at a time with a
//                          carried base; the pool's total comes home
//   hs_tc_copy_kernel      a wavefront per output record: its scalars, its offsets, and its pieces with the lanes along a piece's elements
// Only out_src / out_idx and the sources' pointer table (200 bytes a source) go up; only the 64-byte block of pool totals comes down,
// because the result's block is sized by it.  Every decision of size: trace_cache_layout.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "trace_cache_layout.h"
#include "api_internal.h"

static_assert(HS_TC_POOLS == HS_TRACE_DEV_POOLS && HS_TC_ARRAYS == HS_TRACE_DEV_ARRAYS, "the gather's view of a handle is the handle's");
static_assert(!hs_tc_pool_fits(HS_TC_TOTAL_WRAPPED), "a total the scan could not form is refused like one that is too large");
static_assert(HS_TC_TOTALS_BYTES >= (HS_TC_POOLS + 1)*8, "the totals and their pad word");
static_assert(hs_tc_pool_at(HS_TC_POOLS - 1, 1) + hs_tc_pool_pieces(HS_TC_POOLS - 1, 1) == HS_TC_PIECES, "eight pieces a record");

namespace {
// the pool and the element size of every array of a handle: api_internal.h's lists, the ones trace.hip lays a handle out by
__device__ __constant__ int TC_ARR_POOL_D[HS_TC_ARRAYS] = HS_TRACE_DEV_ARR_POOL_LIST;
__device__ __constant__ int TC_ARR_ESZ_D[HS_TC_ARRAYS]  = HS_TRACE_DEV_ARR_ESZ_LIST;

__device__ __forceinline__ int tc_uni(int v){ return __builtin_amdgcn_readfirstlane(v); }
// inclusive prefix sum over the wavefront, modulo 2^32; `wrapped` is set in a lane one of whose additions passed 2^32.  No addition
// wrapped in any lane <=> every lane's sum is exact: an addition's operands are exact unless an earlier one wrapped.
__device__ __forceinline__ uint32_t tc_wave_scan(uint32_t v, int lane, bool& wrapped){
  for (int o = 1; o < HS_TC_WAVE; o <<= 1){
    const uint32_t u = __shfl_up(v, o);
    if (lane >= o){ const uint32_t w = v + u; wrapped |= w < v; v = w; }
  }
  return v;
}
}  // namespace

extern "C" __global__ void __launch_bounds__(HS_TC_LEN_THREADS) hs_tc_lengths_kernel(hs_tc_dev_t d){
  const int64_t q = (int64_t)blockIdx.x*HS_TC_LEN_THREADS + threadIdx.x;
  const int64_t n = d.n_out;
  if (q >= n) return;
  const hs_tc_src_t& S = d.src[d.out_src[q]];
  const int64_t i = d.out_idx[q];
  for (int p = 0; p < HS_TC_POOLS; p++){
    const int64_t at = hs_tc_pool_at(p, n);
    if (p == HS_TC_FLANK_POOL){
      const int32_t a = S.off[p][2*i], b = S.off[p][2*i+1], c = S.off[p][2*i+2];
      d.from[at + 2*q] = a; d.lens[at + 2*q] = b - a;
      d.from[at + 2*q+1] = b; d.lens[at + 2*q+1] = c - b;
    } else {
      const int32_t a = S.off[p][i], b = S.off[p][i+1];
      d.from[at + q] = a; d.lens[at + q] = b - a;
    }
  }
}

extern "C" __global__ void __launch_bounds__(HS_TC_WAVE) hs_tc_scan_kernel(hs_tc_dev_t d){
  const int lane = threadIdx.x, p = blockIdx.x;
  const int64_t n = hs_tc_pool_pieces(p, d.n_out), at = hs_tc_pool_at(p, d.n_out);
  int64_t carry = 0;
  bool wrapped = false;
  for (int64_t i0 = 0; i0 < n; i0 += HS_TC_WAVE){
    const int64_t i = i0 + lane;
    const uint32_t v = i < n ? (uint32_t)d.lens[at + i] : 0u;
    const uint32_t s = tc_wave_scan(v, lane, wrapped);
    if (i < n) d.incl[at + i] = (int32_t)(carry + s);        // (exact wherever the total fits; where it does not, the host refuses the call)
    carry += (uint32_t)__builtin_amdgcn_readlane((int)s, HS_TC_WAVE - 1);
  }
  if (__any(wrapped)) carry = HS_TC_TOTAL_WRAPPED;           // 64 pieces summed past 2^32: the total is not known, and does not fit
  if (lane == 0){ d.totals[p] = carry; if (p == 0) d.totals[HS_TC_POOLS] = 0; }
}

extern "C" __global__ void __launch_bounds__(HS_TC_WAVE) hs_tc_copy_kernel(hs_tc_dev_t d, hs_tc_out_t o){
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.x, n = d.n_out;
  if (q == 0 && lane < HS_TC_POOLS) o.off[lane][0] = 0;       // the leading zeros (the empty gather launches this workgroup alone)
  if (q >= n) return;
  const hs_tc_src_t& S = d.src[tc_uni(d.out_src[q])];
  const int64_t i = tc_uni(d.out_idx[q]);
  if (lane == 0) o.ll[q] = S.ll[i];
  else if (lane == 1) o.max_index[q] = S.max_index[i];
  else if (lane < 7) o.scal[lane-2][q] = S.scal[lane-2][i];
  for (int a = 0; a < HS_TC_ARRAYS; a++){
    const int p = TC_ARR_POOL_D[a], esz = TC_ARR_ESZ_D[a];
    const int n_pc = p == HS_TC_FLANK_POOL ? 2 : 1;
    for (int f = 0; f < n_pc; f++){
      const int64_t pc = hs_tc_pool_at(p, n) + n_pc*q + f;
      const int len = tc_uni(d.lens[pc]), from = tc_uni(d.from[pc]), end = tc_uni(d.incl[pc]);
      const int64_t to = (int64_t)end - len;
      if (len < 0 || to < 0 || end > o.totals[p]) continue;    // cannot happen for sources whose offsets ascend: a piece is never written outside its pool
      if (esz == 1){
        const char* s = S.arr[a] + from; char* t = o.arr[a] + to;
        for (int k = lane; k < len; k += HS_TC_WAVE) t[k] = s[k];
      } else {
        const int32_t* s = (const int32_t*)S.arr[a] + from; int32_t* t = (int32_t*)o.arr[a] + to;
        for (int k = lane; k < len; k += HS_TC_WAVE) t[k] = s[k];
      }
    }
  }
  if (lane < HS_TC_PIECES){                                    // the record's offsets: off[p][piece + 1]
    int p = lane < HS_TC_FLANK_POOL ? lane : (lane <= HS_TC_FLANK_POOL + 1 ? HS_TC_FLANK_POOL : lane - 1);
    const int f = lane == HS_TC_FLANK_POOL + 1 ? 1 : 0;
    const int n_pc = p == HS_TC_FLANK_POOL ? 2 : 1;
    o.off[p][n_pc*q + f + 1] = d.incl[hs_tc_pool_at(p, n) + n_pc*q + f];
  }
}

// ------------------------------------------------------------------ host side
namespace {
using hipstr::api_fail;

struct GatherLast { double kernel_ms = 0; int64_t bytes_up = 0, bytes_home = 0, n_out = 0; };
thread_local GatherLast t_gather_last;

struct TdGuard {                   // a handle under construction: back behind its stream unless released
  hipstr_trace_dev* t; hipStream_t st;
  ~TdGuard(){ if (t){ hipStreamSynchronize(st); hipstr::trace_dev_release(t); } }
  hipstr_trace_dev* release(){ hipstr_trace_dev* r = t; t = NULL; return r; }
};
struct PinGuard {
  hipstr::Ctx* ctx; hipStream_t st; char* p;
  ~PinGuard(){ if (p){ hipStreamSynchronize(st); hipstr::pin_free(ctx, p); } }
};
struct Events { hipEvent_t e[4] = {NULL, NULL, NULL, NULL}; ~Events(){ for (hipEvent_t x : e) if (x) hipEventDestroy(x); } };      // around the kernels of either half, when timed

// the gather proper: every argument has been checked
int gather_checked(hipstr::Ctx* ctx, int32_t n_src, const hipstr_trace_dev_t* const* src, int32_t n_out, const int32_t* out_src, const int32_t* out_idx,
                   hipstr_trace_dev_t** td){
  hipstr::ApiTables T;
  if (hipstr::api_tables_of(ctx, &T)) return 1;
  const hipStream_t st = T.stream;
  const bool timing = getenv("HIPSTR_TRACE_GATHER_TIMING") != NULL;
  const size_t n = (size_t)n_out;
  std::vector<hs_tc_src_t> tab((size_t)n_src);
  for (int s = 0; s < n_src; s++){
    const hipstr_trace_dev* h = src[s]; hs_tc_src_t& t = tab[s];
    t.ll = h->ll; t.max_index = h->max_index; t.n_req = h->n_req; t.pad = 0;
    for (int i = 0; i < 5; i++) t.scal[i] = h->scal[i];
    for (int p = 0; p < HS_TC_POOLS; p++) t.off[p] = h->off[p];
    for (int a = 0; a < HS_TC_ARRAYS; a++) t.arr[a] = h->arr[a];
  }
  hipstr::HostArena ar;                        // what goes up
  const size_t o_src = ar.add(tab.data(), tab.size()*sizeof(hs_tc_src_t)), o_os = ar.add(out_src, n*4), o_oi = ar.add(out_idx, n*4);
  hipstr::BlockPieces W;                       // the device's scratch, one block
  const size_t o_lens = W.take(n*HS_TC_PIECES*4), o_from = W.take(n*HS_TC_PIECES*4), o_incl = W.take(n*HS_TC_PIECES*4), o_tot = W.take(HS_TC_TOTALS_BYTES);
  hipstr::ScratchBufs scratch;
  scratch.ctx = ctx; scratch.runs_on(st);
  char* ws = NULL;
  if (ar.reserve(ctx) || scratch.alloc(&ws, W.tot) || ar.send(st)) return 1;
  hs_tc_dev_t d;
  d.src = ar.at<hs_tc_src_t>(o_src); d.out_src = ar.at<int32_t>(o_os); d.out_idx = ar.at<int32_t>(o_oi);
  d.lens = (int32_t*)(ws + o_lens); d.from = (int32_t*)(ws + o_from); d.incl = (int32_t*)(ws + o_incl); d.totals = (int64_t*)(ws + o_tot);
  d.n_out = n_out; d.n_src = n_src;
  Events ev;
  if (timing){ for (hipEvent_t& x : ev.e) HS_HIP(hipEventCreate(&x)); HS_HIP(hipEventRecord(ev.e[0], st)); }
  if (n_out > 0) hipLaunchKernelGGL(hs_tc_lengths_kernel, dim3((unsigned)hs_tc_len_workgroups(n_out)), dim3(HS_TC_LEN_THREADS), 0, st, d);
  hipLaunchKernelGGL(hs_tc_scan_kernel, dim3(HS_TC_POOLS), dim3(HS_TC_WAVE), 0, st, d);
  HS_HIP(hipGetLastError());
  if (timing) HS_HIP(hipEventRecord(ev.e[1], st));
  int64_t tot[HS_TC_POOLS + 1];
  {
    PinGuard tb{ctx, st, (char*)hipstr::pin_alloc(ctx, HS_TC_TOTALS_BYTES)};
    if (!tb.p) return api_fail("out of pinned host memory");
    HS_HIP(hipMemcpyAsync(tb.p, d.totals, HS_TC_TOTALS_BYTES, hipMemcpyDeviceToHost, st));
    HS_HIP(hipstr::wait_stream(st));
    memcpy(tot, tb.p, sizeof tot);
  }
  for (int p = 0; p < HS_TC_POOLS; p++)
    if (!hs_tc_pool_fits(tot[p])) return api_fail("too many requests for one call; split the request list");      // (the offsets are 32-bit)
  TdGuard g{hipstr::trace_dev_make(ctx, st, n_out, tot), st};
  if (!g.t) return 1;
  hs_tc_out_t o;
  o.ll = g.t->ll; o.max_index = g.t->max_index;
  for (int i = 0; i < 5; i++) o.scal[i] = g.t->scal[i];
  for (int p = 0; p < HS_TC_POOLS; p++){ o.off[p] = g.t->off[p]; o.totals[p] = tot[p]; }
  for (int a = 0; a < HS_TC_ARRAYS; a++) o.arr[a] = g.t->arr[a];
  if (timing) HS_HIP(hipEventRecord(ev.e[2], st));
  hipLaunchKernelGGL(hs_tc_copy_kernel, dim3((unsigned)hs_tc_copy_workgroups(n_out)), dim3(HS_TC_WAVE), 0, st, d, o);
  HS_HIP(hipGetLastError());
  if (timing) HS_HIP(hipEventRecord(ev.e[3], st));
  if (hipstr::wait_stream(st) != hipSuccess) return api_fail("hipstr_trace_dev_gather: the device failed");
  GatherLast& L = t_gather_last;
  L.kernel_ms = 0; L.bytes_up = (int64_t)(tab.size()*sizeof(hs_tc_src_t) + 2*n*4); L.bytes_home = HS_TC_TOTALS_BYTES; L.n_out = n_out;
  if (timing){ float a = 0, b = 0; HS_HIP(hipEventElapsedTime(&a, ev.e[0], ev.e[1])); HS_HIP(hipEventElapsedTime(&b, ev.e[2], ev.e[3])); L.kernel_ms = (double)a + b; }
  g.t->groups = HIPSTR_TRACE_F_ALL; g.t->checked = true;
  *td = g.release();
  return 0;
}

// what a gather refuses, in the order the header names it; the sources' common context (the calling thread's for none)
int gather_refusals(int32_t n_src, const hipstr_trace_dev_t* const* src, int32_t n_out, const int32_t* out_src, const int32_t* out_idx, hipstr::Ctx** ctx){
  if (n_src < 0 || n_out < 0) return api_fail("hipstr_trace_dev_gather: negative count");
  if ((n_src > 0 && !src) || (n_out > 0 && (!out_src || !out_idx))) return api_fail("null argument");
  for (int s = 0; s < n_src; s++) if (!src[s]) return api_fail("hipstr_trace_dev_gather: null source " + std::to_string(s));
  for (int s = 1; s < n_src; s++)
    if (src[s]->ctx != src[0]->ctx) return api_fail("hipstr_trace_dev_gather: the sources belong to different devices");
  for (int s = 0; s < n_src; s++)          // (a handle of hipstr_debug_trace_dev_from_host: its offsets were never checked either)
    if (src[s]->groups != HIPSTR_TRACE_F_ALL || !src[s]->checked)
      return api_fail("hipstr_trace_dev_gather: source " + std::to_string(s) + " lacks a group or was not made by the library (hipstr_debug_trace_dev_from_host)");
  for (int q = 0; q < n_out; q++){
    if (out_src[q] < 0 || out_src[q] >= n_src) return api_fail("hipstr_trace_dev_gather: out_src out of range at record " + std::to_string(q));
    if (out_idx[q] < 0 || out_idx[q] >= src[out_src[q]]->n_req) return api_fail("hipstr_trace_dev_gather: out_idx out of range at record " + std::to_string(q));
  }
  *ctx = n_src > 0 ? src[0]->ctx : hipstr::api_current_ctx();
  return *ctx ? 0 : 1;
}
}  // namespace

extern "C" int hipstr_trace_dev_gather(int32_t n_src, const hipstr_trace_dev_t* const* src, int32_t n_out, const int32_t* out_src, const int32_t* out_idx,
                                       hipstr_trace_dev_t** td){
  if (td) *td = NULL;
  if (!td) return api_fail("null argument");
  hipstr::Ctx* ctx = NULL;
  if (gather_refusals(n_src, src, n_out, out_src, out_idx, &ctx)) return 1;
  return gather_checked(ctx, n_src, src, n_out, out_src, out_idx, td);
}

// ------------------------------------------------------------------ the cache
struct hipstr_trace_cache {
  hipstr::Ctx* ctx = NULL;                           // of the thread that made the first call that needed the device
  int32_t n_loci = 0;
  std::vector<int32_t> pool_off, n_alleles;
  struct At { int32_t seg, idx; };
  std::vector<std::map<uint64_t, At>> keys;          // per locus: (pool << 32 | haplotype) -> the record; ordered as hipstr_trace_cache_entries lists them
  std::vector<hipstr_trace_dev*> segs;               // what the rounds that missed left, oldest first
  int64_t n_records = 0, n_live = 0;                 // records of all segments; keys
};

namespace {
int tc_bind(hipstr_trace_cache* tc){ if (!tc->ctx) tc->ctx = hipstr::api_current_ctx(); return tc->ctx ? 0 : 1; }
uint64_t tc_key(int32_t pool, int32_t hap){ return ((uint64_t)(uint32_t)pool << 32) | (uint32_t)hap; }
void tc_drop_segments(hipstr_trace_cache* tc){
  for (hipstr_trace_dev* s : tc->segs) hipstr_trace_dev_free(s);
  tc->segs.clear(); tc->n_records = 0;
}
void tc_stats(const hipstr_trace_cache* tc, int64_t hits, int64_t misses, int64_t inserted, hipstr_trace_cache_stats_t* st){
  if (!st) return;
  st->n_hits = hits; st->n_misses = misses; st->n_inserted = inserted;
  st->n_segments = (int64_t)tc->segs.size(); st->n_live = tc->n_live; st->n_dead = tc->n_records - tc->n_live;
}
// the live records in the order of hipstr_trace_cache_entries, as a gather's arguments
void tc_live(const hipstr_trace_cache* tc, std::vector<int32_t>& os, std::vector<int32_t>& oi){
  os.clear(); oi.clear();
  for (const auto& m : tc->keys) for (const auto& kv : m){ os.push_back(kv.second.seg); oi.push_back(kv.second.idx); }
}
int tc_compact(hipstr_trace_cache* tc){
  if (tc->segs.empty()) return 0;
  if (tc->n_live == 0){ tc_drop_segments(tc); return 0; }
  if (tc->segs.size() == 1 && tc->n_records == tc->n_live){      // one segment without dead records: is it already in key order?
    int32_t want = 0; bool ordered = true;
    for (const auto& m : tc->keys) for (const auto& kv : m) if (kv.second.idx != want++) ordered = false;
    if (ordered) return 0;
  }
  std::vector<int32_t> os, oi;
  tc_live(tc, os, oi);
  hipstr_trace_dev* one = NULL;
  if (gather_checked(tc->ctx, (int32_t)tc->segs.size(), tc->segs.data(), (int32_t)os.size(), os.data(), oi.data(), &one)) return 1;
  tc_drop_segments(tc);
  tc->segs.push_back(one); tc->n_records = tc->n_live;
  int32_t i = 0;
  for (auto& m : tc->keys) for (auto& kv : m){ kv.second.seg = 0; kv.second.idx = i++; }
  return 0;
}
}  // namespace

extern "C" hipstr_trace_cache_t* hipstr_trace_cache_create(int32_t n_loci, const int32_t* pool_off, const int32_t* n_alleles){
  if (n_loci < 0 || (n_loci > 0 && (!pool_off || !n_alleles))){ api_fail("null argument or negative locus count"); return NULL; }
  if (n_loci > 0 && pool_off[0] != 0){ api_fail("pool_off must start at 0"); return NULL; }
  for (int l = 0; l < n_loci; l++){
    if (pool_off[l+1] < pool_off[l]){ api_fail("pool_off must be ascending (negative read count)"); return NULL; }
    if (n_alleles[l] < 1 || n_alleles[l] + 1 >= 10000){ api_fail("allele count out of range"); return NULL; }
  }
  hipstr_trace_cache* tc = new hipstr_trace_cache();      // (host only: the context is taken with the first call that needs the device)
  tc->n_loci = n_loci;
  if (n_loci > 0){ tc->pool_off.assign(pool_off, pool_off + n_loci + 1); tc->n_alleles.assign(n_alleles, n_alleles + n_loci); }
  else tc->pool_off.assign(1, 0);
  tc->keys.resize((size_t)n_loci);
  return tc;
}

extern "C" void hipstr_trace_cache_free(hipstr_trace_cache_t* tc){
  if (!tc) return;
  tc_drop_segments(tc);
  delete tc;
}

extern "C" int hipstr_trace_cache_round(hipstr_trace_cache_t* tc, const hipstr_batch_t* pooled, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                                        const int32_t* req_seed, const char* const* hap_to_ref, const uint8_t* locus_takes, hipstr_trace_dev_t** td,
                                        hipstr_trace_cache_stats_t* stats){
  if (td) *td = NULL;
  if (!tc || !pooled || !td || n_req < 0 || (n_req > 0 && (!req_read || !req_allele))) return api_fail("null argument");
  const int nl = tc->n_loci;
  if (pooled->n_loci != nl) return api_fail("hipstr_trace_cache_round: n_loci of the cache disagrees with the batch");
  for (int l = 0; l <= nl && nl > 0; l++)
    if (pooled->read_off[l] != tc->pool_off[l]) return api_fail("hipstr_trace_cache_round: the batch's read offsets differ from the cache's pool_off");
  // ---- hits and misses by key
  std::vector<int32_t> req_locus((size_t)n_req), os((size_t)n_req), oi((size_t)n_req), m_read, m_allele, m_seed, m_req;
  std::vector<std::map<uint64_t, int32_t>> fresh((size_t)nl);      // keys this round traces: -> index in the miss list
  const int32_t new_seg = (int32_t)tc->segs.size();
  int last = 0;
  for (int q = 0; q < n_req; q++){
    const int r = req_read[q];
    if (r < 0 || r >= tc->pool_off[nl]) return api_fail("request names a read outside the batch");
    const int l = (int)(std::upper_bound(tc->pool_off.begin(), tc->pool_off.end(), r) - tc->pool_off.begin()) - 1;
    if (l < last) return api_fail("hipstr_trace_cache_round: requests must be grouped by locus, in locus order (request " + std::to_string(q) + ")");
    last = l;
    if (req_allele[q] < 0 || req_allele[q] >= tc->n_alleles[l]) return api_fail("request names an allele outside its locus");
    req_locus[q] = l;
    const uint64_t key = tc_key(r - tc->pool_off[l], req_allele[q]);
    auto hit = tc->keys[l].find(key);
    if (hit != tc->keys[l].end()){ os[q] = hit->second.seg; oi[q] = hit->second.idx; continue; }
    auto ins = fresh[l].insert(std::make_pair(key, (int32_t)m_read.size()));
    if (ins.second){
      m_read.push_back(r); m_allele.push_back(req_allele[q]); m_req.push_back(q);
      if (req_seed) m_seed.push_back(req_seed[q]);
    }
    os[q] = new_seg; oi[q] = ins.first->second;
  }
  const int32_t n_miss = (int32_t)m_read.size();
  if (tc_bind(tc)) return 1;
  // ---- the misses, traced (a refusal is the full list's: a hit cannot be refused, so the first refused miss is the first refused request)
  hipstr_trace_dev* got = NULL;
  if (n_miss > 0){
    const int rc = hipstr_hmm_trace_resident(pooled, n_miss, m_read.data(), m_allele.data(), req_seed ? m_seed.data() : NULL, hap_to_ref, 0u, &got);
    if (rc) return rc;
    if (got->ctx != tc->ctx){ hipstr_trace_dev_free(got); return api_fail("hipstr_trace_cache_round: the cache belongs to another device than the calling thread's"); }
  }
  // ---- one handle with a record per request
  std::vector<hipstr_trace_dev*> src(tc->segs);
  if (got) src.push_back(got);
  hipstr_trace_dev* out = NULL;
  if (gather_checked(tc->ctx, (int32_t)src.size(), src.data(), n_req, os.data(), oi.data(), &out)){ if (got) hipstr_trace_dev_free(got); return 1; }
  // ---- the cache takes what it did not have, for the loci that take
  int64_t inserted = 0;
  for (int l = 0; l < nl; l++){
    if (locus_takes && !locus_takes[l]) continue;
    for (const auto& kv : fresh[l]){ tc->keys[l][kv.first] = hipstr_trace_cache::At{new_seg, kv.second}; inserted++; }
  }
  if (got){
    if (inserted > 0){ tc->segs.push_back(got); tc->n_records += n_miss; tc->n_live += inserted; }
    else hipstr_trace_dev_free(got);
  }
  if (hs_tc_should_compact(tc->n_live, tc->n_records - tc->n_live, (int64_t)tc->segs.size())) tc_compact(tc);      // (a failed compaction leaves the cache as it was)
  tc_stats(tc, (int64_t)n_req - n_miss, n_miss, inserted, stats);
  *td = out;
  return 0;
}

extern "C" int hipstr_trace_cache_remap(hipstr_trace_cache_t* tc, const int32_t* new_n_alleles, const int32_t* allele_mapping){
  if (!tc || (tc->n_loci > 0 && (!new_n_alleles || !allele_mapping))) return api_fail("null argument");
  const int nl = tc->n_loci;
  size_t base = 0;
  for (int l = 0; l < nl; l++){                      // hipstr_rm_remap's refusals, before anything changes
    const int newA = new_n_alleles[l];
    if (newA < 1 || newA + 1 >= 10000) return api_fail("allele count out of range");
    std::vector<uint8_t> taken((size_t)newA, 0);
    for (int j = 0; j < tc->n_alleles[l]; j++){
      const int m = allele_mapping[base + j];
      if (m == -1) continue;
      if (m < 0 || m >= newA) return api_fail("allele_mapping entry out of range at locus " + std::to_string(l));
      if (taken[m]) return api_fail("two old columns mapped to one new column at locus " + std::to_string(l));
      taken[m] = 1;
    }
    base += (size_t)tc->n_alleles[l];
  }
  base = 0;
  for (int l = 0; l < nl; l++){                      // seq_stutter_genotyper.cpp:401-409
    std::map<uint64_t, hipstr_trace_cache::At> next;
    for (const auto& kv : tc->keys[l]){
      const int m = allele_mapping[base + (uint32_t)kv.first];
      if (m != -1) next[tc_key((int32_t)(kv.first >> 32), m)] = kv.second;
    }
    tc->n_live -= (int64_t)tc->keys[l].size() - (int64_t)next.size();
    tc->keys[l].swap(next);
    base += (size_t)tc->n_alleles[l];
    tc->n_alleles[l] = new_n_alleles[l];
  }
  return 0;
}

extern "C" int hipstr_trace_cache_clear(hipstr_trace_cache_t* tc, const uint8_t* locus){
  if (!tc) return api_fail("null argument");
  for (int l = 0; l < tc->n_loci; l++)
    if (!locus || locus[l]){ tc->n_live -= (int64_t)tc->keys[l].size(); tc->keys[l].clear(); }
  if (tc->n_live == 0) tc_drop_segments(tc);          // nothing names a record any more: the segments go back now
  return 0;
}

extern "C" int hipstr_trace_cache_compact(hipstr_trace_cache_t* tc){
  if (!tc) return api_fail("null argument");
  return tc_compact(tc);
}

extern "C" int hipstr_trace_cache_entries(const hipstr_trace_cache_t* tc, int32_t cap, int32_t* n, int32_t* ent_read, int32_t* ent_allele){
  if (!tc || !n) return api_fail("null argument");
  *n = (int32_t)tc->n_live;
  if (tc->n_live > cap){ api_fail("hipstr_trace_cache_entries: cap is too small"); return 3; }
  if (tc->n_live > 0 && (!ent_read || !ent_allele)) return api_fail("null argument");
  size_t i = 0;
  for (int l = 0; l < tc->n_loci; l++)
    for (const auto& kv : tc->keys[l]){ ent_read[i] = tc->pool_off[l] + (int32_t)(kv.first >> 32); ent_allele[i] = (int32_t)(uint32_t)kv.first; i++; }
  return 0;
}

extern "C" int hipstr_trace_cache_view(hipstr_trace_cache_t* tc, hipstr_trace_dev_t** td){
  if (td) *td = NULL;
  if (!tc || !td) return api_fail("null argument");
  if (tc_bind(tc)) return 1;
  std::vector<int32_t> os, oi;
  tc_live(tc, os, oi);
  return gather_checked(tc->ctx, (int32_t)tc->segs.size(), tc->segs.data(), (int32_t)os.size(), os.data(), oi.data(), td);
}

extern "C" int hipstr_trace_cache_stats(const hipstr_trace_cache_t* tc, hipstr_trace_cache_stats_t* stats){
  if (!tc || !stats) return api_fail("null argument");
  tc_stats(tc, 0, 0, 0, stats);
  return 0;
}

#ifndef HIPSTR_NO_DEBUG_ABI
// Diagnostics (host only): trace_cache_layout.h's decisions for a gather of n_out records and a cache of n_live / n_dead records in n_segments.
extern "C" int hipstr_debug_trace_cache_plan(int64_t n_out, int64_t n_live, int64_t n_dead, int64_t n_segments, int64_t out[12]){
  if (!out || n_out < 0 || n_live < 0 || n_dead < 0 || n_segments < 0) return api_fail("bad argument");
  out[0] = hs_tc_len_workgroups(n_out); out[1] = hs_tc_scan_steps(0, n_out); out[2] = hs_tc_scan_steps(HS_TC_FLANK_POOL, n_out);
  out[3] = hs_tc_copy_workgroups(n_out); out[4] = hs_tc_pool_at(HS_TC_POOLS - 1, n_out) + hs_tc_pool_pieces(HS_TC_POOLS - 1, n_out);
  out[5] = hs_tc_should_compact(n_live, n_dead, n_segments) ? 1 : 0;
  out[6] = HS_TC_COMPACT_MIN_DEAD; out[7] = HS_TC_MAX_SEGMENTS; out[8] = HS_TC_LEN_THREADS; out[9] = HS_TC_WAVE; out[10] = HS_TC_TOTALS_BYTES;
  out[11] = hs_tc_pool_fits(n_out) ? 1 : 0;
  return 0;
}
// the calling thread's last gather: kernel milliseconds (measured when HIPSTR_TRACE_GATHER_TIMING is set, else 0), bytes up, bytes home, records
extern "C" int hipstr_debug_trace_gather_last(double out[4]){
  if (!out) return api_fail("null argument");
  const GatherLast& L = t_gather_last;
  out[0] = L.kernel_ms; out[1] = (double)L.bytes_up; out[2] = (double)L.bytes_home; out[3] = (double)L.n_out;
  return 0;
}
#endif  // HIPSTR_NO_DEBUG_ABI
