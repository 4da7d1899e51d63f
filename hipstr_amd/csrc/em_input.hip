// em_input.hip — the step between a resident traceback result and the stutter EM on gfx950: SeqStutterGenotyper::recompute_stutter_models
// (seq_stutter_genotyper.cpp:1542-1581) walks the traced alignments, hands every read whose trace spans the STR block to its sample
// (:1555-1566) and trains EMStutterGenotyper on them.  hipstr_hmm_trace_resident leaves the records on the device and hipstr_em_train's
// loop (em.hip) runs there; this file selects the reads, compacts them and prepares what em_prepare prepares on the host — the alleles, the
// reads' allele indices, the initial allele frequencies (em_stutter_genotyper.cpp:10-20) — without a per-read array crossing the host link:
//   hs_emi_init_kernel     the per-locus minima / maxima start from ref_allele, the check word from "no read"
//   hs_emi_select_kernel   a wavefront per (locus, sample) run of reads, 64 at a time: which reads enter, their num_bps, the run's count
//                          (ballot + population count), the locus' smallest and largest size, the lowest entering read without STR data
//   hs_emi_scan_kernel     exclusive scan of the run counts, in chunks with a carried base: every run's first compact position, em_read_off
//   hs_emi_scatter_kernel  a wavefront per run: num_bps, sample_label, log_p1, log_p2 and weight 1 to the compact position, in read order
//   hs_emi_alleles_kernel  a workgroup per locus: a presence bitmap over [lo, hi] in LDS gives the distinct sizes other than ref_allele
//                          ascending (ref_allele first) and every read's index among them (a prefix population count); then
//                          init_log_gt_priors in the host's order of additions — a thread per allele walks the locus' reads in order, one
//                          thread sums the alleles in order, both logarithms are cr_math.h's
// Per locus the allele count, the entering reads and lo / hi come home, per run its count: the host builds the EM's locus records and
// posterior units from those (em.hip: em_train_prepared).  Every decision of size: em_input_layout.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "post_layout.h"
#include "em_input_layout.h"
#include "prep.h"
#include "api_internal.h"
#include "cr_math.h"

static_assert(HS_EMI_NO_STR_DATA == HIPSTR_NO_STR_DATA, "the kernels' copy of the public constant");
static_assert(HS_EMI_THREADS == HS_EMI_SCAN_CHUNK, "the scan takes a run per thread");

namespace {
__device__ __forceinline__ int emi_wave_min(int v){ for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ int emi_wave_max(int v){ for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }
}  // namespace

extern "C" __global__ void __launch_bounds__(HS_EMI_THREADS) hs_emi_init_kernel(const hs_emi_dev_t* __restrict__ dp){
  const hs_emi_dev_t& d = *dp;
  const int64_t l = (int64_t)blockIdx.x*HS_EMI_THREADS + threadIdx.x;
  if (l < d.n_loci){ d.lo[l] = d.ref_allele; d.hi[l] = d.ref_allele; }
  if (l == 0) d.check[0] = HS_EMI_NO_READ;
}

extern "C" __global__ void __launch_bounds__(HS_EMI_THREADS) hs_emi_select_kernel(const hs_emi_dev_t* __restrict__ dp){
  const hs_emi_dev_t& d = *dp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ub = (int64_t)blockIdx.x*(HS_EMI_THREADS/64) + wave;
  if (ub >= d.n_units) return;                              // (a whole wavefront; nothing below synchronises the workgroup)
  const hs_post_unit_t u = d.units[ub];
  const int locus = d.unit_locus[ub];
  const hs_emi_locus_t L = d.loci[locus];
  int count = 0;                                            // uniform over the lanes
  int lo = d.ref_allele, hi = d.ref_allele, bad = HS_EMI_NO_READ;
  for (int r0 = 0; r0 < u.n_reads; r0 += HS_EMI_WAVE){
    const int r = r0 + lane;
    const bool in = r < u.n_reads;
    const int g = u.read_begin + (in ? r : 0);
    bool enter = false; int nb = 0;
    if (in && d.seed[g] >= 0){                              // traced_alns[r] != NULL: a seed and a request
      const int q = d.read_req[g];
      if (q >= 0 && d.aln_start[q] < L.blk_start && d.aln_stop[q] > L.blk_end){      // :1558-1559, both strict
        enter = true;
        const int ss = d.stutter_size[q];
        if (ss == HS_EMI_NO_STR_DATA) bad = min(bad, g);    // AlignmentTrace::stutter_size asserts
        nb = (d.str_seq_off[q+1] - d.str_seq_off[q]) + ss;  // :1560
        lo = min(lo, nb); hi = max(hi, nb);
      }
    }
    if (in){ d.read_in[g] = enter ? 1 : 0; d.read_bps[g] = nb; }
    count += __popcll(__ballot(enter));
  }
  lo = emi_wave_min(lo); hi = emi_wave_max(hi); bad = emi_wave_min(bad);
  if (lane == 0){
    d.run_count[ub] = count;
    if (lo < d.ref_allele) atomicMin(&d.lo[locus], lo);
    if (hi > d.ref_allele) atomicMax(&d.hi[locus], hi);
    if (bad != HS_EMI_NO_READ) atomicMin(d.check, bad);
  }
}

// One workgroup: a thread per run of a chunk, an inclusive scan (Hillis-Steele) per chunk, the base carried from chunk to chunk.
extern "C" __global__ void __launch_bounds__(HS_EMI_THREADS) hs_emi_scan_kernel(const hs_emi_dev_t* __restrict__ dp){
  const hs_emi_dev_t& d = *dp;
  const int tid = threadIdx.x;
  __shared__ int sc[HS_EMI_SCAN_CHUNK];
  __shared__ int base;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int u0 = 0; u0 < d.n_units; u0 += HS_EMI_SCAN_CHUNK){
    const int u = u0 + tid;
    const int v = u < d.n_units ? d.run_count[u] : 0;
    sc[tid] = v;
    __syncthreads();
    for (int off = 1; off < HS_EMI_SCAN_CHUNK; off <<= 1){
      const int a = tid >= off ? sc[tid - off] : 0;
      __syncthreads();
      sc[tid] += a;
      __syncthreads();
    }
    if (u < d.n_units) d.run_base[u] = base + sc[tid] - v;
    __syncthreads();
    if (tid == HS_EMI_SCAN_CHUNK - 1) base += sc[HS_EMI_SCAN_CHUNK - 1];
    __syncthreads();
  }
  if (tid == 0) d.run_base[d.n_units] = base;
  __syncthreads();                                          // (the workgroup's own global writes are visible to it behind the barrier)
  for (int l = tid; l <= d.n_loci; l += HS_EMI_THREADS)
    d.em_read_off[l] = l < d.n_loci ? d.run_base[d.loci[l].unit_first] : base;
}

extern "C" __global__ void __launch_bounds__(HS_EMI_THREADS) hs_emi_scatter_kernel(const hs_emi_dev_t* __restrict__ dp){
  const hs_emi_dev_t& d = *dp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ub = (int64_t)blockIdx.x*(HS_EMI_THREADS/64) + wave;
  if (ub >= d.n_units) return;
  const hs_post_unit_t u = d.units[ub];
  const int label = u.samp_index - d.loci[d.unit_locus[ub]].samp_begin;
  int pos = d.run_base[ub];                                 // uniform over the lanes
  for (int r0 = 0; r0 < u.n_reads; r0 += HS_EMI_WAVE){
    const int r = r0 + lane;
    const bool in = r < u.n_reads;
    const int g = u.read_begin + (in ? r : 0);
    const bool enter = in && d.read_in[g] != 0;
    const unsigned long long mask = __ballot(enter);
    if (enter){
      const int at = pos + __popcll(mask & ((1ull << lane) - 1ull));      // entering reads of lower lanes: the reads keep their order
      d.num_bps[at] = d.read_bps[g]; d.sample_label[at] = label; d.weight[at] = 1;
      d.c_log_p1[at] = d.log_p1[g]; d.c_log_p2[at] = d.log_p2[g];
    }
    pos += __popcll(mask);
  }
}

extern "C" __global__ void __launch_bounds__(HS_EMI_THREADS) hs_emi_alleles_kernel(const hs_emi_dev_t* __restrict__ dp){
  const hs_emi_dev_t& d = *dp;
  const int l = blockIdx.x, tid = threadIdx.x;
  const int r0 = d.em_read_off[l], R = d.em_read_off[l+1] - r0;
  const int lo = d.lo[l], hi = d.hi[l], ref = d.ref_allele;
  if (!hs_emi_bitmap_fits(lo, hi)){                         // (the whole workgroup) the call takes the host's preparation
    if (tid == 0) d.n_sizes[l] = -1;
    return;
  }
  __shared__ uint32_t bm[HS_EMI_BITMAP_WORDS];
  __shared__ int pre[HS_EMI_BITMAP_WORDS];
  __shared__ int s_A;
  __shared__ double s_lt;
  const int nw = hs_emi_bitmap_words(lo, hi);
  for (int w = tid; w < nw; w += HS_EMI_THREADS) bm[w] = 0u;
  __syncthreads();
  const int32_t* nbv = d.num_bps + r0;
  for (int r = tid; r < R; r += HS_EMI_THREADS){
    const int nb = nbv[r];
    if (nb != ref){ const unsigned p = (unsigned)(nb - lo); atomicOr(&bm[p >> 5], 1u << (p & 31)); }
  }
  __syncthreads();
  if (tid == 0){
    int run = 0;
    for (int w = 0; w < nw; w++){ pre[w] = run; run += __popc(bm[w]); }
    s_A = run + 1;                                          // the reference size comes first, observed or not
  }
  __syncthreads();
  const int A = s_A;
  const int64_t bo = hs_emi_bps_off(r0, l);
  int32_t* bps = d.bps + bo; double* gtp = d.gtp + bo; int32_t* obs = d.obs + r0;
  if (tid == 0){ bps[0] = ref; d.n_sizes[l] = A; }
  for (int w = tid; w < nw; w += HS_EMI_THREADS){
    uint32_t bits = bm[w]; int k = pre[w];
    while (bits){ const int b = __ffs(bits) - 1; bps[1 + k] = lo + 32*w + b; k++; bits &= bits - 1u; }
  }
  for (int r = tid; r < R; r += HS_EMI_THREADS){
    const int nb = nbv[r];
    int o = 0;
    if (nb != ref){ const unsigned p = (unsigned)(nb - lo); o = 1 + pre[p >> 5] + __popc(bm[p >> 5] & ((1u << (p & 31)) - 1u)); }
    obs[r] = o;
  }
  if (!hs_emi_sizes_fit(A)) return;                         // (the whole workgroup) "too many distinct allele sizes" on the host
  __syncthreads();
  // init_log_gt_priors (em_stutter_genotyper.cpp:10-20): g[a] = 1.0 + sum of 1.0/reads_of_sample over the reads of allele a, added in read order
  const int32_t* lab = d.sample_label + r0;
  const int32_t* ros = d.run_count + d.loci[l].unit_first;
  for (int a = tid; a < A; a += HS_EMI_THREADS){
    double g = 1.0;
    for (int r = 0; r < R; r++) if (obs[r] == a) g += 1.0/(double)ros[lab[r]];
    gtp[a] = g;
  }
  __syncthreads();
  if (tid == 0){
    double tot = 0.0;
    for (int a = 0; a < A; a++) tot += gtp[a];              // in allele order
    s_lt = cr_log(tot);
  }
  __syncthreads();
  const double lt = s_lt;
  for (int a = tid; a < A; a += HS_EMI_THREADS) gtp[a] = cr_log(gtp[a]) - lt;
}

// ---- host side -------------------------------------------------------------------------------------------------
namespace {
using hipstr::api_fail;

// The checks of the host's tables both forms share, worded as hipstr_post_census words its own: the locus of every request, every read's
// request.  read_off: [n_loci+1] the un-pooled reads of every locus.
int emi_check_tables(int nl, const int32_t* read_off, const hipstr_em_trace_request_t* rq, std::vector<int32_t>& req_locus){
  const hipstr_batch_t* b = rq->pooled;
  if (b->n_loci != nl) return api_fail("hipstr_em_batch_from_traces: pooled->n_loci differs from the posterior batch's");
  const int32_t nq = rq->n_req;
  req_locus.resize((size_t)nq);
  {
    int l = 0;
    const int32_t n_pooled = nl ? b->read_off[nl] : 0;
    for (int32_t k = 0; k < nq; k++){
      const int32_t pr = rq->req_read[k];
      if (pr < 0 || pr >= n_pooled) return api_fail("hipstr_em_batch_from_traces: req_read outside the pooled reads");
      while (l < nl && pr >= b->read_off[l+1]) l++;
      if (pr < b->read_off[l]) return api_fail("hipstr_em_batch_from_traces: requests must be grouped by locus, in locus order");
      req_locus[k] = l;
    }
  }
  for (int l = 0; l < nl; l++)
    for (int r = read_off[l]; r < read_off[l+1]; r++){
      const int32_t k = rq->read_req[r];
      if (k < -1 || k >= nq) return api_fail("hipstr_em_batch_from_traces: read_req outside [-1, n_req)");
      if (k >= 0 && req_locus[k] != l) return api_fail("hipstr_em_batch_from_traces: a read's request belongs to another locus");
    }
  return 0;
}
int emi_fail_no_str(int read){
  return api_fail("hipstr_em_batch_from_traces: read " + std::to_string(read) + " enters the EM but its request has no STR data (AlignmentTrace::stutter_size asserts)");
}
bool emi_null_request(const hipstr_em_trace_request_t* rq){
  if (!rq || !rq->pooled || !rq->seed || !rq->read_req) return true;
  const hipstr_batch_t* b = rq->pooled;
  return b->n_loci < 0 || (b->n_loci && (!b->blk_start || !b->blk_end || !b->period || !b->read_off)) || (rq->n_req > 0 && !rq->req_read);
}
}  // namespace

extern "C" int hipstr_em_batch_from_traces(const hipstr_post_batch_t* pb, const hipstr_em_trace_request_t* rq, const hipstr_trace_out_t* tr,
                                           int32_t* em_read_off, int32_t* sample_label, int32_t* num_bps, double* log_p1, double* log_p2){
  if (!pb || !tr || !em_read_off || !sample_label || !num_bps || !log_p1 || !log_p2 || emi_null_request(rq)) return api_fail("null argument");
  const int nl = pb->n_loci;
  if (nl < 0 || (nl && (!pb->n_samples || !pb->read_off || !pb->sample_label || !pb->log_p1 || !pb->log_p2))) return api_fail("null argument");
  if (rq->n_req < 0) return api_fail("hipstr_em_batch_from_traces: negative n_req");
  if (rq->n_req && (!tr->aln_start || !tr->aln_stop || !tr->stutter_size || !tr->str_seq_off))
    return api_fail("hipstr_em_batch_from_traces: trace output without aln_start / aln_stop / stutter_size / str_seq_off");
  std::vector<int32_t> req_locus;
  const int32_t zero_off[1] = {0};
  if (emi_check_tables(nl, nl ? pb->read_off : zero_off, rq, req_locus)) return 1;
  const hipstr_batch_t* b = rq->pooled;
  auto enters = [&](int l, int r){
    if (rq->seed[r] < 0) return false;
    const int q = rq->read_req[r];
    return q >= 0 && tr->aln_start[q] < b->blk_start[3*l + 1] && tr->aln_stop[q] > b->blk_end[3*l + 1];      // :1558-1559
  };
  for (int l = 0; l < nl; l++)                               // everything checked before anything is written
    for (int r = pb->read_off[l]; r < pb->read_off[l+1]; r++)
      if (enters(l, r) && tr->stutter_size[rq->read_req[r]] == HIPSTR_NO_STR_DATA) return emi_fail_no_str(r);
  int32_t n = 0;
  for (int l = 0; l < nl; l++){
    em_read_off[l] = n;
    for (int r = pb->read_off[l]; r < pb->read_off[l+1]; r++){
      if (!enters(l, r)) continue;
      const int q = rq->read_req[r];
      num_bps[n] = (tr->str_seq_off[q+1] - tr->str_seq_off[q]) + tr->stutter_size[q];      // :1560
      sample_label[n] = pb->sample_label[r]; log_p1[n] = pb->log_p1[r]; log_p2[n] = pb->log_p2[r];
      n++;
    }
  }
  em_read_off[nl] = n;
  return 0;
}

namespace {
// A device-built preparation: the blocks it lies in (they go back to the caches when it dies, behind the stream) and what came home.
struct EmiRun {
  hipstr::PostView V;
  hipstr::ApiTables T;
  hipstr::HostArena ar;
  hipstr::ResultBlocks B;
  hs_emi_dev_t h;
  int nl = 0; size_t n = 0, nu = 0;
  const int32_t *run_count = NULL, *lo = NULL, *hi = NULL, *em_read_off = NULL, *n_sizes = NULL;      // pinned: what came home
  bool host_path = false;            // the whole call takes em_prepare on the fetched compact arrays
  int fetch(void* dst, const void* src, size_t bytes){ return hipstr::fetch_to_host(V.ctx, T.stream, dst, src, bytes); }
};

// Everything up to the EM loop: the refusals, the five kernels, the counts home.  nl == 0: nothing is done (X.nl == 0).
int emi_prepare(hipstr_post_dev_t* pd, const hipstr_em_trace_request_t* rq, const hipstr_trace_dev_t* td, EmiRun& X){
  if (rq->n_req < 0) return api_fail("hipstr_em_batch_from_traces: negative n_req");
  if (rq->n_req != td->n_req) return api_fail("hipstr_em_train_dev: rq->n_req differs from the trace handle's");
  hipstr::post_view(pd, &X.V);
  const hipstr::PostView& V = X.V;
  if (td->ctx != V.ctx) return api_fail("hipstr_em_train_dev: the trace handle lives on another device than the posteriors");
  if (rq->n_req && (!td->scal[0] || !td->scal[3] || !td->scal[4] || !td->off[1]))
    return api_fail("hipstr_em_batch_from_traces: trace output without aln_start / aln_stop / stutter_size / str_seq_off");
  const int nl = (int)V.n_loci;
  const size_t n = (size_t)V.n_reads, nu = V.n_units;
  // the loci's runs and reads, from the run's units (locus-major, a unit per sample)
  std::vector<hs_emi_locus_t> loci((size_t)nl);
  std::vector<int32_t> unit_locus(nu), read_off, unit_off;
  V.locus_tables(read_off, unit_off);
  const hipstr_batch_t* b = rq->pooled;
  for (int l = 0; l < nl; l++){
    hs_emi_locus_t& L = loci[l]; memset(&L, 0, sizeof L);
    const size_t ui = (size_t)unit_off[l];
    L.unit_first = unit_off[l]; L.n_units = V.n_samples[l];
    L.samp_begin = ui < nu ? V.units[ui].samp_index : (int32_t)V.n_samp;
    std::fill(unit_locus.begin() + unit_off[l], unit_locus.begin() + unit_off[l+1], l);
    if (b->n_loci == nl){ L.blk_start = b->blk_start[3*l + 1]; L.blk_end = b->blk_end[3*l + 1]; }
  }
  std::vector<int32_t> req_locus;
  if (emi_check_tables(nl, read_off.data(), rq, req_locus)) return 1;
  if (nl == 0) return 0;
  if (hipstr::api_tables_of(V.ctx, &X.T)) return 1;
  hipStream_t st = X.T.stream;
  X.nl = nl; X.n = n; X.nu = nu;

  hipstr::HostArena& ar = X.ar;
  const size_t o_loci = ar.add(loci.data(), loci.size()*sizeof(hs_emi_locus_t)), o_uloc = ar.add(unit_locus.data(), nu*4),
               o_seed = ar.add(rq->seed, n*4), o_rreq = ar.add(rq->read_req, n*4);
  hs_emi_dev_t& h = X.h; memset(&h, 0, sizeof h);
  const size_t o_args = ar.add(&h, sizeof h);
  if (ar.reserve(V.ctx)) return 1;
  // what comes home, back to back (one copy), then what stays on the device
  hipstr::ResultBlocks& B = X.B;
  const size_t r_count = B.take(nu*4), r_lo = B.take((size_t)nl*4), r_hi = B.take((size_t)nl*4), r_check = B.take(4), r_eoff = B.take(((size_t)nl + 1)*4),
               r_nsz = B.take((size_t)nl*4);
  B.end_results();
  const size_t d_rbps = B.take(n*4), d_rin = B.take(n), d_base = B.take((nu + 1)*4), d_nb = B.take(n*4), d_lab = B.take(n*4), d_w = B.take(n*4), d_obs = B.take(n*4),
               d_p1 = B.take(n*8), d_p2 = B.take(n*8), d_bps = B.take((n + (size_t)nl)*4), d_gtp = B.take((n + (size_t)nl)*8);
  if (B.reserve(V.ctx, st)) return 1;
  h.units = V.d_units; h.loci = ar.at<hs_emi_locus_t>(o_loci); h.unit_locus = ar.at<int32_t>(o_uloc);
  h.n_units = (int32_t)nu; h.n_loci = nl; h.ref_allele = rq->ref_allele; h.n_reads = (int32_t)n;
  h.log_p1 = V.log_p1; h.log_p2 = V.log_p2; h.seed = ar.at<int32_t>(o_seed); h.read_req = ar.at<int32_t>(o_rreq);
  h.stutter_size = td->scal[0]; h.aln_start = td->scal[3]; h.aln_stop = td->scal[4]; h.str_seq_off = td->off[1];
  h.read_bps = B.dev<int32_t>(d_rbps); h.read_in = B.dev<uint8_t>(d_rin); h.run_base = B.dev<int32_t>(d_base);
  h.run_count = B.dev<int32_t>(r_count); h.lo = B.dev<int32_t>(r_lo); h.hi = B.dev<int32_t>(r_hi); h.check = B.dev<int32_t>(r_check);
  h.em_read_off = B.dev<int32_t>(r_eoff); h.n_sizes = B.dev<int32_t>(r_nsz);
  h.num_bps = B.dev<int32_t>(d_nb); h.sample_label = B.dev<int32_t>(d_lab); h.weight = B.dev<int32_t>(d_w); h.obs = B.dev<int32_t>(d_obs);
  h.c_log_p1 = B.dev<double>(d_p1); h.c_log_p2 = B.dev<double>(d_p2); h.bps = B.dev<int32_t>(d_bps); h.gtp = B.dev<double>(d_gtp);
  // the run's inputs may still be on their way (a small run sends them asynchronously on its own stream)
  if (V.ev_up && st != V.stream) HS_HIP(hipStreamWaitEvent(st, V.ev_up, 0));
  if (ar.send(st)) return 1;
  const hs_emi_dev_t* d_args = ar.at<hs_emi_dev_t>(o_args);
  const unsigned g_runs = (unsigned)hs_emi_run_workgroups((int64_t)nu);
  hipLaunchKernelGGL(hs_emi_init_kernel, dim3((unsigned)((nl + HS_EMI_THREADS - 1)/HS_EMI_THREADS)), dim3(HS_EMI_THREADS), 0, st, d_args);
  if (nu) hipLaunchKernelGGL(hs_emi_select_kernel, dim3(g_runs), dim3(HS_EMI_THREADS), 0, st, d_args);
  hipLaunchKernelGGL(hs_emi_scan_kernel, dim3(1), dim3(HS_EMI_THREADS), 0, st, d_args);
  if (nu) hipLaunchKernelGGL(hs_emi_scatter_kernel, dim3(g_runs), dim3(HS_EMI_THREADS), 0, st, d_args);
  hipLaunchKernelGGL(hs_emi_alleles_kernel, dim3((unsigned)nl), dim3(HS_EMI_THREADS), 0, st, d_args);
  HS_HIP(hipGetLastError());
  if (B.fetch()) return 1;
  X.run_count = B.host<int32_t>(r_count); X.lo = B.host<int32_t>(r_lo); X.hi = B.host<int32_t>(r_hi);
  X.em_read_off = B.host<int32_t>(r_eoff); X.n_sizes = B.host<int32_t>(r_nsz);
  const int32_t bad = *B.host<int32_t>(r_check);
  if (bad != HS_EMI_NO_READ) return emi_fail_no_str(bad);
  // what the device does not prepare: the batches hipstr_em_train refuses (its verdict and message: em_prepare's, on the compact arrays)
  // and a legal locus whose sizes span the table of integer logarithms or more
  const int64_t n_logs = (int64_t)hipstr::host_tables().int_log.size();
  X.host_path = n_logs != HS_EMI_SPAN_LIMIT || (getenv("HIPSTR_EM_HOST_LOOP") && atoi(getenv("HIPSTR_EM_HOST_LOOP")) != 0);
  for (int l = 0; l < nl && !X.host_path; l++)
    if (b->period[l] < 1 || b->period[l] > 9 || V.n_samples[l] < 1 || X.n_sizes[l] < 0 || !hs_emi_sizes_fit(X.n_sizes[l])) X.host_path = true;
  return 0;
}

// the compact arrays on the host, as a hipstr_em_batch_t (the host path, and the debug fetch)
struct EmiHostBatch {
  std::vector<int32_t> read_off, label, bps; std::vector<double> p1, p2;
  hipstr_em_batch_t eb;
};
int emi_host_batch(EmiRun& X, const hipstr_em_trace_request_t* rq, EmiHostBatch& B){
  const int nl = X.nl;
  const size_t m = (size_t)X.em_read_off[nl];
  B.read_off.assign(X.em_read_off, X.em_read_off + nl + 1);
  B.label.resize(m); B.bps.resize(m); B.p1.resize(m); B.p2.resize(m);
  if (X.fetch(B.bps.data(), X.h.num_bps, m*4) || X.fetch(B.label.data(), X.h.sample_label, m*4) || X.fetch(B.p1.data(), X.h.c_log_p1, m*8) ||
      X.fetch(B.p2.data(), X.h.c_log_p2, m*8)) return 1;
  hipstr_em_batch_t& eb = B.eb; memset(&eb, 0, sizeof eb);
  eb.n_loci = nl; eb.period = rq->pooled->period; eb.haploid = X.V.haploid; eb.n_samples = X.V.n_samples; eb.read_off = B.read_off.data();
  eb.sample_label = B.label.data(); eb.num_bps = B.bps.data(); eb.log_p1 = B.p1.data(); eb.log_p2 = B.p2.data();
  eb.ref_allele = rq->ref_allele; eb.max_iter = rq->max_iter; eb.min_ll_abs_change = rq->min_ll_abs_change; eb.min_ll_frac_change = rq->min_ll_frac_change;
  return 0;
}
}  // namespace

extern "C" int hipstr_em_train_dev(hipstr_post_dev_t* pd, const hipstr_em_trace_request_t* rq, const hipstr_trace_dev_t* td, hipstr_em_trace_out_t* out){
  if (!pd || !td || !out || !out->trained || !out->stutter || !out->n_iter || !out->final_ll || emi_null_request(rq)) return api_fail("null argument");
  EmiRun X;
  if (emi_prepare(pd, rq, td, X)) return 1;
  const int nl = X.nl;
  if (nl == 0){ if (out->em_read_off) out->em_read_off[0] = 0; return 0; }
  std::vector<int32_t> n_sizes(X.n_sizes, X.n_sizes + nl);
  if (X.host_path){
    EmiHostBatch B;
    if (emi_host_batch(X, rq, B)) return 1;
    if (hipstr::em_train_batch_on(X.T, &B.eb, out->trained, out->stutter, out->n_iter, out->final_ll)) return 1;
    for (int l = 0; l < nl; l++){                            // the EM's alleles: the distinct sizes other than ref_allele, and ref_allele
      std::vector<int32_t> v;
      for (int r = B.read_off[l]; r < B.read_off[l+1]; r++) if (B.bps[r] != rq->ref_allele) v.push_back(B.bps[r]);
      std::sort(v.begin(), v.end());
      n_sizes[l] = 1 + (int32_t)(std::unique(v.begin(), v.end()) - v.begin());
    }
  } else {
    std::vector<hipstr::EmLocusFacts> facts((size_t)nl);
    for (int l = 0; l < nl; l++){
      hipstr::EmLocusFacts& F = facts[l];
      F.A = X.n_sizes[l]; F.S = X.V.n_samples[l]; F.read_begin = X.em_read_off[l]; F.R = X.em_read_off[l+1] - X.em_read_off[l];
      F.period = rq->pooled->period[l]; F.haploid = X.V.haploid[l] ? 1 : 0; F.bps_off = (int32_t)hs_emi_bps_off(X.em_read_off[l], l);
    }
    const hipstr::EmDeviceArrays arr = { X.h.bps, X.h.obs, X.h.sample_label, X.h.weight, X.h.c_log_p1, X.h.c_log_p2, X.h.gtp };
    if (hipstr::em_train_prepared(X.T, nl, facts.data(), X.run_count, arr, rq->max_iter, rq->min_ll_abs_change, rq->min_ll_frac_change,
                                  out->trained, out->stutter, out->n_iter, out->final_ll)) return 1;
  }
  if (out->em_read_off) memcpy(out->em_read_off, X.em_read_off, ((size_t)nl + 1)*4);
  if (out->n_sizes) memcpy(out->n_sizes, n_sizes.data(), (size_t)nl*4);
  return 0;
}

#ifndef HIPSTR_NO_DEBUG_ABI
extern "C" int hipstr_debug_em_input_plan(int64_t n_runs, int64_t run_reads, int64_t lo, int64_t hi, int64_t n_sizes, int64_t out[12]){
  if (!out || n_runs < 0 || run_reads < 0 || hi < lo || n_sizes < 1) return api_fail("bad argument");
  const bool fits = hs_emi_bitmap_fits(lo, hi);
  out[0] = hs_emi_run_steps(run_reads); out[1] = hs_emi_last_step(run_reads); out[2] = hs_emi_run_workgroups(n_runs);
  out[3] = hs_emi_scan_chunks(n_runs); out[4] = n_runs ? hs_emi_scan_chunk_len(n_runs, out[3] - 1) : 0;
  out[5] = fits ? 1 : 0; out[6] = fits ? hs_emi_bitmap_words(lo, hi) : 0; out[7] = fits && hs_emi_sizes_fit(n_sizes) ? 1 : 0;
  out[8] = HS_EMI_THREADS; out[9] = HS_EMI_WAVE; out[10] = HS_EMI_SCAN_CHUNK; out[11] = HS_EMI_SPAN_LIMIT;
  return 0;
}

extern "C" int hipstr_debug_em_input_fetch(hipstr_post_dev_t* pd, const hipstr_em_trace_request_t* rq, const hipstr_trace_dev_t* td, hipstr_debug_em_input_t* o){
  if (!pd || !td || !o || !o->em_read_off || !o->num_bps || !o->sample_label || !o->obs || !o->log_p1 || !o->log_p2 || !o->size_off || !o->sizes ||
      !o->log_freq || !o->route || emi_null_request(rq)) return api_fail("null argument");
  EmiRun X;
  if (emi_prepare(pd, rq, td, X)) return 1;
  const int nl = X.nl;
  o->em_read_off[0] = 0; o->size_off[0] = 0; *o->route = 0;
  if (nl == 0) return 0;
  EmiHostBatch B;
  if (emi_host_batch(X, rq, B)) return 1;
  const size_t m = (size_t)X.em_read_off[nl];
  std::vector<int32_t> size_off, sizes, obs; std::vector<double> freq;
  if (X.host_path){
    if (hipstr::em_prepare_host(&B.eb, size_off, sizes, obs, freq)) return 1;
  } else {
    obs.resize(m);
    if (X.fetch(obs.data(), X.h.obs, m*4)) return 1;
    std::vector<int32_t> all(m + (size_t)nl); std::vector<double> allf(m + (size_t)nl);
    if (X.fetch(all.data(), X.h.bps, all.size()*4) || X.fetch(allf.data(), X.h.gtp, allf.size()*8)) return 1;
    size_off.assign(1, 0);
    for (int l = 0; l < nl; l++){                            // the loci's pieces (hs_emi_bps_off), dense
      const size_t bo = (size_t)hs_emi_bps_off(X.em_read_off[l], l);
      sizes.insert(sizes.end(), all.begin() + bo, all.begin() + bo + X.n_sizes[l]);
      freq.insert(freq.end(), allf.begin() + bo, allf.begin() + bo + X.n_sizes[l]);
      size_off.push_back((int32_t)sizes.size());
    }
  }
  *o->route = X.host_path ? 1 : 0;
  memcpy(o->em_read_off, X.em_read_off, ((size_t)nl + 1)*4);
  if (m){ memcpy(o->num_bps, B.bps.data(), m*4); memcpy(o->sample_label, B.label.data(), m*4); memcpy(o->obs, obs.data(), m*4);
          memcpy(o->log_p1, B.p1.data(), m*8); memcpy(o->log_p2, B.p2.data(), m*8); }
  memcpy(o->size_off, size_off.data(), size_off.size()*4);
  if (!sizes.empty()){ memcpy(o->sizes, sizes.data(), sizes.size()*4); memcpy(o->log_freq, freq.data(), freq.size()*8); }
  return 0;
}
#endif  // HIPSTR_NO_DEBUG_ABI
