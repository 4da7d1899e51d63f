// census.hip — the allele census between two rounds of SeqStutterGenotyper::genotype() on gfx950: the stutter-candidate alleles of
// get_stutter_candidate_alleles (seq_stutter_genotyper.cpp:843-879) and the called / spanned marks of get_unused_alleles (:229-315), from the
// resident MAP pairs and likelihood matrix of a posterior run and the five trace fields of the round's requests.
//
// One work item is a locus; its requests, reads, keys and samples are the lanes of six phases with a barrier between them:
//   A  requests: FNV-1a hash of the request's STR sequence, the span test of its trace
//   B  requests: class = the lowest-numbered request of the locus with the same content (equal length and hash, then equal bytes)
//   C  reads:    n_spanning / n_span_stutter of the read's sample (integer atomics), one key (sample, class) per read that spans with
//                stutter, the spanned mark of a read that spans without (get_unused_alleles' own tie rule, :280-284), the sample's
//                "has an aligned read" flag
//   D  keys:     occurrences of the lane's key among the locus' keys, the test of :869; a key that passes marks its class
//   E  requests: a marked canonical request whose string block 1 does not hold (:870) is a candidate; then its position among the locus'
//                candidates in orderByLengthAndSequence (a count of the candidates that come before it)
//   F  samples:  the called marks of the sample's MAP pair
// Everything counted is an integer and every mark is an idempotent store, so no order of arrival changes a byte of the output.  Where a key
// lands in the key list depends on the order the atomics arrive in; its count does not.
// The workspace of a locus (census_layout.h: three dwords per request, a dword per read, the key counter) lies in LDS — one wavefront's slice
// for a locus that fits a wavefront (route 0, four loci per workgroup, no workgroup barrier), the workgroup's 48 KiB (route 1) — or in a
// global block (route 2); the phases are the same code over a pointer.  hs_census_scan_kernel turns the loci's candidate counts into
// cand_off, hs_census_emit_kernel writes every candidate's request at its position.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "census_layout.h"
#include "device_common.h"

namespace {

template <int ROUTE>
__device__ __forceinline__ void census_sync(){
  if (ROUTE == HS_CENSUS_ROUTE_WAVE){         // one wavefront: its LDS operations complete in order; keep the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  } else
    __syncthreads();
}

__device__ __forceinline__ int census_load(const int32_t* p){ return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// is the string one of block 1's options (HapBlock::contains)
__device__ __forceinline__ bool census_in_block(const hs_census_dev_t& d, const hs_census_locus_t& L, const char* s, int len){
  for (int o = 0; o < L.n_opts[1]; o++){
    const int b = d.o1_off[L.o1_begin + o], e = d.o1_off[L.o1_begin + o + 1];
    if (e - b == len && hs_census_same(d.o1_seq + b, s, len)) return true;
  }
  return false;
}

template <int ROUTE>
__device__ __forceinline__ void census_body(const hs_census_dev_t& d, const hs_census_locus_t& L, int locus, int32_t* ws, const int t){
  constexpr int T = ROUTE == HS_CENSUS_ROUTE_WAVE ? 64 : HS_CENSUS_THREADS;
  const int nq = L.n_req, nr = L.n_reads;
  int32_t* hsh = ws, *cls = ws + nq, *flg = ws + 2*(int64_t)nq, *keys = ws + HS_CENSUS_REQ_INTS*(int64_t)nq, *n_keys = keys + nr;
  const int32_t* off = d.str_seq_off + L.req_begin;
  // ---- A
  for (int q = t; q < nq; q += T){
    const int Q = L.req_begin + q;
    hsh[q] = (int32_t)hs_census_hash(d.str_seq + off[q], off[q+1] - off[q]);
    flg[q] = (d.aln_start[Q] < L.blk_start && d.aln_stop[Q] > L.blk_end) ? HS_CENSUS_SPAN : 0;
  }
  if (t == 0) *n_keys = 0;
  census_sync<ROUTE>();
  // ---- B
  for (int q = t; q < nq; q += T) cls[q] = hs_census_class_of(q, hsh, off, d.str_seq);
  census_sync<ROUTE>();
  // ---- C
  for (int r = t; r < nr; r += T){
    const int g = L.read_begin + r;
    if (d.seed[g] < 0) continue;
    const int s = d.read_samp[g];
    d.has_read[s] = 1;
    const int rr = d.read_req[g];
    if (rr < 0) continue;
    const int q = rr - L.req_begin;
    if (!(flg[q] & HS_CENSUS_SPAN)) continue;
    atomicAdd(&d.n_spanning[s], 1);                                         // :860
    if (d.stutter_size[rr] != 0){                                           // :858-859
      atomicAdd(&d.n_span_stutter[s], 1);
      const int k = atomicAdd(n_keys, 1);
      keys[k] = (s - L.samp_begin)*nq + cls[q];
    } else if (d.h2a[1]){                                                   // :276-285
      const int ha = d.map_gt[2*s], hb = d.map_gt[2*s + 1];
      if (ha < 0 || hb < 0) continue;                                       // no MAP pair (the reference would index haplotype -1)
      int best = ha;
      if (!L.haploid && ha != hb){
        const double* row = d.log_aln_probs + L.ll_off + (int64_t)r*L.n_alleles;
        const double v1 = d.log_p1[g] + row[ha], v2 = d.log_p2[g] + row[hb];
        if (fabs(v1 - v2) > 1e-10) best = v1 > v2 ? ha : hb;                // TOLERANCE, mathops.cpp:10
      }
      d.spanned[L.opt_begin[1] + d.h2a[1][L.hap_begin + best]] = 1;
    }
  }
  census_sync<ROUTE>();
  // ---- D
  const int nk = census_load(n_keys);
  for (int i = t; i < nk; i += T){
    const int key = keys[i], s = key / nq, c = key - s*nq;
    const int count = hs_census_count_key(keys, nk, key);
    if (hs_census_qualifies(count, census_load(&d.n_spanning[L.samp_begin + s]), d.min_reads, d.min_frac)) atomicOr(&flg[c], HS_CENSUS_QUAL);
  }
  census_sync<ROUTE>();
  // ---- E
  for (int q = t; q < nq; q += T)
    if ((flg[q] & HS_CENSUS_QUAL) && cls[q] == q && !census_in_block(d, L, d.str_seq + off[q], off[q+1] - off[q])) atomicOr(&flg[q], HS_CENSUS_CAND);
  census_sync<ROUTE>();
  int mine = 0;
  for (int q = t; q < nq; q += T){
    int rank = -1;
    if (flg[q] & HS_CENSUS_CAND){ rank = hs_census_rank_of(q, nq, flg, off, d.str_seq); mine++; }
    d.req_rank[L.req_begin + q] = rank;
  }
  if (mine) atomicAdd(&d.cand_count[locus], mine);
  // ---- F
  for (int s = t; s < L.n_samp; s += T){
    const int S = L.samp_begin + s;
    const int ha = d.map_gt[2*S], hb = d.map_gt[2*S + 1];
    if (!d.has_read[S] || (d.uncallable && d.uncallable[S]) || ha < 0 || hb < 0) continue;      // :296
    for (int b = 0; b < 3; b++)
      if (d.h2a[b]){
        d.called[L.opt_begin[b] + d.h2a[b][L.hap_begin + ha]] = 1;                              // :297-298
        d.called[L.opt_begin[b] + d.h2a[b][L.hap_begin + hb]] = 1;
      }
  }
}

}  // namespace

// route 0: a wavefront per locus, its workspace a slice of the workgroup's LDS
extern "C" __global__ void __launch_bounds__(HS_CENSUS_THREADS) hs_census_wave_kernel(const hs_census_dev_t* __restrict__ dp){
  const hs_census_dev_t& d = *dp;
  __shared__ int32_t lds[HS_CENSUS_THREADS/64][HS_CENSUS_WAVE_INTS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x*(HS_CENSUS_THREADS/64) + wave;
  if (i >= d.n_list[HS_CENSUS_ROUTE_WAVE]) return;          // (a whole wavefront; nothing below synchronises the workgroup)
  const int locus = d.list[HS_CENSUS_ROUTE_WAVE][i];
  census_body<HS_CENSUS_ROUTE_WAVE>(d, d.loci[locus], locus, lds[wave], lane);
}
// route 1: a workgroup per locus, the workspace in LDS
extern "C" __global__ void __launch_bounds__(HS_CENSUS_THREADS) hs_census_lds_kernel(const hs_census_dev_t* __restrict__ dp){
  const hs_census_dev_t& d = *dp;
  __shared__ int32_t lds[HS_CENSUS_LDS_INTS];
  const int locus = d.list[HS_CENSUS_ROUTE_LDS][blockIdx.x];
  census_body<HS_CENSUS_ROUTE_LDS>(d, d.loci[locus], locus, lds, threadIdx.x);
}
// route 2: a workgroup per locus, the workspace in a global block
extern "C" __global__ void __launch_bounds__(HS_CENSUS_THREADS) hs_census_global_kernel(const hs_census_dev_t* __restrict__ dp){
  const hs_census_dev_t& d = *dp;
  const int locus = d.list[HS_CENSUS_ROUTE_GLOBAL][blockIdx.x];
  const hs_census_locus_t L = d.loci[locus];
  census_body<HS_CENSUS_ROUTE_GLOBAL>(d, L, locus, d.ws + L.ws_off, threadIdx.x);
}

// candidates in front of every locus: one workgroup; a thread sums a contiguous share of the loci, thread 0 chains the shares
extern "C" __global__ void __launch_bounds__(HS_CENSUS_THREADS) hs_census_scan_kernel(const hs_census_dev_t* __restrict__ dp){
  const hs_census_dev_t& d = *dp;
  __shared__ int part[HS_CENSUS_THREADS];
  const int tid = threadIdx.x;
  const int per = (d.n_loci + HS_CENSUS_THREADS - 1)/HS_CENSUS_THREADS;
  const int l0 = min(d.n_loci, tid*per), l1 = min(d.n_loci, l0 + per);
  int sum = 0;
  for (int l = l0; l < l1; l++) sum += d.cand_count[l];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0){
    int run = 0;
    for (int i = 0; i < HS_CENSUS_THREADS; i++){ const int v = part[i]; part[i] = run; run += v; }
    d.cand_off[d.n_loci] = run;
  }
  __syncthreads();
  int run = part[tid];
  for (int l = l0; l < l1; l++){ d.cand_off[l] = run; run += d.cand_count[l]; }
}

// lanes are the requests of the whole batch: a candidate goes to its position
extern "C" __global__ void __launch_bounds__(HS_CENSUS_THREADS) hs_census_emit_kernel(const hs_census_dev_t* __restrict__ dp){
  const hs_census_dev_t& d = *dp;
  const int64_t Q = (int64_t)blockIdx.x*HS_CENSUS_THREADS + threadIdx.x;
  if (Q >= d.n_req) return;
  const int rank = d.req_rank[Q];
  if (rank < 0) return;
  const int64_t k = (int64_t)d.cand_off[d.req_locus[Q]] + rank;
  if (k < d.cap_cand) d.cand_req[k] = (int32_t)Q;
}

// ---- the trace fields of a resident traceback result (hipstr_post_census_dev)
// The two checks of hipstr_post_census that read the trace's values, one workgroup: the offsets of str_seq (requests are the lanes) and the
// spanning request without STR data (reads are the lanes).  Thread 0 stores what was found and the lowest offending read.
extern "C" __global__ void __launch_bounds__(HS_CENSUS_THREADS) hs_census_check_kernel(const hs_census_dev_t* __restrict__ dp){
  const hs_census_dev_t& d = *dp;
  __shared__ int s_bad, s_read;
  const int tid = threadIdx.x;
  if (tid == 0){ s_bad = 0; s_read = 0x7fffffff; }
  __syncthreads();
  int bad = 0, first = 0x7fffffff;
  if (d.check_offsets && d.n_req > 0){
    for (int q = tid; q < d.n_req; q += HS_CENSUS_THREADS) if (d.str_seq_off[q+1] < d.str_seq_off[q]) bad |= HS_CENSUS_BAD_DECREASE;
    if (tid == 0 && d.str_seq_off[0] < 0) bad |= HS_CENSUS_BAD_NEGATIVE;
    if (tid == 0 && d.str_seq_off[d.n_req] > d.str_total) bad |= HS_CENSUS_BAD_DECREASE;
  }
  for (int r = tid; r < d.n_reads; r += HS_CENSUS_THREADS){
    const int k = d.read_req[r];
    if (k < 0 || d.seed[r] < 0) continue;
    const hs_census_locus_t& L = d.loci[d.req_locus[k]];
    if (d.aln_start[k] < L.blk_start && d.aln_stop[k] > L.blk_end && d.stutter_size[k] == HS_CENSUS_NO_STR_DATA) first = min(first, r);
  }
  first = wave_min_i(first);
  bad = (__ballot((bad & HS_CENSUS_BAD_NEGATIVE) != 0) ? HS_CENSUS_BAD_NEGATIVE : 0) | (__ballot((bad & HS_CENSUS_BAD_DECREASE) != 0) ? HS_CENSUS_BAD_DECREASE : 0);
  if ((tid & 63) == 0){
    if (bad) atomicOr(&s_bad, bad);
    if (first != 0x7fffffff) atomicMin(&s_read, first);
  }
  __syncthreads();
  if (tid == 0){
    d.check[0] = s_bad | (s_read != 0x7fffffff ? HS_CENSUS_BAD_NO_STR : 0);
    d.check[1] = s_read;
  }
}

// The candidates' strings, after hs_census_emit_kernel has fixed cand_req: one workgroup scans the candidates' lengths into cand_seq_off (a
// thread sums a contiguous share, thread 0 chains the shares) — the total is what cap_chars is checked against — then a wavefront per
// candidate copies its bytes from str_seq, a lane per byte.  More candidates than cap_cand: none is looked at (return code 3 either way).
extern "C" __global__ void __launch_bounds__(HS_CENSUS_THREADS) hs_census_gather_kernel(const hs_census_dev_t* __restrict__ dp){
  const hs_census_dev_t& d = *dp;
  __shared__ int64_t part[HS_CENSUS_THREADS];
  __shared__ int64_t total_s;
  const int tid = threadIdx.x;
  const int n_all = d.cand_off[d.n_loci];
  const int n = n_all <= d.cap_cand ? n_all : 0;
  const int per = (n + HS_CENSUS_THREADS - 1)/HS_CENSUS_THREADS;
  const int k0 = min(n, tid*per), k1 = min(n, k0 + per);
  int64_t sum = 0;
  for (int k = k0; k < k1; k++){ const int q = d.cand_req[k]; sum += d.str_seq_off[q+1] - d.str_seq_off[q]; }
  part[tid] = sum;
  __syncthreads();
  if (tid == 0){
    int64_t run = 0;
    for (int i = 0; i < HS_CENSUS_THREADS; i++){ const int64_t v = part[i]; part[i] = run; run += v; }
    total_s = run;
    *d.cand_chars = run;
    d.cand_seq_off[n] = (int32_t)run;
  }
  __syncthreads();
  const int64_t total = total_s;
  int64_t run = part[tid];
  for (int k = k0; k < k1; k++){ const int q = d.cand_req[k]; d.cand_seq_off[k] = (int32_t)run; run += d.str_seq_off[q+1] - d.str_seq_off[q]; }
  if (total > d.cap_chars) return;                          // (the whole workgroup: return code 3)
  __syncthreads();                                          // every candidate's start is written
  const int lane = tid & 63;
  for (int k = tid >> 6; k < n; k += HS_CENSUS_THREADS/64){
    const int q = d.cand_req[k];
    const int from = d.str_seq_off[q], len = d.str_seq_off[q+1] - from;
    const int64_t at = d.cand_seq_off[k];
    for (int i = lane; i < len; i += 64) d.cand_seq[at + i] = d.str_seq[from + i];
  }
}
