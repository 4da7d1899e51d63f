// assign.hip — reads assigned to their sample's MAP haplotypes, per-sample read counts and the traceback request list on gfx950.
//
// SeqStutterGenotyper::write_vcf_record's loop over the reads of a locus (seq_stutter_genotyper.cpp:1079-1157) with the phase totals of
// :1355-1356, and the pick of retrace_alignments (:805-841).  The unit is the posterior stage's (locus, sample) pair; lanes are reads.
// A lane gathers the two likelihoods of its read that matter — the columns of the sample's MAP pair — and evaluates the reference's
// expressions in its operation order (the library is built with -ffp-contract=off); exp / log are the correctly rounded ones of cr_math.h.
// Counters are ballots + population counts.  The log-sum-exp of a sample's phase posteriors (mathops.cpp:64-70) takes the maximum by
// reduction and then adds the exponentials SERIALLY IN READ ORDER: double addition does not reassociate.
//
// Request list: request k is the k-th distinct (locus, pool, haplotype) met in read order — the order trace_cache_ fills in.  A first-occurrence
// table per locus takes an atomic minimum of the read index per key (direct, or hashed by open addressing: where a key lands depends on the
// order the atomics arrive in, the minimum it ends up with does not), a read is a first occurrence when the table holds its own index; the
// distinct keys of a locus are counted on the way (an integer sum: any order), a one-workgroup scan turns the counts into bases, and one
// workgroup per locus walks its reads in order, numbers the first occurrences and hands every read the number of its key.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "post_layout.h"
#include "cr_math.h"

namespace {

__device__ __forceinline__ uint32_t assign_hash(uint32_t key, uint32_t mask){
  uint32_t h = key * 0x9E3779B1u; h ^= h >> 15; h *= 0x85EBCA77u; h ^= h >> 13;
  return h & mask;
}

// slot of `key` in the locus' table; insert: claims one for a key that has none (the slot is found again by every later look-up: linear probing,
// no deletions).  *fresh: this call made the key's entry (exactly one call per key sees it).
__device__ __forceinline__ int assign_slot_insert(int32_t* tab, const hs_assign_locus_t& L, int key, int r, bool* fresh){
  if (!L.hashed){
    const int old = atomicMin(&tab[key], r);
    *fresh = (old == HS_ASSIGN_EMPTY);
    return key;
  }
  const uint32_t mask = (uint32_t)L.slots - 1;
  uint32_t h = assign_hash((uint32_t)key, mask);
  for (;;){
    const int k = atomicCAS(&tab[h], HS_ASSIGN_EMPTY, key);
    if (k == HS_ASSIGN_EMPTY || k == key){
      atomicMin(&tab[L.slots + h], r);
      *fresh = (k == HS_ASSIGN_EMPTY);
      return (int)h;
    }
    h = (h + 1) & mask;
  }
}
__device__ __forceinline__ int assign_slot_find(const int32_t* tab, const hs_assign_locus_t& L, int key){
  if (!L.hashed) return key;
  const uint32_t mask = (uint32_t)L.slots - 1;
  uint32_t h = assign_hash((uint32_t)key, mask);
  while (tab[h] != key) h = (h + 1) & mask;       // (every key looked up was inserted by hs_assign_kernel)
  return (int)h;
}

// WAVES wavefronts per unit: 1 = the workgroup's four wavefronts take a unit each, 4 = the workgroup takes one unit.
template <int WAVES>
__device__ __forceinline__ void assign_body(const hs_assign_dev_t& d){
  constexpr int T = 64*WAVES;                               // lanes of a unit
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = WAVES == 1 ? lane : tid;
  const int64_t ub = WAVES == 1 ? (int64_t)blockIdx.x*(HS_ASSIGN_THREADS/64) + wave : (int64_t)blockIdx.x;
  __shared__ double red_v[HS_ASSIGN_THREADS/64];
  __shared__ int    red_c[8];
  __shared__ double ebuf[HS_ASSIGN_THREADS];
  __shared__ double tot_s;
  const bool live = ub < d.n_units;
  if (WAVES == 1 && !live) return;                          // (a whole wavefront; nothing below synchronises the workgroup in this mode)
  const hs_post_unit_t u = d.units[ub];
  const int A = u.n_alleles, s = u.samp_index;
  const int ul = d.unit_locus[ub], locus = ul >> 1;
  const bool haploid = (ul & 1) != 0;
  const int ha = d.map_gt[2*s], hb = d.map_gt[2*s + 1];
  // a sample without a MAP pair (hs_posterior_kernel: every diplotype -inf / NaN — the reference would index haplotype -1): its reads are skipped
  const bool no_map = ha < 0 || hb < 0;
  const double* LL0 = d.log_aln_probs + u.ll_off;
  const hs_assign_locus_t L = d.loci[locus];
  int32_t* tab = d.tab + L.tab_off;

  int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};                      // the wavefront's counts (uniform over its lanes)
  int n_new = 0;                                            // keys this lane entered into the table
  double lmax = -__builtin_huge_val();
  // ---- per read (seq_stutter_genotyper.cpp:1079-1144)
  for (int r0 = 0; r0 < u.n_reads; r0 += T){
    const int r = r0 + t;
    const bool in = r < u.n_reads;
    const int g = u.read_begin + (in ? r : 0);
    const bool skip = !in || no_map || d.seed[g] < 0;       // :1080
    bool snp = false, s_one = false, uq1 = false, uq2 = false, rv = false;
    if (in && skip){ d.best_hap[g] = -1; d.read_strand[g] = -1; d.read_req[g] = -1; }
    if (!skip){
      const double p1 = d.log_p1[g], p2 = d.log_p2[g];
      const double la = LL0[(int64_t)r*A + ha], lb = LL0[(int64_t)r*A + hb];
      const double x1 = (d.log_half + p1) + la, x2 = (d.log_half + p2) + lb;
      // log_sum_exp(x1, x2), mathops.cpp:52-57
      const double total = (x1 > x2) ? x1 + cr_log(1 + cr_exp(x2 - x1)) : x2 + cr_log(1 + cr_exp(x1 - x2));
      const double lpo = x1 - total;                        // :1091
      d.log_phase_one[g] = lpo;
      lmax = fmax(lmax, lpo);
      int strand = 0;                                       // :1095-1109
      if (!haploid && ((ha != hb) || (fabs(p1 - p2) > 1e-10))){
        const double v1 = p1 + la, v2 = p2 + lb;
        if (fabs(v1 - v2) > d.strand_tolerance){
          strand = (v1 > v2) ? 0 : 1;
          uq1 = strand == 0; uq2 = strand != 0;
          rv = d.reverse != NULL && d.reverse[g] != 0;
        }
      }
      const int best = d.rule == 1 ? ((x1 > x2) ? ha : hb)  // retrace_alignments, :825
                                   : (strand == 0 ? ha : hb);   // write_vcf_record, :1113
      d.best_hap[g] = best; d.read_strand[g] = strand;
      snp = fabs(p1 - p2) > 1e-10; s_one = p1 > p2;         // :1138-1144
      if (d.pool_index){
        bool fresh;
        assign_slot_insert(tab, L, d.pool_index[g]*A + best, g, &fresh);
        n_new += fresh ? 1 : 0;
      }
    }
    c[0] += __popcll(__ballot(!skip));
    c[1] += __popcll(__ballot(snp));
    c[2] += __popcll(__ballot(snp && s_one));
    c[3] += __popcll(__ballot(snp && !s_one));
    c[4] += __popcll(__ballot(uq1));
    c[5] += __popcll(__ballot(uq2));
    c[6] += __popcll(__ballot(uq1 && rv));
    c[7] += __popcll(__ballot(uq2 && rv));
  }
  if (d.pool_index){
    for (int o = 32; o >= 1; o >>= 1) n_new += __shfl_xor(n_new, o);
    if (lane == 0 && n_new) atomicAdd(&d.locus_count[locus], n_new);
  }
  for (int o = 32; o >= 1; o >>= 1) lmax = fmax(lmax, __shfl_xor(lmax, o));
  if (WAVES > 1){
    if (tid < 8) red_c[tid] = 0;
    if (lane == 0) red_v[wave] = lmax;
    __syncthreads();
    if (lane == 0) for (int k = 0; k < 8; k++) if (c[k]) atomicAdd(&red_c[k], c[k]);
    for (int w = 0; w < WAVES; w++) lmax = fmax(lmax, red_v[w]);
    __syncthreads();
    for (int k = 0; k < 8; k++) c[k] = red_c[k];
  }
  // ---- phase totals (:1355-1356): log_sum_exp of the sample's phase posteriors (mathops.cpp:64-70) — the exponentials of the reads that
  // count, added in read order (a skipped read adds +0.0, which leaves a non-negative total as it is, bit for bit)
  double tot = 0.0;
  for (int r0 = 0; r0 < u.n_reads && c[0] > 0; r0 += T){
    const int r = r0 + t;
    const int g = u.read_begin + (r < u.n_reads ? r : 0);
    double e = 0.0;
    if (r < u.n_reads && d.best_hap[g] >= 0) e = cr_exp(d.log_phase_one[g] - lmax);     // (this lane's own stores)
    if (WAVES == 1){
      const int n = min(64, u.n_reads - r0);
      for (int i = 0; i < n; i++) tot += __shfl(e, i);      // every lane the same chain: the total needs no broadcast
    } else {
      ebuf[tid] = e;
      __syncthreads();
      if (tid == 0){
        const int n = min(T, u.n_reads - r0);
        for (int i = 0; i < n; i++) tot += ebuf[i];
      }
      __syncthreads();
    }
  }
  if (WAVES > 1){
    if (tid == 0) tot_s = tot;
    __syncthreads();
    tot = tot_s;
  }
  if (t == 0){
    for (int k = 0; k < 8; k++) d.counters[(int64_t)k*d.n_samp + s] = c[k];
    const double ph1 = c[0] == 0 ? 0.0 : cr_exp(lmax + cr_log(tot));
    d.phase1[s] = ph1;
    d.phase2[s] = (double)c[0] - ph1;
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(HS_ASSIGN_THREADS) hs_assign_kernel(const hs_assign_dev_t* __restrict__ dp){ assign_body<1>(*dp); }
extern "C" __global__ void __launch_bounds__(HS_ASSIGN_THREADS) hs_assign_kernel_wg(const hs_assign_dev_t* __restrict__ dp){ assign_body<HS_ASSIGN_THREADS/64>(*dp); }

// requests in front of every locus and their total: one workgroup; a thread sums a contiguous share of the loci, thread 0 chains the shares
extern "C" __global__ void __launch_bounds__(HS_ASSIGN_THREADS) hs_assign_scan_kernel(const hs_assign_dev_t* __restrict__ dp){
  const hs_assign_dev_t& d = *dp;
  __shared__ int part[HS_ASSIGN_THREADS];
  const int tid = threadIdx.x;
  const int per = (d.n_loci + HS_ASSIGN_THREADS - 1)/HS_ASSIGN_THREADS;
  const int l0 = min(d.n_loci, tid*per), l1 = min(d.n_loci, l0 + per);
  int sum = 0;
  for (int l = l0; l < l1; l++) sum += d.locus_count[l];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0){
    int run = 0;
    for (int i = 0; i < HS_ASSIGN_THREADS; i++){ const int v = part[i]; part[i] = run; run += v; }
    *d.n_req = run;
  }
  __syncthreads();
  int run = part[tid];
  for (int l = l0; l < l1; l++){ d.locus_base[l] = run; run += d.locus_count[l]; }
}

// one workgroup per locus: its reads in order, 256 at a time; first occurrences numbered by a ballot prefix, then every read takes the number of its key
extern "C" __global__ void __launch_bounds__(HS_ASSIGN_THREADS) hs_assign_requests_kernel(const hs_assign_dev_t* __restrict__ dp){
  const hs_assign_dev_t& d = *dp;
  const hs_assign_locus_t L = d.loci[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* tab = d.tab + L.tab_off;
  const int32_t* first = tab + (L.hashed ? L.slots : 0);
  int32_t* reqid = tab + (L.hashed ? 2*(int64_t)L.slots : (int64_t)L.slots);
  __shared__ int wcount[HS_ASSIGN_THREADS/64];
  int base = d.locus_base[blockIdx.x];
  for (int r0 = 0; r0 < L.n_reads; r0 += HS_ASSIGN_THREADS){
    const int r = r0 + tid, g = L.read_begin + r;
    int slot = -1, best = -1, pool = 0;
    bool is_first = false;
    if (r < L.n_reads && (best = d.best_hap[g]) >= 0){
      pool = d.pool_index[g];
      slot = assign_slot_find(tab, L, pool*L.n_alleles + best);
      is_first = first[slot] == g;
    }
    const unsigned long long m = __ballot(is_first);
    if (lane == 0) wcount[wave] = __popcll(m);
    __syncthreads();
    int k = base + __popcll(m & ((1ull << lane) - 1));
    for (int w = 0; w < wave; w++) k += wcount[w];
    int all = 0;
    for (int w = 0; w < HS_ASSIGN_THREADS/64; w++) all += wcount[w];
    base += all;
    if (is_first){
      reqid[slot] = k;
      if (k < d.cap_req){ d.req_read[k] = L.pool_off + pool; d.req_allele[k] = best; }
    }
    __syncthreads();                                        // this chunk's numbers are in the table (and wcount may be written again)
    if (slot >= 0) d.read_req[g] = reqid[slot];             // a key's first read lies in this chunk or an earlier one
  }
}

// Read counts that need the tracebacks, from a resident traceback result (post_layout.h: hs_tstat_*): a wavefront per run of reads of one
// sample, its reads 64 at a time; the per-sample counts are ballots + population counts, added to the sample once per run.
extern "C" __global__ void __launch_bounds__(HS_ASSIGN_THREADS) hs_trace_stats_kernel(const hs_tstat_dev_t* __restrict__ dp){
  const hs_tstat_dev_t& d = *dp;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ub = (int64_t)blockIdx.x*(HS_ASSIGN_THREADS/64) + wave;
  if (ub >= d.n_units) return;                              // (a whole wavefront; nothing below synchronises the workgroup)
  const hs_tstat_unit_t u = d.units[ub];
  const hs_tstat_locus_t L = d.loci[u.locus];
  int n_st = 0, n_fi = 0;                                   // uniform over the lanes
  for (int r0 = 0; r0 < u.n_reads; r0 += 64){
    const int r = r0 + lane;
    const bool in = r < u.n_reads;
    const int g = u.read_begin + (in ? r : 0);
    const int q = in ? d.read_req[g] : -1;                  // a read without a request counts nowhere (:1080)
    bool st = false, fi = false;
    int ml = HS_TSTAT_NO_ML_BP;
    if (q >= 0){
      const int ss = d.stutter_size[q];
      const bool str_data = ss != HS_TSTAT_NO_STR_DATA;
      st = str_data && ss != 0;                             // has_stutter(), AlignmentTraceback.h:79-85
      fi = d.flank_ins[q] != 0 || d.flank_del[q] != 0;      // :1126
      if (d.aln_start[q] < L.start_bound && d.aln_stop[q] > L.stop_bound)      // :1152-1154
        ml = d.allele_bp_diff[L.var_begin + d.hap_to_allele[L.hap_begin + d.best_hap[g]]] + (str_data ? ss : 0);
    }
    if (in) d.ml_bp[g] = ml;
    n_st += __popcll(__ballot(st));
    n_fi += __popcll(__ballot(fi));
  }
  if (lane == 0){
    if (n_st) atomicAdd(&d.n_stutter[u.samp], n_st);
    if (n_fi) atomicAdd(&d.n_flank_indel[u.samp], n_fi);
  }
}
