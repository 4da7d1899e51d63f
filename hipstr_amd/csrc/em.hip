// em.hip — de novo stutter model training on gfx950: EMStutterGenotyper::train (em_stutter_genotyper.cpp:146-226) for a batch
// of loci.
//
// A read is its observed STR size; the "alignment" likelihood of a read given an allele is the stutter pmf, so every O(R·A)
// and O(R·A²) array of the reference is a function of small tables and is recomputed on the fly instead of stored:
//   hs_em_fill        per locus: log_aln_probs[r][a] = log_stutter_pmf(bps[a], bps[obs_r]) (calc_hap_aln_probs, :146-150) and the
//                     allele-frequency diplotype priors, ONE A×A block per locus shared by its samples (:129-144)
//   hs_posterior_kernel  (post_kernels.hip, unchanged arithmetic) = Genotyper::calc_log_sample_posteriors
//   hs_em_mstep       per locus: total LL; recalc_log_gt_priors (:22-57: streaming log-sum-exps, a thread per allele, samples
//                     in order); the seven fast_log_sum_exp reductions of recalc_stutter_model (:64-127) over
//                     (read, allele_1, allele_2, phase), with the read-phase posteriors of :152-169 evaluated in place — the
//                     R×A²×2 array log_read_phase_posteriors_ never exists.  fast_log_sum_exp(vector) is a max and a sum of
//                     float terms, both order-independent, so the reductions are parallel.
// Round 5: the iteration loop is device-resident.  hs_em_finish forms the new parameters and train()'s convergence tests on the device
// (the host did, with three synchronous copies in and two out per lock-step round), with the CORRECTLY ROUNDED exp / log of cr_math.h in
// the reference's operation order — the host libm's bits wherever that is itself correctly rounded, so iteration counts and parameters
// are the CPU run's; hs_em_compact / hs_em_units rebuild the list of loci (and of their (locus, sample) posterior units) that are still
// training, so a late round launches and touches only those; the host enqueues round i + 1 while it waits for the 8-byte count of round
// i - 1 (a bound for the grids, and the stop signal).  HIPSTR_EM_HOST_LOOP=1 selects the round-4 loop (host libm, all loci per round).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <chrono>
#include <sched.h>
#include <unistd.h>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "post_layout.h"
#include "em_layout.h"
#include "prep.h"
#include "api_internal.h"
#include "cr_math.h"
#include "float_lse.h"

extern "C" __global__ void hs_posterior_kernel(const hs_post_dev_t* dp);

struct hs_em_locus_t {
  int32_t A, S, R, period, haploid;
  int32_t read_begin;      // into the per-read arrays
  int32_t samp_begin;      // into sample_total
  int32_t bps_off;         // into bps / log_gt_priors (A entries)
  int64_t post_off;        // S*A*A posteriors
  int64_t ll_off;          // R*A log_aln_probs
  int64_t prior_off;       // A*A priors
  int64_t sa_off;          // S*A per-(sample, allele) values (gmax)
};

struct hs_em_dev_t {
  const hs_em_locus_t* loci;
  const int32_t* active;       // [n_loci]
  const double*  logp;         // [9*n_loci] in_step, in_nostep, in_up, in_down, out_step, out_nostep, out_up, out_down, log_equal
  const int32_t* bps;          // allele sizes
  const int32_t* obs;          // [n_reads] allele index of the read's size
  const int32_t* sample_label; // [n_reads]
  const double*  log_p1;
  const double*  log_p2;
  double*  gtp;                // log_gt_priors_, same offsets as bps
  double*  ll;                 // log_aln_probs
  double*  prior;
  const double*  post;
  const double*  sample_total;
  const double*  int_log;
  double*  new_ll;             // [n_loci]
  double*  sums;               // [7*n_loci] in_up, in_down, in_eq, in_diffs, out_up, out_down, out_diffs
  double*  row_lse;            // scratch: log_sum_exp of every posterior row (s, allele_1); a locus uses [post_off, post_off + S*A)
  int32_t* cat;                // [R*A per locus, at ll_off] what a read of this size says about the stutter model if it came from this allele:
                               //   category (0 in_up, 1 in_down, 2 in_eq, 4 out_up, 5 out_down) | diffs vector (3 in, 6 out, 255 none) << 8
  double*  leff;               // same layout: ln |effective difference| (the addend of the diffs vectors), 0 where there is none
  double*  part;               // [n_loci][HS_EM_PARTS][7] partial maxima, then partial sums, of the seven M-step vectors
  unsigned long long* dbg;     // HIPSTR_TIMING: [0..1] rows listed / rows scanned in the maxima pass, [2..3] in the sums pass
  double*  gmax;               // [S*A per locus, at sa_off] largest log posterior of any diplotype of the sample that holds the allele (hs_em_gmax)
  double   log_thresh, log_half, log_1p1;
  // ---- device-resident loop (NULL / unused with the host loop): workgroup b of a per-locus kernel takes locus list[b] if b < counts[0]
  const int32_t* list;         // loci still training, ascending
  const int32_t* counts;       // [0] loci in `list`, [1] their (locus, sample) units
  int32_t* next_list;          // the lists of the next round (hs_em_compact / hs_em_units write them; the two argument blocks swap roles)
  int32_t* next_counts;
  int32_t* next_units;         // (locus, sample) units of the loci in next_list, in order
  int32_t* next_unit_begin;    // [n_loci] scratch: first slot of a listed locus' units in next_units
  const int32_t* unit_first;   // [n_loci] index of the locus' first unit
  double*  logp_rw;            // = logp, writable (hs_em_finish writes the next round's nine logs)
  double*  sp;                 // [6*n_loci] current stutter parameters
  double*  cur_ll;             // [n_loci] LL of the previous round (-DBL_MAX before the first)
  int32_t* iter;               // [n_loci] 1-based number of the round a locus is in
  int32_t* state;              // [n_loci] 0 training, 1 converged (train() returned true), 2 out of iterations (false)
  int32_t* n_iter;             // [n_loci] outputs: rounds run, LL of the last one
  double*  final_ll;
  int32_t  max_iter, n_loci;
  double   min_abs, min_frac;
};
// the locus of this workgroup: through the active list (device loop) or the mask (host loop); -1 = nothing to do
__device__ __forceinline__ int em_locus(const hs_em_dev_t& d){
  if (d.list) return ((int)blockIdx.x < d.counts[0]) ? d.list[blockIdx.x] : -1;
  return d.active[blockIdx.x] ? (int)blockIdx.x : -1;
}
// (the sizes every kernel below is cut by — HS_EM_PARTS, HS_EM_TILE, HS_EM_CHUNK, HS_EM_MAXA_LDS ... — and the decisions taken from them: em_layout.h)

namespace {

// (the float log-sum-exp primitives — f_fasterexp / f_fasterlog, fast_lse2 — for device and host: float_lse.h)

// StutterModel::log_stutter_pmf (stutter_model.cpp:29-53) from the nine logs the constructor keeps (stutter_model.h:44-58)
__device__ __forceinline__ double em_pmf(const double* lp, int period, int sample_bps, int read_bps){
  const int diff = read_bps - sample_bps;
  if (diff % period != 0){
    const int eff = diff - diff/period;
    return eff < 0 ? (lp[7] + lp[5]) + lp[4]*(double)(-eff-1) : (lp[6] + lp[5]) + lp[4]*(double)(eff-1);
  }
  const int rep = diff/period;
  if (rep == 0) return lp[8];
  return rep < 0 ? (lp[3] + lp[1]) + lp[0]*(double)(-rep-1) : (lp[2] + lp[1]) + lp[0]*(double)(rep-1);
}

__global__ void __launch_bounds__(256) hs_em_fill(const hs_em_dev_t* __restrict__ dp){
  const hs_em_dev_t& d = *dp;
  const int l = em_locus(d);
  if (l < 0) return;
  const hs_em_locus_t L = d.loci[l];
  const double* lp = d.logp + 9*l;
  const int32_t* bps = d.bps + L.bps_off;
  const double* gtp = d.gtp + L.bps_off;
  const int A = L.A;
  for (int x = threadIdx.x; x < L.R*A; x += 256){
    const int r = x / A, a = x - r*A;
    const int ob = bps[d.obs[L.read_begin + r]];
    d.ll[L.ll_off + x] = em_pmf(lp, L.period, bps[a], ob);
    // recalc_stutter_model's bookkeeping for (read, source allele) (:76-104): it does not depend on the iteration, but it is cheap
    // next to the pmf and keeps the M-step free of integer divisions
    const int bd = ob - bps[a];
    int cat = 2, dcat = 255; double le = 0.0;
    if (bd != 0){
      if (bd % L.period != 0){ const int eff = bd - bd/L.period; cat = bd > 0 ? 4 : 5; dcat = 6; le = d.int_log[abs(eff)]; }
      else { const int eff = bd/L.period; cat = bd > 0 ? 0 : 1; dcat = 3; le = d.int_log[abs(eff)]; }
    }
    d.cat[L.ll_off + x] = cat | (dcat << 8);
    d.leff[L.ll_off + x] = le;
  }
  for (int x = threadIdx.x; x < A*A; x += 256){          // EMStutterGenotyper::init_log_sample_priors (:129-144)
    const int i1 = x / A, i2 = x - i1*A;
    d.prior[L.prior_off + x] = !L.haploid ? gtp[i1] + gtp[i2] : (i1 == i2 ? gtp[i1] : -DBL_MAX/2);
  }
}

// block reductions over 256 threads
__device__ __forceinline__ double block_max(double v, double* red){
  const int tid = threadIdx.x;
  red[tid] = v; __syncthreads();
  for (int s = 128; s > 0; s >>= 1){ if (tid < s) red[tid] = fmax(red[tid], red[tid+s]); __syncthreads(); }
  const double out = red[0]; __syncthreads();
  return out;
}
__device__ __forceinline__ double block_sum(double v, double* red){
  const int tid = threadIdx.x;
  red[tid] = v; __syncthreads();
  for (int s = 128; s > 0; s >>= 1){ if (tid < s) red[tid] += red[tid+s]; __syncthreads(); }
  const double out = red[0]; __syncthreads();
  return out;
}

// recalc_log_gt_priors (:22-57) of one locus by one workgroup: thread a owns allele a; the two scans in the reference's order.
// Independent of the stutter reductions, so it rides in their first launch as one more slice (blockIdx.y == HS_EM_PARTS).
__device__ void em_gt_priors(const hs_em_dev_t& d, const hs_em_locus_t& L, int tid){
#ifdef HS_EM_TIME
  unsigned long long tk0 = __builtin_amdgcn_s_memtime(), tk1 = 0, tk2 = 0, tkA = 0, tkB = 0;
#endif
  const int A = L.A, S = L.S;
  const double* post = d.post + L.post_off;
  double* gtp = d.gtp + L.bps_off;
  // log_sum_exp of every row (sample, allele_1) first, all rows in parallel (each row summed in allele_2 order as the reference does);
  // the streaming scans below are sequential per allele by definition
  double* row_lse = d.row_lse + L.post_off;     // S*A values in this locus' own S*A*A region: disjoint between loci whatever their A
  // The rows are fetched a tile at a time into LDS, contiguously (a thread walking its own row straight from memory touches 64 cache lines
  // per load: the kernel was bound by exactly that), then: a thread per row takes the maximum, ALL threads form the exponentials in place,
  // a thread per row adds them in allele order and takes the logarithm.
  extern __shared__ double hs_em_dyn[];
  {
    const int Ap = hs_em_row_stride(A);                  // odd row stride: the per-row walks of neighbouring threads fall into different banks
    const int tile_rows = hs_em_row_tile_rows(A);
    __shared__ double s_rm[256];
    __shared__ int s_fm[256];
    if (tile_rows >= 1){
      for (int x0 = 0; x0 < S*A; x0 += tile_rows){
        const int nr = min(tile_rows, S*A - x0);
        for (int e = tid; e < nr*A; e += 256){ const int rr = e / A, j = e - rr*A; hs_em_dyn[rr*Ap + j] = post[(int64_t)x0*A + e]; }
        __syncthreads();
        if (tid < nr){
          const double* row = hs_em_dyn + tid*Ap;
          double rm = row[0]; int fm = 0;
          for (int j = 1; j < A; j++) if (row[j] > rm){ rm = row[j]; fm = j; }
          s_rm[tid] = rm; s_fm[tid] = fm;
        }
        __syncthreads();
        // (behind the row's first maximum the running total is >= 1: a term below 2^-54 leaves it as it is and is not formed — +0.0 instead)
        for (int e = tid; e < nr*A; e += 256){
          const int rr = e / A, j = e - rr*A;
          const double x_ = hs_em_dyn[rr*Ap + j] - s_rm[rr];
          hs_em_dyn[rr*Ap + j] = (j > s_fm[rr] && x_ < HS_EM_TERM_FLOOR) ? 0.0 : cr_exp(x_);
        }
        __syncthreads();
        if (tid < nr){
          __builtin_amdgcn_s_setprio(3);
          const double* row = hs_em_dyn + tid*Ap;
          double rs = 0.0;
          for (int j = 0; j < A; j++) rs += row[j];
          row_lse[x0 + tid] = s_rm[tid] + cr_log(rs);
          __builtin_amdgcn_s_setprio(0);
        }
        __syncthreads();
      }
    } else {                                             // a row does not fit the tile (thousands of alleles): straight from memory
      for (int x = tid; x < S*A; x += 256){
        const double* row = post + (int64_t)x*A;
        double rm = row[0];
        for (int j = 1; j < A; j++) rm = fmax(rm, row[j]);
        double rs = 0.0;
        for (int j = 0; j < A; j++) rs += cr_exp(row[j] - rm);
        row_lse[x] = rm + cr_log(rs);
      }
    }
  }
  __syncthreads();
#ifdef HS_EM_TIME
  tk1 = __builtin_amdgcn_s_memtime();
#endif
  // The two scans of allele a are ONE dependent chain over S + S A values (update_streaming_log_sum_exp, mathops.cpp:72-80): lane a owns it.
  // What is expensive in a step is the exponential — of (value - running maximum) where the value does not exceed the maximum, of
  // (old maximum - value) where it becomes the new one — and the running maximum in front of every step is a prefix maximum of the values
  // alone: it does not depend on the sums.  So the values are taken HS_EM_CHUNK at a time in four phases: (1) all threads put the chunk's
  // values into LDS, (2) lane a walks its chunk once for the maximum in front of every step (a compare per step), (3) ALL threads form
  // the step's exponential with that maximum (correctly rounded, cr_math.h; a term that cannot change a total >= 1 is marked instead),
  // (4) lane a walks its chunk again: an addition per step, a multiplication and an addition where the maximum moves.  Same values,
  // same operations in the same order as the scalar chain, and no exponential inside the dependent chain (until round 5 a lane whose
  // maximum had moved inside a chunk evaluated the rest of the chunk the long way — with 33 chains side by side in one wavefront nearly
  // every step of the walk paid for somebody's exponential: ~540 cycles per step).  (A > 64: alleles beyond the first wavefront's lanes loop.)
  constexpr int CH = HS_EM_CHUNK;
  constexpr int NE = (CH*HS_EM_MAXA_LDS + 255)/256;      // a thread's share of a chunk's (position, allele) pairs
  double* const Ebuf = hs_em_dyn;                         // [CH][na]: the maximum in front of the step, then the step's exponential
  double* const Vbuf = hs_em_dyn + CH*HS_EM_MAXA_LDS;    // [CH][na]: the values (the walks are dependent chains and must not wait for L2 at every step)
  const int64_t n1 = S, ntot = hs_em_chain_len(S, A);
  for (int a0 = 0; a0 < A; a0 += HS_EM_MAXA_LDS){
    const int na = hs_em_sweep_alleles(A, a0);
    double m = -DBL_MAX/2, t = 0.0;                      // lane a - a0 < na of the first wavefront: the chain's state
    // a thread's pairs are the same in every chunk: position i (of the chunk) and allele al of pair e = tid + 256 q
    int pi[NE], pidx[NE];
#pragma unroll
    for (int q = 0; q < NE; q++){ const int e = tid + 256*q; const int i = e / na; pi[q] = i; pidx[q] = i*na + (e - i*na); }
    double nxt[NE];
    auto fetch = [&](int64_t c0){                        // this thread's share of the chunk at c0: requested here, used after the next barrier but one
      const int cn = hs_em_chunk_len(ntot, c0);
#pragma unroll
      for (int q = 0; q < NE; q++) if (pi[q] < cn){
        const int64_t ci = c0 + pi[q]; const int a = a0 + (pidx[q] - pi[q]*na);
        nxt[q] = ci < n1 ? row_lse[ci*A + a] : post[(ci - n1)*A + a];      // the chain of allele a: row_lse(s, a) for s < S, then post[(s, i1), a]
      }
    };
    fetch(0);
    for (int64_t c0 = 0; c0 < ntot; c0 += CH){
      const int cn = hs_em_chunk_len(ntot, c0);
#pragma unroll
      for (int q = 0; q < NE; q++) if (pi[q] < cn) Vbuf[pidx[q]] = nxt[q];
      __syncthreads();
#ifdef HS_EM_TIME
      const unsigned long long ta = __builtin_amdgcn_s_memtime();
#endif
      if (tid < na){                                     // (2) the maximum in front of every step
        __builtin_amdgcn_s_setprio(3);                   // the workgroup waits for this one wavefront's chain: it goes first whenever it is ready
        double mr = m;
        for (int i0 = 0; i0 < cn; i0 += 8){
          double lvv[8];
#pragma unroll
          for (int q = 0; q < 8; q++) lvv[q] = Vbuf[min(i0 + q, cn - 1)*na + tid];
#pragma unroll
          for (int q = 0; q < 8; q++){
            if (i0 + q >= cn) break;
            Ebuf[(i0 + q)*na + tid] = mr;
            mr = (lvv[q] > mr) ? lvv[q] : mr;            // (the walk below moves its maximum by the same test)
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
#ifdef HS_EM_TIME
      tkB += __builtin_amdgcn_s_memtime() - ta;
#endif
      __syncthreads();
      if (c0 + CH < ntot) fetch(c0 + CH);                // the next chunk's values travel while this chunk's exponentials are formed
#pragma unroll
      for (int q = 0; q < NE; q++) if (pi[q] < cn){      // (3)
        const double lv = Vbuf[pidx[q]], mb = Ebuf[pidx[q]];
        double ex;
        if (lv <= mb){ const double x_ = lv - mb; ex = (x_ < HS_EM_TERM_FLOOR) ? -1.0 : cr_exp(x_); }       // -1: "below 2^-54" (see the walk)
        else ex = cr_exp(mb - lv);                        // the factor of the total gathered under the old maximum
        Ebuf[pidx[q]] = ex;
      }
      __syncthreads();
#ifdef HS_EM_TIME
      const unsigned long long tb = __builtin_amdgcn_s_memtime();
#endif
      if (tid < na){                                     // (4)
        __builtin_amdgcn_s_setprio(3);
        // eight steps' operands are fetched together, ahead of the (dependent) chain: a step that waited for its own two LDS reads took ~400 cycles
        for (int i0 = 0; i0 < cn; i0 += 8){
          double lvv[8], exv[8];
#pragma unroll
          for (int q = 0; q < 8; q++){
            const int i = min(i0 + q, cn - 1);
            lvv[q] = Vbuf[i*na + tid]; exv[q] = Ebuf[i*na + tid];
          }
#pragma unroll
          for (int q = 0; q < 8; q++){
            if (i0 + q >= cn) break;
            const double lv = lvv[q];
            if (lv <= m){
              // (once a maximum is set the total is >= 1: a term below 2^-54 leaves it as it is, bit for bit; before that — t < 1 only while
              //  m is still the initial -DBL_MAX/2, where no value is below it — it cannot occur)
              if (exv[q] >= 0.0) t += exv[q];
            } else { t *= exv[q]; t += 1.0; m = lv; }
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
#ifdef HS_EM_TIME
      tkB += __builtin_amdgcn_s_memtime() - tb;
#endif
      __syncthreads();
    }
    if (tid < na) gtp[a0 + tid] = m + cr_log(t);
    __syncthreads();
  }
#ifdef HS_EM_TIME
  tk2 = __builtin_amdgcn_s_memtime();
  if (tid == 0 && (blockIdx.x % 2000) == 7) printf("gt_priors locus %d A %d S %d: rows %llu  scans %llu (walks %llu)\n", (int)blockIdx.x, A, S, tk1 - tk0, tk2 - tk1, tkB);
#endif
  if (tid == 0){                                          // normalise: exact log_sum_exp in allele order
    double m = gtp[0];
    for (int a = 1; a < A; a++) m = fmax(m, gtp[a]);
    double t = 0.0;
    for (int a = 0; a < A; a++) t += cr_exp(gtp[a] - m);
    const double lt = m + cr_log(t);
    for (int a = 0; a < A; a++) gtp[a] -= lt;
  }
}

// gmax[s][a] = the largest log posterior among the diplotypes (a, j) and (j, a) of sample s: the bound hs_em_mstep_part prunes by.
// A wavefront per sample, lanes = the second allele: every row of the sample's A x A block is read once, contiguously (a thread per
// (sample, allele) walking its row and its column touched 64 cache lines per load: 15 ms per round of 10 000 loci, now ~1).
__global__ void __launch_bounds__(256) hs_em_gmax(const hs_em_dev_t* __restrict__ dp){
  const hs_em_dev_t& d = *dp;
  const int l = em_locus(d);
  if (l < 0) return;
  const hs_em_locus_t L = d.loci[l];
  const int A = L.A, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double* post = d.post + L.post_off;
  double* g = d.gmax + L.sa_off;
  if (hs_em_gmax_wave(A)){
    for (int s_ = w; s_ < L.S; s_ += HS_EM_GMAX_WAVES){
      const double* gp = post + (int64_t)s_*A*A;
      double colmax = -DBL_MAX, mine = -DBL_MAX;              // lane j: max over a of gp[a][j];  lane a: max over j of gp[a][j]
      for (int a = 0; a < A; a++){
        const double v = (lane < A) ? gp[a*A + lane] : -DBL_MAX;
        colmax = fmax(colmax, v);
        double rm = v;
        for (int o = 32; o >= 1; o >>= 1) rm = fmax(rm, __shfl_xor(rm, o));
        if (lane == a) mine = rm;
      }
      if (lane < A) g[s_*A + lane] = fmax(colmax, mine);
    }
  } else {
    for (int x = threadIdx.x; x < L.S*A; x += 256){
      const int s_ = x / A, a = x - s_*A;
      const double* gp = post + (int64_t)s_*A*A;
      double m = gp[a*A];
      for (int j = 0; j < A; j++) m = fmax(m, fmax(gp[a*A + j], gp[j*A + a]));
      g[x] = m;
    }
  }
}

// recalc_stutter_model (:64-127): seven log-sum-exps over factor = log P(diplotype | sample) + log P(phase | read, diplotype), one term per
// (read, diplotype, phase) — R x A^2 x 2 of them, the only large loop of the EM.  fast_log_sum_exp needs the maximum first, so the loop
// runs twice, as two kernels; each locus is cut into HS_EM_PARTS slices (one workgroup each) whose partial maxima / partial sums are
// combined afterwards: a maximum is order-independent, and the sums are sums of float terms taken in double, exact in any order.
//   PASS 0: part[l][k][0..6] = maxima of slice k;  hs_em_mstep_keepmax: keep[l][0..6] = their maximum (with the pseudocount entries, :69-71);
//   PASS 1: part[l][k][0..6] = sums of slice k relative to keep[l]
template <int PASS>
__global__ void __launch_bounds__(256) hs_em_mstep_part(const hs_em_dev_t* __restrict__ dp, const double* __restrict__ keep){
  const hs_em_dev_t& d = *dp;
  const int l = em_locus(d), k_part = blockIdx.y, tid = threadIdx.x;
  if (l < 0) return;
  const hs_em_locus_t L = d.loci[l];
  const int A = L.A, nd = A*A;
  const double* post = d.post + L.post_off;
  const double* ll = d.ll + L.ll_off;
  const int32_t* catv = d.cat + L.ll_off;
  const double* leff = d.leff + L.ll_off;
  double* part = d.part + ((size_t)l*HS_EM_PARTS)*7;
  __shared__ double red[256];
  double mx[7];
  if (PASS == 1) for (int k = 0; k < 7; k++) mx[k] = keep[7*l + k];      // the maxima over all slices and the pseudocount entries (hs_em_mstep_keepmax)
  double acc[7];
  for (int k = 0; k < 7; k++) acc[k] = (PASS == 0) ? ((k == 3 || k == 6) ? d.log_1p1 : 0.0) : 0.0;
  // A thread owns (read r, source allele a) and walks the other allele j: both phases' terms with source a — phase 0 of diplotype
  // (a, j) and phase 1 of (j, a) — feed the same two vectors (the category and diffs vector of (r, a), hs_em_fill), so the
  // seven-way choice is made once per (r, a) and the walk itself is branch-free.
  const int total = L.R*A;
  const int x0 = hs_em_slice_begin(total, k_part), x1 = hs_em_slice_begin(total, k_part + 1);
  // Round 5: most (read, source allele) rows cannot matter and are recognised without walking them.  Every term of a row is
  //   f = log P(diplotype | sample) + log P(phase | read, diplotype)  <=  G + c,   G = gmax[sample][a] (hs_em_gmax: the sample's best diplotype
  // that holds allele a), c = 4e-6 (the phase term is <= 0 up to the float log-sum-exp's approximation error: its bit-trick log dips to
  // -1.65e-6 at 1.0, fastonebigheader.h:320-338), and every operation between f and its use is monotone in f.  So
  //   PASS 0: a row whose bound cannot exceed the pseudocount entries every vector starts from (0, ln 1.1) cannot raise a maximum;
  //   PASS 1: a row whose bound is not above max + LOG_THRESH only has terms the threshold drops (mathops.cpp:102-103)
  // — and neither is walked.  The rows that are left (a few per cent: the alleles of a read's sample's plausible genotypes) are gathered
  // into a list per tile of HS_EM_TILE rows, so that the walk keeps every lane busy.  Same maxima, same sums (of float terms, in double:
  // exact in any order).
  const double* gmax = d.gmax + L.sa_off;
  constexpr double PH_C = HS_EM_PRUNE_C;
  __shared__ int s_rows[HS_EM_TILE];
  __shared__ int s_cnt;
  for (int t0 = x0; t0 < x1; t0 += HS_EM_TILE){
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const int t1 = min(x1, t0 + HS_EM_TILE);
    for (int x = t0 + tid; x < t1; x += 256){
      const int r = x / A, a = x - r*A;
      const double Gb = gmax[(int64_t)d.sample_label[L.read_begin + r]*A + a] + PH_C;
      const int c2 = catv[x];
      const int cat = c2 & 0xff, dcat = c2 >> 8;
      const double le = leff[x];
      bool need;
      if (PASS == 0){
        need = Gb > 0.0;                                                   // (vectors 0, 1, 2, 4, 5 start from the pseudocount entry 0.0)
        if (dcat < 7) need = need || (Gb + le > d.log_1p1);                // (the diffs vectors from ln 1.1)
      } else {
        double mc = 0.0, md = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++){ if (k == cat) mc = mx[k]; if (k == dcat) md = mx[k]; }
        need = (Gb - mc > d.log_thresh);
        if (dcat < 7) need = need || ((Gb + le) - md > d.log_thresh);
      }
      if (need) s_rows[atomicAdd(&s_cnt, 1)] = x;
    }
    __syncthreads();
    const int n_live = s_cnt;
    if (d.dbg && tid == 0){ atomicAdd(d.dbg + 2*PASS, (unsigned long long)n_live); atomicAdd(d.dbg + 2*PASS + 1, (unsigned long long)(t1 - t0)); }
    for (int li = tid; li < n_live; li += 256){
      const int x = s_rows[li];
    const int r = x / A, a = x - r*A;
    const int g = L.read_begin + r;
    // recalc_log_read_phase_posteriors (:152-169); the pmf values are the E-step's log_aln_probs
    const double b1 = d.log_half + d.log_p1[g], b2 = d.log_half + d.log_p2[g];
    const double one_a = b1 + ll[x], two_a = b2 + ll[x];
    const double* gp = post + (int64_t)d.sample_label[g]*nd;
    const double* llr = ll + r*A;
    const int c2 = catv[x];
    const int cat = c2 & 0xff, dcat = c2 >> 8;
    const double le = leff[x];
    const bool same = (b1 == b2);                         // no phasing information: the two mixtures of a pair are the same number
    if (PASS == 0){
      double m = -DBL_MAX;
      for (int j = 0; j < A; j++){
        const double lj = llr[j];
        const double both0 = fast_lse2(one_a, b2 + lj, d.log_thresh);                         // diplotype (a, j)
        const double both1 = same ? both0 : fast_lse2(b1 + lj, two_a, d.log_thresh);          // diplotype (j, a)
        m = fmax(m, fmax(gp[a*A + j] + (one_a - both0), gp[j*A + a] + (two_a - both1)));
      }
      const double md = m + le;                           // adding one number keeps the order: max(f) + le == max(f + le)
#pragma unroll
      for (int k = 0; k < 7; k++){
        if (k == cat) acc[k] = fmax(acc[k], m);
        if (k == dcat) acc[k] = fmax(acc[k], md);
      }
    } else {
      double mc = 0.0, md = 0.0;
#pragma unroll
      for (int k = 0; k < 7; k++){ if (k == cat) mc = mx[k]; if (k == dcat) md = mx[k]; }
      const bool has_d = dcat < 7;
      double sc = 0.0, sd = 0.0;
      for (int j = 0; j < A; j++){
        const double lj = llr[j];
        const double both0 = fast_lse2(one_a, b2 + lj, d.log_thresh);
        const double both1 = same ? both0 : fast_lse2(b1 + lj, two_a, d.log_thresh);
        const double f0 = gp[a*A + j] + (one_a - both0), f1 = gp[j*A + a] + (two_a - both1);
        { const double df = f0 - mc; if (df > d.log_thresh) sc += (double)f_fasterexp((float)df); }
        { const double df = f1 - mc; if (df > d.log_thresh) sc += (double)f_fasterexp((float)df); }
        if (has_d){
          { const double df = (f0 + le) - md; if (df > d.log_thresh) sd += (double)f_fasterexp((float)df); }
          { const double df = (f1 + le) - md; if (df > d.log_thresh) sd += (double)f_fasterexp((float)df); }
        }
      }
#pragma unroll
      for (int k = 0; k < 7; k++){
        if (k == cat) acc[k] += sc;
        if (k == dcat) acc[k] += sd;
      }
    }
      }
    __syncthreads();
  }
  double out[7];
  for (int k = 0; k < 7; k++) out[k] = (PASS == 0) ? block_max(acc[k], red) : block_sum(acc[k], red);
  if (tid == 0) for (int k = 0; k < 7; k++) part[k_part*7 + k] = out[k];
}

// recalc_log_gt_priors of every active locus: long dependent scans on a few lanes.  Nothing in the stutter reductions needs their result
// (the next iteration's hs_em_fill does), so the kernel runs beside them on a second stream.
__global__ void __launch_bounds__(256) hs_em_gt_priors(const hs_em_dev_t* __restrict__ dp){
  const hs_em_dev_t& d = *dp;
  const int l = em_locus(d);
  if (l < 0) return;
  const hs_em_locus_t L = d.loci[l];
  em_gt_priors(d, L, threadIdx.x);
}

__global__ void __launch_bounds__(64) hs_em_mstep_keepmax(const hs_em_dev_t* __restrict__ dp, double* __restrict__ keep){
  const hs_em_dev_t& d = *dp;
  const int l = em_locus(d);
  if (l < 0 || threadIdx.x >= 7) return;
  const double* part = d.part + ((size_t)l*HS_EM_PARTS)*7;
  double m = (threadIdx.x == 3 || threadIdx.x == 6) ? d.log_1p1 : 0.0;
  for (int q = 0; q < HS_EM_PARTS; q++) m = fmax(m, part[q*7 + threadIdx.x]);
  keep[7*l + threadIdx.x] = m;
}

__global__ void __launch_bounds__(256) hs_em_mstep(const hs_em_dev_t* __restrict__ dp, const double* __restrict__ keep){
  const hs_em_dev_t& d = *dp;
  const int l = em_locus(d), tid = threadIdx.x;
  if (l < 0) return;
  const hs_em_locus_t L = d.loci[l];
  const int S = L.S;

  // total log-likelihood of the E-step: sum of the sample totals in sample order (genotyper.cpp:75)
  if (tid == 0){
    double t = 0.0;
    for (int s = 0; s < S; s++) t += d.sample_total[L.samp_begin + s];
    d.new_ll[l] = t;
  }
  if (tid == 0){
    const double* part = d.part + ((size_t)l*HS_EM_PARTS)*7;
    for (int k = 0; k < 7; k++){
      const double mxk = keep[7*l + k];
      double t = 0.0;
      for (int q = 0; q < HS_EM_PARTS; q++) t += part[q*7 + k];
      // the pseudocount entries: 0.0 in every vector, ln 1.1 in the two diffs vectors
      { const double df = 0.0 - mxk; if (df > d.log_thresh) t += (double)f_fasterexp((float)df); }
      if (k == 3 || k == 6){ const double df = d.log_1p1 - mxk; if (df > d.log_thresh) t += (double)f_fasterexp((float)df); }
      d.sums[7*l + k] = mxk + (double)f_fasterlog((float)t);
    }
  }
}

// ---- the device-resident loop (round 5) ---------------------------------------------------------------------------------
// StutterModel's nine logs (stutter_model.h:44-58) from the six parameters, correctly rounded
__device__ __forceinline__ void em_logs(const double* sp, double* q){
  q[0] = cr_log(1-sp[0]); q[1] = cr_log(sp[0]); q[2] = cr_log(sp[1]); q[3] = cr_log(sp[2]);
  q[4] = cr_log(1-sp[3]); q[5] = cr_log(sp[3]); q[6] = cr_log(sp[4]); q[7] = cr_log(sp[5]);
  q[8] = cr_log(1-sp[1]-sp[2]-sp[4]-sp[5]);
}
__device__ __forceinline__ double em_lse2_exact(double a, double b){      // mathops.cpp:52-57
  return a > b ? a + cr_log(1 + cr_exp(b - a)) : b + cr_log(1 + cr_exp(a - b));
}

// init_stutter_model (:59-62) and the loop's starting state, a thread per locus
__global__ void __launch_bounds__(HS_EM_INIT_THREADS) hs_em_init(const hs_em_dev_t* __restrict__ dp){
  const hs_em_dev_t& d = *dp;
  const int l = blockIdx.x*HS_EM_INIT_THREADS + threadIdx.x;
  if (l >= d.n_loci) return;
  const double init[6] = { 0.9, 0.1, 0.1, 0.8, 0.01, 0.01 };
  for (int k = 0; k < 6; k++) d.sp[6*l + k] = init[k];
  em_logs(init, d.logp_rw + 9*(size_t)l);
  d.cur_ll[l] = -DBL_MAX; d.iter[l] = 1; d.n_iter[l] = 0; d.final_ll[l] = 0.0;
  d.state[l] = (1 > d.max_iter) ? 2 : 0;                  // no iteration allowed: train() returns false without running one
}

// The end of a round for one locus (a thread): the E-step's total LL and the seven M-step totals (what hs_em_mstep hands the host loop),
// then train()'s tests and update (:186-224) in the reference's order, exp / log correctly rounded, and the next round's nine logs.
__global__ void __launch_bounds__(64) hs_em_finish(const hs_em_dev_t* __restrict__ dp, const double* __restrict__ keep){
  const hs_em_dev_t& d = *dp;
  const int l = em_locus(d);
  if (l < 0 || threadIdx.x != 0) return;
  const hs_em_locus_t L = d.loci[l];
  double new_LL = 0.0;
  for (int s = 0; s < L.S; s++) new_LL += d.sample_total[L.samp_begin + s];     // genotyper.cpp:75
  double t[7];
  const double* part = d.part + ((size_t)l*HS_EM_PARTS)*7;
  for (int k = 0; k < 7; k++){
    const double mxk = keep[7*l + k];
    double tt = 0.0;
    for (int q = 0; q < HS_EM_PARTS; q++) tt += part[q*7 + k];
    { const double df = 0.0 - mxk; if (df > d.log_thresh) tt += (double)f_fasterexp((float)df); }
    if (k == 3 || k == 6){ const double df = d.log_1p1 - mxk; if (df > d.log_thresh) tt += (double)f_fasterexp((float)df); }
    t[k] = mxk + (double)f_fasterlog((float)tt);
  }
  const int it = d.iter[l];
  d.n_iter[l] = it; d.final_ll[l] = new_LL;
  const double LL = d.cur_ll[l];
  if (new_LL < LL + 1e-10){ d.state[l] = 1; return; }                           // :190-194 (TOLERANCE = 1e-10)
  const double out_total = fast_lse2(t[4], t[5], d.log_thresh);
  const double in_pgeom  = fmin(0.999, cr_exp(em_lse2_exact(t[0], t[1]) - t[3]));
  const double out_pgeom = fmin(0.999, cr_exp(out_total - t[6]));
  const double m3 = fmax(fmax(t[0], t[1]), t[2]);
  const double lse3 = m3 + cr_log(cr_exp(t[0]-m3) + cr_exp(t[1]-m3) + cr_exp(t[2]-m3));      // mathops.cpp:59-62
  const double log_total = em_lse2_exact(lse3, out_total);
  const double nw[6] = { in_pgeom, cr_exp(t[0] - log_total), cr_exp(t[1] - log_total), out_pgeom, cr_exp(t[4] - log_total), cr_exp(t[5] - log_total) };
  const double abs_change = new_LL - LL, frac_change = -(new_LL - LL)/LL;
  bool conv = false;
  if (abs_change < d.min_abs && frac_change < d.min_frac) conv = true;
  else {
    conv = true;
    for (int k = 0; k < 6; k++) if (!(fabs(d.sp[6*l + k] - nw[k]) < 0.0001)) conv = false;     // parameters_within_threshold (stutter_model.h:62-65)
  }
  for (int k = 0; k < 6; k++) d.sp[6*l + k] = nw[k];
  if (conv){ d.state[l] = 1; return; }
  d.cur_ll[l] = new_LL; d.iter[l] = it + 1;
  if (it + 1 > d.max_iter){ d.state[l] = 2; return; }                           // ran out of iterations: train() returns false
  em_logs(nw, d.logp_rw + 9*(size_t)l);
}

// The loci still training, ascending, and where their (locus, sample) units go: one workgroup, an exclusive scan over the loci in chunks.
__global__ void __launch_bounds__(HS_EM_COMPACT_THREADS) hs_em_compact(const hs_em_dev_t* __restrict__ dp){
  const hs_em_dev_t& d = *dp;
  const int tid = threadIdx.x;
  __shared__ int sc_n[HS_EM_COMPACT_THREADS], sc_u[HS_EM_COMPACT_THREADS];
  __shared__ int base_n, base_u;
  if (tid == 0){ base_n = 0; base_u = 0; }
  __syncthreads();
  for (int l0 = 0; l0 < d.n_loci; l0 += HS_EM_COMPACT_THREADS){
    const int l = l0 + tid;
    const int on = (l < d.n_loci && d.state[l] == 0) ? 1 : 0;
    const int nu = on ? d.loci[l].S : 0;
    sc_n[tid] = on; sc_u[tid] = nu;
    __syncthreads();
    for (int off = 1; off < HS_EM_COMPACT_THREADS; off <<= 1){               // inclusive scan (Hillis-Steele)
      const int a = (tid >= off) ? sc_n[tid - off] : 0, b = (tid >= off) ? sc_u[tid - off] : 0;
      __syncthreads();
      sc_n[tid] += a; sc_u[tid] += b;
      __syncthreads();
    }
    if (on){
      d.next_list[base_n + sc_n[tid] - 1] = l;
      d.next_unit_begin[l] = base_u + sc_u[tid] - nu;
    }
    __syncthreads();
    if (tid == HS_EM_COMPACT_THREADS - 1){ base_n += sc_n[HS_EM_COMPACT_THREADS - 1]; base_u += sc_u[HS_EM_COMPACT_THREADS - 1]; }
    __syncthreads();
  }
  if (tid == 0){ d.next_counts[0] = base_n; d.next_counts[1] = base_u; }
}
__global__ void __launch_bounds__(HS_EM_UNITS_THREADS) hs_em_units(const hs_em_dev_t* __restrict__ dp){
  const hs_em_dev_t& d = *dp;
  if ((int)blockIdx.x >= d.next_counts[0]) return;
  const int l = d.next_list[blockIdx.x];
  const int S = d.loci[l].S, b = d.next_unit_begin[l], u0 = d.unit_first[l];
  for (int s = threadIdx.x; s < S; s += HS_EM_UNITS_THREADS) d.next_units[b + s] = u0 + s;
}

// ---- host side -------------------------------------------------------------------------------------------------

double h_lse2(double a, double b){ return a > b ? a + log(1 + exp(b - a)) : b + log(1 + exp(a - b)); }       // mathops.cpp:52-57

// |effective difference| of an observed size against an allele size, as hs_em_fill forms it (the index into the table of integer
// logarithms), in 64 bits: the size difference itself may not fit an int
inline int64_t em_abs_eff(int64_t ob, int64_t allele, int period){
  const int64_t bd = ob - allele;
  const int64_t eff = (bd % period != 0) ? bd - bd/period : bd/period;
  return eff < 0 ? -eff : eff;
}

// What hipstr_em_train knows about a batch before the first device call (em_stutter_genotyper.h:55-100, .cpp:10-20): per locus the allele
// sizes, the reads' allele indices, the initial allele frequencies and its offsets into the device arrays; the (locus, sample) units of the
// posterior kernel.  Every refusal of an input is decided here — hipstr_debug_em_plan runs the same function.
struct EmPrep {
  std::vector<hs_em_locus_t> loci;
  std::vector<hs_post_unit_t> units;
  std::vector<int32_t> bps, obs, unit_locus;
  std::vector<double> gtp;
  int64_t post_off = 0, ll_off = 0, prior_off = 0, sa_off = 0; int samp_off = 0;
};
// One locus' record and its (locus, sample) posterior units, behind those of the loci before it (P's running offsets): the layout of every
// device array of the loop.  bps_off: where the locus' A allele sizes and log frequencies start in bps / gtp.
void em_push_locus(EmPrep& P, int l, int A, int S, int r0, int R, int period, int haploid, int32_t bps_off, const int32_t* reads_of_sample){
  hs_em_locus_t& L = P.loci[l];
  memset(&L, 0, sizeof L);
  L.A = A; L.S = S; L.R = R; L.period = period; L.haploid = haploid;
  L.read_begin = r0; L.samp_begin = P.samp_off; L.bps_off = bps_off;
  L.post_off = P.post_off; L.ll_off = P.ll_off; L.prior_off = P.prior_off; L.sa_off = P.sa_off;
  int r = r0;
  for (int s = 0; s < S; s++){                                       // posterior-kernel units: (locus, sample)
    hs_post_unit_t u; memset(&u, 0, sizeof u);
    u.post_off = P.post_off + (int64_t)s*A*A; u.prior_off = P.prior_off; u.n_alleles = A; u.samp_index = P.samp_off + s;
    u.read_begin = r; u.ll_off = P.ll_off + (int64_t)(r - r0)*A;
    r += reads_of_sample[s];
    u.n_reads = r - u.read_begin;
    P.units.push_back(u); P.unit_locus.push_back(l);
  }
  P.post_off += (int64_t)S*A*A; P.ll_off += (int64_t)R*A; P.prior_off += (int64_t)A*A; P.samp_off += S; P.sa_off += (int64_t)S*A;
}
int em_prepare(const hipstr_em_batch_t* eb, bool host_loop, EmPrep& P){
  using hipstr::api_fail;
  const int nl = eb->n_loci;
  const int n_reads = eb->read_off[nl];
  const int64_t n_logs = (int64_t)hipstr::host_tables().int_log.size();      // entries of the table of integer logarithms (mathops.cpp:13-21)
  std::vector<hs_em_locus_t>& loci = P.loci; std::vector<hs_post_unit_t>& units = P.units;
  std::vector<int32_t>& bps = P.bps; std::vector<int32_t>& obs = P.obs; std::vector<int32_t>& unit_locus = P.unit_locus;
  std::vector<double>& gtp = P.gtp;
  loci.assign(nl, hs_em_locus_t()); obs.assign(n_reads, 0);
  // per locus, independent of the others (host threads): allele sizes, the reads' allele indices, the initial allele frequencies
  struct LocusPrep { std::vector<int> sizes; std::vector<double> gtp; std::vector<int32_t> reads_of_sample; const char* err = NULL; };
  std::vector<LocusPrep> lp(nl);
  hipstr::parallel_for(nl, nl >= 64 ? hipstr::host_threads() : 1, [&](int l){
    LocusPrep& Q = lp[l];
    const int S = eb->n_samples[l], r0 = eb->read_off[l], r1 = eb->read_off[l+1];
    if (eb->period[l] < 1 || eb->period[l] > 9){ Q.err = "STR period must be in [1,9] (stutter_model.h:38)"; return; }
    if (S < 1){ Q.err = "locus without samples"; return; }
    std::vector<int>& sizes = Q.sizes;
    for (int r = r0; r < r1; r++) if (eb->num_bps[r] != eb->ref_allele) sizes.push_back(eb->num_bps[r]);
    std::sort(sizes.begin(), sizes.end());
    sizes.erase(std::unique(sizes.begin(), sizes.end()), sizes.end());
    sizes.insert(sizes.begin(), eb->ref_allele);
    const int A = (int)sizes.size();
    if (A + 1 >= n_logs){ Q.err = "too many distinct allele sizes"; return; }
    // Every (observed size, allele) pair looks its effective difference up in the table of integer logarithms (hs_em_fill; the reference
    // does the same, em_stutter_genotyper.cpp:76-104 with mathops.cpp:13-21): beyond the table there is no answer.  |eff| <= |difference|,
    // so a span of the sizes (the reference allele included, observed or not) below the table's length settles it with one subtraction.
    {
      int64_t lo = sizes[0], hi = sizes[0];
      if (A > 1){ lo = std::min<int64_t>(lo, sizes[1]); hi = std::max<int64_t>(hi, sizes[A-1]); }
      if (hi - lo >= n_logs){
        for (int i = 0; i < A && !Q.err; i++) for (int j = i + 1; j < A; j++)       // (|eff| is the same either way round)
          if (em_abs_eff(sizes[j], sizes[i], eb->period[l]) >= n_logs){ Q.err = "allele sizes too far apart (effective difference beyond the table of integer logarithms, mathops.cpp:13-21)"; break; }
        if (Q.err) return;
      }
    }
    Q.reads_of_sample.assign(S, 0);
    int prev = 0;
    for (int r = r0; r < r1; r++){
      const int s = eb->sample_label[r];
      if (s < prev || s >= S){ Q.err = "reads of a locus must be grouped by ascending sample label (genotyper.h:112-119)"; return; }
      prev = s; Q.reads_of_sample[s]++;
      obs[r] = (int32_t)(std::lower_bound(sizes.begin() + 1, sizes.end(), eb->num_bps[r]) - sizes.begin());
      if (eb->num_bps[r] == eb->ref_allele) obs[r] = 0;
    }
    std::vector<double> g(A, 1.0);                                     // init_log_gt_priors (:10-20)
    for (int r = r0; r < r1; r++) g[obs[r]] += 1.0/Q.reads_of_sample[eb->sample_label[r]];
    double tot = 0.0; for (int a = 0; a < A; a++) tot += g[a];
    // (cr_math.h's correctly rounded log on the host as well: every exp / log of the EM is the same function on either side — the host libm's
    //  bits wherever that is correctly rounded; HIPSTR_EM_HOST_LOOP=1 takes the libm itself, as in round 4)
    const double lt = host_loop ? log(tot) : cr_log(tot);
    Q.gtp.resize(A);
    for (int a = 0; a < A; a++) Q.gtp[a] = (host_loop ? log(g[a]) : cr_log(g[a])) - lt;
  });
  for (int l = 0; l < nl; l++){
    const LocusPrep& Q = lp[l];
    if (Q.err) return api_fail(Q.err);
    const int r0 = eb->read_off[l], r1 = eb->read_off[l+1];
    em_push_locus(P, l, (int)Q.sizes.size(), eb->n_samples[l], r0, r1 - r0, eb->period[l], (eb->haploid && eb->haploid[l]) ? 1 : 0, (int32_t)bps.size(), Q.reads_of_sample.data());
    gtp.insert(gtp.end(), Q.gtp.begin(), Q.gtp.end());
    bps.insert(bps.end(), Q.sizes.begin(), Q.sizes.end());
  }
  return 0;
}

// ---- The loop of train() (:171-226) for a prepared batch: P's locus records and posterior units, and the seven per-read and per-allele
// arrays they index — uploaded with the rest from em_prepare's host arrays (hipstr_em_train) or built on the device (em_input.hip:
// hipstr_em_train_dev).  em_loop below is the sequence of its stages.

// The call's memory is ONE layout: every array of the loop is a piece of the device block of a hipstr::ResultBlocks (what comes home first,
// then the workspace) or of the uploaded block of a hipstr::HostArena, sized from P's totals.  lay() names every array once, as a piece and
// as the address the kernels get; it runs twice: without blocks the addresses are offsets and only the sizes count (em_blocks, and
// hipstr_debug_em_plan's "blocks"), with them it fills the argument structs (em_arguments).  Each
// run starts both piece lists afresh and must take the same branches: em_loop checks that the second arrives at the first's sizes.  Most pieces serve both loops; a piece that only
// one loop's kernels touch is that loop's: the device loop's lists, counts, state and parameters; the host loop's masks (em_locus' `active`,
// the posterior kernel's `unit_active`) and hs_em_mstep's new_ll / sums; the nine logs per locus are uploaded in the one and workspace in
// the other.  tests/test_em_routes.py restates the list.
constexpr int EM_NBUF = 4;          // rounds whose counts may be on their way home
struct EmHostArrays { const int32_t *sample_label, *weight; const double *log_p1, *log_p2; size_t n_reads; };      // hipstr_em_train's own, beside P's bps / obs / gtp
struct EmBlocks {
  hipstr::ResultBlocks B; hipstr::HostArena ar;
  bool device_loop = true, timing = false; int pieces = 0;
  hs_em_dev_t h[2]; hs_post_dev_t ph[2];          // the argument structs: one pair for the host loop, two for the device loop (the lists swap roles)
  const hs_em_dev_t* d_h = NULL; const hs_post_dev_t* d_ph = NULL;      // ... where they land
  double* keep = NULL; int32_t* polled = NULL;   // hs_em_mstep_keepmax's maxima; the counts of EM_NBUF rounds (a results' piece for its pinned side: the device side is idle)
  std::vector<int32_t> first_unit;
  size_t round_off = 0, round_bytes = 0;          // the host loop's per-round upload within the arena
  template <typename T> T* piece(size_t count){ pieces++; return (T*)((uintptr_t)B.d + B.take(count*sizeof(T))); }
  template <typename T> T* sent(const T* src, size_t count){ pieces++; return (T*)((uintptr_t)ar.dev + ar.add(src, count*sizeof(T))); }
  template <typename T> T* home(const T* p) const { return (T*)(B.h + ((const char*)p - B.d)); }             // a results' piece on the host, after fetch
  template <typename T> T* staged(const T* p) const { return (T*)(ar.pin + ((const char*)p - ar.dev)); }      // an uploaded piece in the pinned block

  void lay(const EmPrep& P, const EmHostArrays* up, const hipstr::EmDeviceArrays* on_device, const double* int_log, int max_iter, double min_abs_change, double min_frac_change){
    const hipstr::HostTables& HT = hipstr::host_tables();
    const size_t nl = P.loci.size(), nu = P.units.size(), ns = (size_t)P.samp_off, n_args = device_loop ? 2 : 1;
    B.tot = B.res = 0; ar.pieces.clear(); ar.total = 0; pieces = 0;
    hs_em_dev_t e; memset(&e, 0, sizeof e);
    hs_post_dev_t p; memset(&p, 0, sizeof p);
    // ---- what comes home: the device loop's four outputs and polled counts, or hs_em_mstep's for the host; a timed call's counters
    if (device_loop){ e.state = piece<int32_t>(nl); e.n_iter = piece<int32_t>(nl); e.final_ll = piece<double>(nl); e.sp = piece<double>(6*nl); polled = piece<int32_t>(2*EM_NBUF); }
    else { e.new_ll = piece<double>(nl); e.sums = piece<double>(7*nl); }
    if (timing) e.dbg = piece<unsigned long long>(4);
    B.end_results();
    // ---- workspace
    p.map_gt = piece<int32_t>(2*ns); e.ll = piece<double>(P.ll_off); e.prior = piece<double>(P.prior_off); p.log_post = piece<double>(P.post_off);
    p.sample_total = piece<double>(ns); e.row_lse = piece<double>(P.post_off); e.cat = piece<int32_t>(P.ll_off); e.leff = piece<double>(P.ll_off);
    e.part = piece<double>(7*(size_t)HS_EM_PARTS*nl); keep = piece<double>(7*nl); e.gmax = piece<double>(P.sa_off);
    // ---- uploaded: locus records and units; hipstr_em_train's seven arrays (hipstr_em_train_dev's are on the device); the argument structs
    e.loci = sent(P.loci.data(), nl); p.units = sent(P.units.data(), nu);
    const hipstr::EmDeviceArrays in = !up ? *on_device : hipstr::EmDeviceArrays{
      sent(P.bps.data(), P.bps.size()), sent(P.obs.data(), P.obs.size()), sent(up->sample_label, up->n_reads), sent(up->weight, up->n_reads),
      sent(up->log_p1, up->n_reads), sent(up->log_p2, up->n_reads), sent(P.gtp.data(), P.gtp.size()) };
    d_h = sent(h, n_args); d_ph = sent(ph, n_args);
    // ---- one loop's own
    int32_t *list[2] = {NULL, NULL}, *counts[2] = {NULL, NULL}, *ulist[2] = {NULL, NULL};
    if (device_loop){
      e.logp = e.logp_rw = piece<double>(9*nl);
      for (int k = 0; k < 2; k++) list[k] = piece<int32_t>(nl);
      for (int k = 0; k < 2; k++) counts[k] = piece<int32_t>(2);
      for (int k = 0; k < 2; k++) ulist[k] = piece<int32_t>(nu);
      e.next_unit_begin = piece<int32_t>(nl); e.iter = piece<int32_t>(nl); e.cur_ll = piece<double>(nl);
      first_unit.resize(nl);
      { int32_t u = 0; for (size_t l = 0; l < nl; l++){ first_unit[l] = u; u += P.loci[l].S; } }
      e.unit_first = sent(first_unit.data(), nl);
    } else {
      // The host writes these three into the pinned block and sends [round_off, round_off + round_bytes) again every round: they must stay
      // the arena's last pieces (em_loop checks it).  The first round writes them while send()'s copy of the whole block may still read
      // the pinned bytes: whatever that copy carries of them, the round's own copy follows it on the same stream, ahead of the kernels.
      round_off = ar.total;
      e.active = sent<int32_t>(NULL, nl); p.unit_active = sent<int32_t>(NULL, nu); e.logp = sent<double>(NULL, 9*nl);
      round_bytes = ar.total - round_off;
    }
    // ---- the structs
    e.bps = in.bps; e.obs = in.obs; e.sample_label = in.sample_label; e.log_p1 = in.log_p1; e.log_p2 = in.log_p2; e.gtp = in.gtp; e.int_log = int_log;
    e.post = p.log_post; e.sample_total = p.sample_total;
    e.log_thresh = HT.log_thresh; e.log_half = HT.log_half; e.log_1p1 = device_loop ? cr_log(1.1) : log(1.1);
    e.max_iter = max_iter; e.n_loci = (int32_t)nl; e.min_abs = min_abs_change; e.min_frac = min_frac_change;
    p.log_aln_probs = e.ll; p.log_p1 = in.log_p1; p.log_p2 = in.log_p2; p.read_weight = in.weight; p.log_prior = e.prior;
    p.log_thresh = HT.log_thresh; p.log_half = HT.log_half; p.sym_prior = 1;          // hs_em_fill: log f(a1) + log f(a2), or the haploid diagonal
    for (int k = 0; k < 2; k++){        // (the two sets of lists: a round reads one and writes the other; NULL with the host loop)
      h[k] = e; h[k].list = list[k]; h[k].counts = counts[k]; h[k].next_list = list[k ^ 1]; h[k].next_counts = counts[k ^ 1]; h[k].next_units = ulist[k ^ 1];
      ph[k] = p; ph[k].unit_list = ulist[k]; ph[k].n_list = device_loop ? counts[k] + 1 : NULL;
    }
  }
};

// The calling thread's auxiliary stream as the side stream of a round (the allele-frequency scans), and pooled events: fork, join, and
// the device loop's counts.  The call joins the side stream into its own before it waits for that; where it leaves between a fork and
// that wait, the side stream is waited for here — before the blocks go back (EmBlocks is declared first, so it dies last).
struct EmSide {
  hipstr::Ctx* ctx; hipStream_t stream = NULL; bool busy = false;
  hipEvent_t fork = NULL, join = NULL, counts[EM_NBUF] = {NULL, NULL, NULL, NULL};
  explicit EmSide(hipstr::Ctx* c) : ctx(c) {}
  ~EmSide(){
    if (busy) hipStreamSynchronize(stream);
    for (hipEvent_t e : {fork, join, counts[0], counts[1], counts[2], counts[3]}) hipstr::event_put(ctx, e);
  }
  int open(bool device_loop){            // 1 + the last error when the stream or an event is not to be had
    bool ok = (stream = hipstr::ctx_aux_stream(ctx)) && (fork = hipstr::event_get(ctx)) && (join = hipstr::event_get(ctx));
    for (int i = 0; ok && device_loop && i < EM_NBUF; i++) ok = (counts[i] = hipstr::event_get(ctx)) != NULL;
    return ok ? 0 : 1;
  }
};

// One round's launches.  The loops differ in the grids (a bound on the listed loci and units, or all of them), in who forms the next
// parameters (hs_em_finish, or hs_em_mstep's sums for the host) and in the device loop's lists of the next round.
int em_queue_round(hipStream_t st, EmSide& side, const hs_em_dev_t* H, const hs_post_dev_t* PH, double* keep, unsigned grid_loci, unsigned grid_units, bool device_loop){
  hipLaunchKernelGGL(hs_em_fill, dim3(grid_loci), dim3(256), 0, st, H);
  hipLaunchKernelGGL(hs_posterior_kernel, dim3(grid_units), dim3(256), 0, st, PH);
  HS_HIP(hipEventRecord(side.fork, st));                             // posteriors are in place: the allele-frequency scans branch off
  HS_HIP(hipStreamWaitEvent(side.stream, side.fork, 0));             // (beside the M-step on the side stream: 0.51 against 0.57 s per 10 000 loci in series, profiles/r05_notes.md)
  side.busy = true;
  hipLaunchKernelGGL(hs_em_gt_priors, dim3(grid_loci), dim3(HS_EM_THREADS), hs_em_lds_doubles()*sizeof(double), side.stream, H);
  HS_HIP(hipEventRecord(side.join, side.stream));
  hipLaunchKernelGGL(hs_em_gmax, dim3(grid_loci), dim3(256), 0, st, H);
  hipLaunchKernelGGL(hs_em_mstep_part<0>, dim3(grid_loci, HS_EM_PARTS), dim3(256), 0, st, H, (const double*)NULL);
  hipLaunchKernelGGL(hs_em_mstep_keepmax, dim3(grid_loci), dim3(64), 0, st, H, keep);
  hipLaunchKernelGGL(hs_em_mstep_part<1>, dim3(grid_loci, HS_EM_PARTS), dim3(256), 0, st, H, (const double*)keep);
  if (device_loop) hipLaunchKernelGGL(hs_em_finish, dim3(grid_loci), dim3(64), 0, st, H, (const double*)keep);
  else hipLaunchKernelGGL(hs_em_mstep, dim3(grid_loci), dim3(256), 0, st, H, (const double*)keep);
  HS_HIP(hipStreamWaitEvent(st, side.join, 0));                      // the new allele frequencies: the next round's hs_em_fill reads them, or the host this round's results
  if (device_loop){
    hipLaunchKernelGGL(hs_em_compact, dim3(1), dim3(HS_EM_COMPACT_THREADS), 0, st, H);
    hipLaunchKernelGGL(hs_em_units, dim3(grid_loci), dim3(HS_EM_UNITS_THREADS), 0, st, H);
  }
  return 0;
}

// HIPSTR_TIMING's stopwatch: a lap is printed, or added to a sum
struct EmClock {
  const bool timing = getenv("HIPSTR_TIMING") != NULL;
  std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
  void lap(const char* what, double* into){
    const auto now = std::chrono::steady_clock::now();
    const double dt = std::chrono::duration<double>(now - t_prev).count();
    t_prev = now;
    if (into) *into += dt; else if (timing) fprintf(stderr, "hipstr_em_train: %s %.3f ms\n", what, 1e3*dt);
  }
};

// The device-resident loop: the host queues round r + 1 while the counts of round r - 1 travel.  Returns the rounds queued in *rounds.
int em_run_device(const hipstr::ApiTables& T, const EmPrep& P, EmBlocks& M, EmSide& side, int max_iter, int* rounds){
  const int nl = (int)P.loci.size();
  hipStream_t st = T.stream;
  int32_t* const polled = M.home(M.polled);
  // the starting state, and the lists of round 0 (written through block 1, whose "next" set is block 0's current one)
  hipLaunchKernelGGL(hs_em_init, dim3(hs_em_init_blocks(nl)), dim3(HS_EM_INIT_THREADS), 0, st, M.d_h + 1);
  hipLaunchKernelGGL(hs_em_compact, dim3(1), dim3(HS_EM_COMPACT_THREADS), 0, st, M.d_h + 1);
  hipLaunchKernelGGL(hs_em_units, dim3(nl), dim3(HS_EM_UNITS_THREADS), 0, st, M.d_h + 1);
  unsigned bound_l = (unsigned)nl, bound_u = (unsigned)P.units.size();
  for (int r = 0; r <= hs_em_last_round(max_iter); r++){
    if (bound_l > 0){
      if (em_queue_round(st, side, M.d_h + (r & 1), M.d_ph + (r & 1), M.keep, bound_l, std::max(1u, bound_u), true)) return 1;
      (*rounds)++;
    }
    HS_HIP(hipMemcpyAsync(polled + 2*(r % EM_NBUF), M.h[r & 1].next_counts, 2*sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HS_HIP(hipEventRecord(side.counts[r % EM_NBUF], st));
    HS_HIP(hipGetLastError());
    if (r >= 1){
      // what round r - 1 left: the loci (and units) of round r — a bound for the grids of round r + 1, and the stop signal — while
      // round r is already queued
      HS_HIP(hipstr::wait_event(side.counts[(r - 1) % EM_NBUF]));
      bound_l = (unsigned)polled[2*((r - 1) % EM_NBUF)]; bound_u = (unsigned)polled[2*((r - 1) % EM_NBUF) + 1];
      if (bound_l == 0) break;
    }
  }
  return 0;
}
// ... and its results: one copy home
int em_results(EmBlocks& M, int nl, uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll){
  if (M.B.fetch()) return 1;
  const hs_em_dev_t& h = M.h[0];
  const int32_t* state = M.home(h.state);
  for (int l = 0; l < nl; l++) trained[l] = state[l] == 1 ? 1 : 0;
  memcpy(n_iter, M.home(h.n_iter), nl*sizeof(int32_t)); memcpy(final_ll, M.home(h.final_ll), nl*sizeof(double));
  memcpy(stutter, M.home(h.sp), 6*(size_t)nl*sizeof(double));
  return 0;
}

// The round-4 loop (HIPSTR_EM_HOST_LOOP=1), the yardstick of the device loop: the EM loop of train() (:171-226) with all loci in lock
// step, converged loci masked out, the parameters formed on the host with its libm.  The masks and the nine logs go up from the arena's
// pinned block, new_ll and sums come home as the results, every round.
int em_run_host(const hipstr::ApiTables& T, const EmPrep& P, EmBlocks& M, EmSide& side, EmClock& clock, int max_iter, double min_abs_change, double min_frac_change,
                uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll){
  const hipstr::HostTables& HT = hipstr::host_tables();
  const int nl = (int)P.loci.size(); const size_t n_units = P.units.size();
  double t_gpu = 0.0, t_host = 0.0;
  struct State { double sp[6]; double LL; int it; bool done, ok; };
  std::vector<State> st(nl);
  for (int l = 0; l < nl; l++){
    const double init[6] = { 0.9, 0.1, 0.1, 0.8, 0.01, 0.01 };        // init_stutter_model (:59-62)
    memcpy(st[l].sp, init, sizeof init);
    st[l].LL = -DBL_MAX; st[l].it = 1; st[l].done = false; st[l].ok = false;
    n_iter[l] = 0; final_ll[l] = 0; trained[l] = 0;
  }
  int32_t* const active = M.staged(M.h[0].active); int32_t* const unit_active = M.staged(M.ph[0].unit_active);
  double* const logp = M.staged(M.h[0].logp);
  const double* const newll = M.home(M.h[0].new_ll); const double* const sums = M.home(M.h[0].sums);
  for (;;){
    int n_active = 0;
    for (int l = 0; l < nl; l++){
      State& s = st[l];
      if (!s.done && s.it > max_iter){ s.done = true; s.ok = false; }      // ran out of iterations: train() returns false
      active[l] = s.done ? 0 : 1; n_active += active[l];
      const double* sp = s.sp;                                                 // StutterModel constructor (stutter_model.h:44-58)
      double* q = &logp[9*(size_t)l];
      q[0] = log(1-sp[0]); q[1] = log(sp[0]); q[2] = log(sp[1]); q[3] = log(sp[2]);
      q[4] = log(1-sp[3]); q[5] = log(sp[3]); q[6] = log(sp[4]); q[7] = log(sp[5]);
      q[8] = log(1-sp[1]-sp[2]-sp[4]-sp[5]);
    }
    if (n_active == 0) break;
    for (size_t u = 0; u < n_units; u++) unit_active[u] = active[P.unit_locus[u]];
    clock.lap("", &t_host);
    HS_HIP(hipMemcpyAsync(M.ar.dev + M.round_off, M.ar.pin + M.round_off, M.round_bytes, hipMemcpyHostToDevice, T.stream));
    if (em_queue_round(T.stream, side, M.d_h, M.d_ph, M.keep, (unsigned)nl, (unsigned)n_units, false)) return 1;
    HS_HIP(hipGetLastError());
    if (M.B.fetch()) return 1;
    side.busy = false;
    clock.lap("", &t_gpu);
    for (int l = 0; l < nl; l++){
      State& s = st[l];
      if (!active[l]) continue;
      const double new_LL = newll[l];
      n_iter[l] = s.it; final_ll[l] = new_LL;
      if (new_LL < s.LL + 1e-10){ s.done = true; s.ok = true; continue; }      // :190-194 (TOLERANCE = 1e-10)
      const double* t = &sums[7*(size_t)l];                                    // in_up, in_down, in_eq, in_diffs, out_up, out_down, out_diffs
      const double out_total = fast_lse2(t[4], t[5], HT.log_thresh);
      const double in_pgeom  = std::min(0.999, exp(h_lse2(t[0], t[1]) - t[3]));
      const double out_pgeom = std::min(0.999, exp(out_total - t[6]));
      const double m3 = std::max(std::max(t[0], t[1]), t[2]);
      const double lse3 = m3 + log(exp(t[0]-m3) + exp(t[1]-m3) + exp(t[2]-m3));          // mathops.cpp:59-62
      const double log_total = h_lse2(lse3, out_total);
      const double nw[6] = { in_pgeom, exp(t[0] - log_total), exp(t[1] - log_total), out_pgeom, exp(t[4] - log_total), exp(t[5] - log_total) };
      const double abs_change = new_LL - s.LL, frac_change = -(new_LL - s.LL)/s.LL;
      bool conv = false;
      if (abs_change < min_abs_change && frac_change < min_frac_change) conv = true;
      else {
        conv = true;
        for (int k = 0; k < 6; k++) if (!(fabs(s.sp[k] - nw[k]) < 0.0001)) conv = false;      // parameters_within_threshold (stutter_model.h:62-65)
      }
      memcpy(s.sp, nw, sizeof nw);
      if (conv){ s.done = true; s.ok = true; continue; }
      s.LL = new_LL; s.it++;
    }
  }
  if (clock.timing) fprintf(stderr, "hipstr_em_train: iterations: copies + kernels %.3f ms, host updates %.3f ms\n", 1e3*t_gpu, 1e3*t_host);
  for (int l = 0; l < nl; l++){
    trained[l] = st[l].ok ? 1 : 0;
    memcpy(stutter + 6*(size_t)l, st[l].sp, 6*sizeof(double));
  }
  return 0;
}

// `up`: the host arrays that go up with the rest (hipstr_em_train), or NULL: the seven arrays are on the device already, `on_device`
int em_loop(const hipstr::ApiTables& T, const EmPrep& P, const EmHostArrays* up, const hipstr::EmDeviceArrays* on_device, int max_iter, double min_abs_change,
            double min_frac_change, bool host_loop, uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll){
  EmClock clock;
  const int nl = (int)P.loci.size();
  EmBlocks M;
  M.device_loop = !host_loop; M.timing = clock.timing;
  auto lay = [&]{ M.lay(P, up, on_device, T.int_log, max_iter, min_abs_change, min_frac_change); };
  lay();                                                                    // em_blocks: the sizes, then the blocks
  const size_t tot = M.B.tot, res = M.B.res, sent = M.ar.total;
  if (M.ar.reserve(T.ctx) || M.B.reserve(T.ctx, T.stream)) return 1;
  lay();                                                                    // em_arguments: the same pass on the blocks' addresses
  if (M.B.tot != tot || M.B.res != res || M.ar.total != sent || (host_loop && M.round_off + M.round_bytes != sent))
    return hipstr::api_fail("hipstr_em_train: the layout's two passes disagree, or a piece follows the host loop's per-round upload");
  if (M.ar.send(T.stream)) return 1;
  if (M.timing) HS_HIP(hipMemsetAsync(M.h[0].dbg, 0, 4*sizeof(unsigned long long), T.stream));
  clock.lap("device state", NULL);
  EmSide side(T.ctx);
  if (side.open(!host_loop)) return 1;
  if (host_loop) return em_run_host(T, P, M, side, clock, max_iter, min_abs_change, min_frac_change, trained, stutter, n_iter, final_ll);
  clock.lap("device-loop state", NULL);
  int rounds = 0; double t_gpu = 0.0;
  if (em_run_device(T, P, M, side, max_iter, &rounds) || em_results(M, nl, trained, stutter, n_iter, final_ll)) return 1;
  side.busy = false;
  clock.lap("device loop", &t_gpu);
  if (M.timing){
    const unsigned long long* c = M.home(M.h[0].dbg);
    fprintf(stderr, "hipstr_em_train: device-resident loop, %d rounds queued: %.3f ms; M-step rows walked: maxima pass %llu of %llu, sums pass %llu of %llu\n", rounds, 1e3*t_gpu, c[0], c[1], c[2], c[3]);
  }
  return 0;
}

// hipstr_em_train on the device of T: em_prepare on the host, its arrays uploaded with the loop's own, the loop.
int em_train_on(const hipstr::ApiTables& T, const hipstr_em_batch_t* eb, uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll){
  const size_t n_reads = (size_t)eb->read_off[eb->n_loci];
  const bool host_loop = getenv("HIPSTR_EM_HOST_LOOP") && atoi(getenv("HIPSTR_EM_HOST_LOOP")) != 0;       // the round-4 loop: host libm, every locus in every round
  const auto t0 = std::chrono::steady_clock::now();
  // ---- alleles, read -> allele index, initial allele frequencies, (locus, sample) units; the refusals
  EmPrep P;
  if (em_prepare(eb, host_loop, P)) return 1;
  if (getenv("HIPSTR_TIMING")) fprintf(stderr, "hipstr_em_train: %s %.3f ms\n", "alleles and units", 1e3*std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  const std::vector<int32_t> ones(n_reads, 1);
  const EmHostArrays up = { eb->sample_label, ones.data(), eb->log_p1, eb->log_p2, n_reads };
  return em_loop(T, P, &up, NULL, eb->max_iter, eb->min_ll_abs_change, eb->min_ll_frac_change, host_loop, trained, stutter, n_iter, final_ll);
}

}  // namespace

extern "C" int hipstr_em_train(const hipstr_em_batch_t* eb, uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll){
  hipstr::ApiTimer prof_t(hipstr::PB_EM_TRAIN);
  using hipstr::api_fail;
  if (!eb || !trained || !stutter || !n_iter || !final_ll) return api_fail("null argument");
  const int nl = eb->n_loci;
  if (nl < 0) return api_fail("negative locus count");
  if (nl == 0) return 0;
  hipstr::ApiTables T;
  if (hipstr::api_device_tables(&T)) return 1;
  return em_train_on(T, eb, trained, stutter, n_iter, final_ll);
}

// ---- what em_input.hip (hipstr_em_train_dev) calls: api_internal.h
int hipstr::em_train_batch_on(const ApiTables& T, const hipstr_em_batch_t* eb, uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll){
  return em_train_on(T, eb, trained, stutter, n_iter, final_ll);
}
int hipstr::em_prepare_host(const hipstr_em_batch_t* eb, std::vector<int32_t>& size_off, std::vector<int32_t>& sizes, std::vector<int32_t>& obs, std::vector<double>& log_freq){
  EmPrep P;
  if (eb->n_loci > 0 && em_prepare(eb, false, P)) return 1;
  size_off.assign(1, 0);
  for (const hs_em_locus_t& L : P.loci) size_off.push_back(L.bps_off + L.A);
  sizes = P.bps; obs = P.obs; log_freq = P.gtp;
  return 0;
}
int hipstr::em_train_prepared(const ApiTables& T, int n_loci, const EmLocusFacts* facts, const int32_t* reads_of_sample, const EmDeviceArrays& arr,
                              int max_iter, double min_abs_change, double min_frac_change, uint8_t* trained, double* stutter, int32_t* n_iter, double* final_ll){
  hipstr::ApiTimer prof_t(hipstr::PB_EM_TRAIN);
  EmPrep P;
  P.loci.assign((size_t)n_loci, hs_em_locus_t());
  int64_t so = 0;
  for (int l = 0; l < n_loci; l++){
    const EmLocusFacts& F = facts[l];
    em_push_locus(P, l, F.A, F.S, F.read_begin, F.R, F.period, F.haploid, F.bps_off, reads_of_sample + so);
    so += F.S;
  }
  return em_loop(T, P, NULL, &arr, max_iter, min_abs_change, min_frac_change, false, trained, stutter, n_iter, final_ll);
}

#ifndef HIPSTR_NO_DEBUG_ABI
// Diagnostics (host only): the launch decisions hipstr_em_train takes for a batch, from the same preparation (em_prepare: the refusals are
// the call's) and the same functions (em_layout.h; post_layout.h for the posterior kernel's path), as one JSON object.
static const char* const kEmRoutes[] = {
  "gmax_wave", "gmax_thread", "rows_tile_full", "rows_tile_reduced", "rows_direct", "sweeps_1", "sweeps_2", "sweeps_3plus",
  "scan_last_chunk_full", "scan_last_chunk_partial", "slices_all_filled", "slices_some_empty", "slices_no_rows", "slice_one_tile",
  "slice_many_tiles", "post_registers", "post_chunked", "post_no_reads", "post_one_tile", "post_many_tiles", "init_one_block",
  "init_many_blocks", "compact_one_chunk", "compact_many_chunks", "units_one_pass", "units_strided" };
enum { EM_N_ROUTES = sizeof kEmRoutes / sizeof kEmRoutes[0] };
extern "C" int hipstr_debug_em_plan(const hipstr_em_batch_t* eb, char* json, int cap){
  using hipstr::api_fail;
  if (!eb) return api_fail("null argument"), -1;
  const int nl = eb->n_loci;
  if (nl < 0) return api_fail("negative locus count"), -1;
  EmPrep P;
  if (nl > 0 && em_prepare(eb, false, P)) return -1;
  std::string o; char b[512];
  auto put = [&](const char* fmt, auto... a){ snprintf(b, sizeof b, fmt, a...); o += b; };
  put("{\"thresholds\": {\"HS_EM_THREADS\": %d, \"HS_EM_PARTS\": %d, \"HS_EM_TILE\": %d, \"HS_EM_CHUNK\": %d, \"HS_EM_MAXA_LDS\": %d, \"HS_EM_GMAX_WAVE_MAXA\": %d, "
      "\"HS_EM_GMAX_WAVES\": %d, \"HS_EM_INIT_THREADS\": %d, \"HS_EM_COMPACT_THREADS\": %d, \"HS_EM_UNITS_THREADS\": %d, \"HS_EM_PRUNE_C\": %.17g, "
      "\"HS_EM_TERM_FLOOR\": %.17g, \"lds_doubles\": %d, \"int_log_len\": %d, \"last_round\": %d, \"HS_POST_THREADS\": %d, \"HS_POST_REGS\": %d, \"HS_POST_ECHUNK\": %d}, \"routes\": [",
      HS_EM_THREADS, HS_EM_PARTS, HS_EM_TILE, HS_EM_CHUNK, HS_EM_MAXA_LDS, HS_EM_GMAX_WAVE_MAXA, HS_EM_GMAX_WAVES, HS_EM_INIT_THREADS, HS_EM_COMPACT_THREADS,
      HS_EM_UNITS_THREADS, (double)HS_EM_PRUNE_C, (double)HS_EM_TERM_FLOOR, hs_em_lds_doubles(), (int)hipstr::host_tables().int_log.size(),
      hs_em_last_round(eb->max_iter), HS_POST_THREADS, HS_POST_REGS, HS_POST_ECHUNK);
  for (const char* r : kEmRoutes) put("\"%s\", ", r);
  o.resize(o.size() - 2);
  o += "], \"loci\": [";
  bool hit[EM_N_ROUTES] = {false};
  int max_S = 0;
  size_t u0 = 0;
  for (int l = 0; l < nl; l++){
    const hs_em_locus_t& L = P.loci[l];
    const int A = L.A, S = L.S, R = L.R;
    max_S = std::max(max_S, S);
    const bool wave = hs_em_gmax_wave(A);
    hit[wave ? 0 : 1] = true;
    // rows (sample, allele_1) of the posteriors per LDS tile
    const int tr = hs_em_row_tile_rows(A);
    const int64_t rows = (int64_t)S*A;
    const int64_t row_tiles = tr >= 1 ? (rows + tr - 1)/tr : 0;
    const int last_tile = tr >= 1 ? (int)(rows - (row_tiles - 1)*tr) : 0;
    hit[tr < 1 ? 4 : tr == HS_EM_THREADS ? 2 : 3] = true;
    // sweeps of HS_EM_MAXA_LDS chains; chunks of a chain
    const int sweeps = hs_em_sweeps(A);
    int last_sweep = 0; for (int a0 = 0; a0 < A; a0 += HS_EM_MAXA_LDS) last_sweep = hs_em_sweep_alleles(A, a0);
    hit[sweeps == 1 ? 5 : sweeps == 2 ? 6 : 7] = true;
    const int64_t ntot = hs_em_chain_len(S, A);
    int64_t chunks = 0; int last_chunk = 0;
    for (int64_t c0 = 0; c0 < ntot; c0 += HS_EM_CHUNK){ chunks++; last_chunk = hs_em_chunk_len(ntot, c0); }
    hit[last_chunk == HS_EM_CHUNK ? 8 : 9] = true;
    // slices of the R*A (read, source allele) rows
    const int total = R*A;
    int smin = INT32_MAX, smax = 0, empty = 0;
    for (int k = 0; k < HS_EM_PARTS; k++){
      const int n = hs_em_slice_begin(total, k + 1) - hs_em_slice_begin(total, k);
      smin = std::min(smin, n); smax = std::max(smax, n); if (n == 0) empty++;
    }
    const int tiles = (smax + HS_EM_TILE - 1)/HS_EM_TILE;
    hit[empty == 0 ? 10 : empty == HS_EM_PARTS ? 12 : 11] = true;
    if (tiles >= 1) hit[tiles == 1 ? 13 : 14] = true;
    // the posterior kernel on the locus' largest unit: one launch of hs_posterior_kernel (sym_prior), never split
    int ur = 0;
    for (int s = 0; s < S; s++) ur = std::max(ur, (int)P.units[u0 + s].n_reads);
    u0 += S;
    const bool regs = hs_post_in_registers(A*A);
    const int rt = regs ? hs_post_reads_per_tile(A, ur) : 0, ptiles = regs ? (ur + rt - 1)/rt : 0;
    hit[regs ? 15 : 16] = true;
    if (ur == 0) hit[17] = true; else if (regs) hit[ptiles == 1 ? 18 : 19] = true;
    put("%s{\"A\": %d, \"S\": %d, \"R\": %d, \"period\": %d, \"haploid\": %d, \"gmax\": \"%s\", \"row_tile\": ", l ? ", " : "", A, S, R, L.period, L.haploid, wave ? "wave" : "thread");
    if (tr >= 1) put("%d", tr); else o += "\"direct\"";
    put(", \"row_tiles\": %lld, \"last_row_tile\": %d, \"sweeps\": %d, \"last_sweep\": %d, \"scan_chunks\": %lld, \"scan_last\": %d, \"slice_rows\": [%d, %d], "
        "\"empty_slices\": %d, \"slice_tiles\": %d, \"post\": [\"%s\", %d, %d, %d]}", (long long)row_tiles, last_tile, sweeps, last_sweep, (long long)chunks, last_chunk,
        smin, smax, empty, tiles, regs ? "registers" : "chunked", ur, rt, ptiles);
  }
  const unsigned ib = nl > 0 ? hs_em_init_blocks(nl) : 0; const int cc = nl > 0 ? hs_em_compact_chunks(nl) : 0;
  const int passes = (max_S + HS_EM_UNITS_THREADS - 1)/HS_EM_UNITS_THREADS;
  if (nl > 0){ hit[ib == 1 ? 20 : 21] = true; hit[cc == 1 ? 22 : 23] = true; hit[passes <= 1 ? 24 : 25] = true; }
  put("], \"n_loci\": %d, \"init_blocks\": %u, \"compact_chunks\": %d, \"compact_last_chunk\": %d, \"max_S\": %d, \"units_passes\": %d, \"routes_hit\": [",
      nl, ib, cc, nl > 0 ? nl - (cc - 1)*HS_EM_COMPACT_THREADS : 0, max_S, passes);
  bool first = true;
  for (int i = 0; i < EM_N_ROUTES; i++) if (hit[i]){ put("%s\"%s\"", first ? "" : ", ", kEmRoutes[i]); first = false; }
  // the memory of the call: EmBlocks' layout for the device loop of hipstr_em_train (untimed) — the device block and how much of it comes
  // home, the uploaded block (pinned and device, each), and the arrays that are pieces of the two
  EmBlocks M;
  const EmHostArrays up = { NULL, NULL, NULL, NULL, nl > 0 ? (size_t)eb->read_off[nl] : 0 };
  M.lay(P, &up, NULL, NULL, eb->max_iter, eb->min_ll_abs_change, eb->min_ll_frac_change);
  put("], \"blocks\": {\"device_bytes\": %zu, \"result_bytes\": %zu, \"upload_bytes\": %zu, \"pieces\": %d}}", M.B.tot, M.B.res, M.ar.total, M.pieces);
  if (json && cap > 0){ const size_t m = std::min(o.size(), (size_t)cap - 1); memcpy(json, o.data(), m); json[m] = 0; }
  return (int)o.size();
}
#endif  // HIPSTR_NO_DEBUG_ABI
