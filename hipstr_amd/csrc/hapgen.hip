// hapgen.hip — HaplotypeGenerator on gfx950: the three haplotype blocks of a batch of single-region loci from their un-pooled reads
// (HaplotypeGenerator.cpp:12-366, seq_stutter_genotyper.cpp:428-432), in front of hipstr_pool_batch.  Integer work except one double
// division, one double sum in a fixed order and three double comparisons per string, so device and host twin (hapgen_host.cpp) agree bit
// for bit.
//
//   hs_hapgen_extract_kernel  a lane per read: the span test and the CIGAR walk of extract_sequence give the run of the read's bases that
//                             is its allele (offset, length; -1 = not counted); the locus' four bounds (start / stop of all reads, of the
//                             flagged reads) are reduced across the wavefront where it holds reads of one locus, then one atomic each
//   hs_hapgen_hash_kernel     a wavefront per counted read: a 64-bit hash of the folded bytes of the run (any start byte; length 0 is a key)
//   hs_hapgen_group_kernel    a workgroup per locus: the status from the bounds; the hashes go into an open-addressing table in LDS, the
//                             lowest read index leads a slot; every member is compared with its leader byte for byte, folded (a difference
//                             raises the locus' redo flag); then per-sample counts, a counting sort of the counted reads by sample, a thread
//                             per distinct string for its per-sample counts in ascending sample order (strong samples, the double sum), the
//                             (length, bytes) rank of every distinct string, the selection, the options in order, the common prefix /
//                             suffix, trim, and the blocks' coordinates
//   hs_hapgen_scan_kernel     one workgroup: the loci's option counts and sequence bytes into offsets
//   hs_hapgen_copy_kernel     a workgroup per locus: the offsets of its options, then a wavefront per option copies the folded bytes
// One workgroup does everything a locus needs after the grouping, so the per-locus steps the issue lists as "the same kernel or a
// following one" are phases of hs_hapgen_group_kernel between barriers: none of them has work for more than a few hundred threads.
// No kernel waits on memory and no workgroup talks to another; every loop has a bound taken from the uploaded tables.  Correctness never
// rests on the hash: a locus with its redo flag up, and a locus beyond a cap of hapgen_layout.h, is done by the host twin in the same call.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "api_internal.h"
#include "hapgen_host.h"
#include "hapgen_layout.h"

namespace {

#define HG_NT HS_HAPGEN_THREADS

// ------------------------------------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ int hg_wave_incl_scan(int v, int lane){
  for (int dlt = 1; dlt < 64; dlt <<= 1){ const int o = __shfl_up(v, dlt); if (lane >= dlt) v += o; }
  return v;
}
// exclusive prefix of the workgroup's values in thread order; total = their sum.  part: four dwords of LDS.  Every thread calls it.
__device__ __forceinline__ int hg_wg_excl_scan(int v, int32_t* part, int& total){
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = hg_wave_incl_scan(v, lane);
  __syncthreads();
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < HG_NT/64; w++){ const int pw = part[w]; tot += pw; if (w < wave) base += pw; }
  total = tot;
  return base + incl - v;
}

extern "C" __global__ void __launch_bounds__(HG_NT) hs_hapgen_extract_kernel(const hs_hapgen_dev_t d){
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x*HG_NT + threadIdx.x;
  const bool active = r < d.n;
  const unsigned long long act = __ballot(active);
  if (act == 0) return;                                               // (the whole wavefront)
  const int lc = active ? d.rlocus[r] : 0;
  const int start = active ? d.start[r] : 0, stop = active ? d.stop[r] : 0;
  const bool use = active && d.use[r] != 0;
  // ---- the four bounds: across the wavefront first where all its reads are of one locus
  {
    int mn_a = active ? start : INT_MAX, mx_a = active ? stop : INT_MIN, mn_f = use ? start : INT_MAX, mx_f = use ? stop : INT_MIN;
    const int first = __ffsll((long long)act) - 1;
    const int lc0 = __shfl(lc, first);
    if (__ballot(active && lc != lc0) == 0){
      for (int m = 32; m >= 1; m >>= 1){
        mn_a = min(mn_a, __shfl_xor(mn_a, m)); mx_a = max(mx_a, __shfl_xor(mx_a, m));
        mn_f = min(mn_f, __shfl_xor(mn_f, m)); mx_f = max(mx_f, __shfl_xor(mx_f, m));
      }
      if (lane == first){
        atomicMin(&d.bounds[4*lc0], mn_a); atomicMax(&d.bounds[4*lc0+1], mx_a); atomicMin(&d.bounds[4*lc0+2], mn_f); atomicMax(&d.bounds[4*lc0+3], mx_f);
      }
    } else if (active){
      atomicMin(&d.bounds[4*lc], mn_a); atomicMax(&d.bounds[4*lc+1], mx_a); atomicMin(&d.bounds[4*lc+2], mn_f); atomicMax(&d.bounds[4*lc+3], mx_f);
    }
  }
  if (!active) return;
  int off = -1, len = -1;
  if (use && !d.chrom_fail[lc]){
    const int rs = d.rs0[lc] - HS_HAPGEN_LEFT_PAD, re = d.rp0[lc] + HS_HAPGEN_RIGHT_PAD;
    if (start < rs && stop > re){                                     // :83-84
      // the walk of :86-152 over read bases; every turn of the loop moves to the next run or forward within one: at most 2 turns per
      // run and 3 more per run for the region's two edges
      const int c0 = d.coff[r], nc = d.coff[r+1] - c0;
      int ci = 0, ch = 0, pos = start, ri = 0, kept = 0;
      for (int turn = 0; turn < 5*nc + 5 && ci < nc; turn++){
        const int num = d.clen[c0 + ci]; const char op = d.cop[c0 + ci];
        if (ch == num){ ci++; ch = 0; }
        else if (pos > re) break;
        else if (pos == re){
          if (op != 'I') break;
          kept += num; ri += num; ch = 0; ci++;
        }
        else if (pos >= rs){
          int nb = min(re - pos, num - ch);
          if (op == 'I'){ nb = num; kept += nb; ri += nb; }
          else if (op == 'D') pos += nb;
          else { kept += nb; ri += nb; pos += nb; }
          ch += nb;
        }
        else {
          int nb;
          if (op == 'I'){ nb = num - ch; ri += nb; }
          else { nb = min(rs - pos, num - ch); pos += nb; if (op != 'D') ri += nb; }
          ch += nb;
        }
      }
      off = ri - kept; len = kept;
    }
  }
  d.ext_off[r] = off; d.ext_len[r] = len;
}

extern "C" __global__ void __launch_bounds__(HG_NT) hs_hapgen_hash_kernel(const hs_hapgen_dev_t d){
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x*(HG_NT/64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (r >= d.n) return;
  const int len = d.ext_len[r];
  if (len < 0) return;
  const char* p = d.bases + d.boff[r] + d.ext_off[r];                 // any alignment: bytes
  unsigned long long sum = 0;
  for (int piece = lane; piece*HS_HAPGEN_HASH_STEP < len; piece += 64){
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 8; k++){
      const int i = piece*HS_HAPGEN_HASH_STEP + k, j = i + 8;
      if (i < len) lo |= (uint64_t)(uint8_t)hs_hapgen_fold(p[i]) << (8*k);
      if (j < len) hi |= (uint64_t)(uint8_t)hs_hapgen_fold(p[j]) << (8*k);
    }
    sum += hs_pool_hash_piece(lo, hi, (uint64_t)piece);
  }
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
  if (lane == 0) d.hash[r] = hs_pool_hash_finish(sum, len, d.hash_bits);
}

extern __shared__ uint64_t hs_hapgen_lds[];

// (length, folded bytes) order of two runs of bases
__device__ __forceinline__ int hg_cmp(const char* a, int la, const char* b, int lb){
  if (la != lb) return la < lb ? -1 : 1;
  for (int i = 0; i < la; i++){
    const unsigned x = (uint8_t)hs_hapgen_fold(a[i]), y = (uint8_t)hs_hapgen_fold(b[i]);
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

extern "C" __global__ void __launch_bounds__(HG_NT) hs_hapgen_group_kernel(const hs_hapgen_dev_t d){
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lc = blockIdx.x;
  const int r0 = d.lread_off[lc], n = d.lread_off[lc+1] - r0;
  int32_t* res = d.lres + HS_HAPGEN_LRES*lc;
  const int rs0 = d.rs0[lc], rp0 = d.rp0[lc];
  const int mn_a = d.bounds[4*lc], mx_a = d.bounds[4*lc+1], mn_f = d.bounds[4*lc+2], mx_f = d.bounds[4*lc+3];
  const int status = d.chrom_fail[lc] ? 1 : hs_hapgen_status(rs0, rp0, (int64_t)1 << 40, mn_f, mx_f);
  if (status != 0 || n <= 0){                                        // (a locus the host does has no reads here and is not looked at)
    for (int r = t; r < n; r += HG_NT){ d.ext_off[r0 + r] = -1; d.ext_len[r0 + r] = -1; }
    if (t < HS_HAPGEN_LRES) res[t] = t == HS_HG_STATUS ? (n <= 0 && status == 0 ? 2 : status) : t == HS_HG_MIN ? mn_a : t == HS_HG_MAX ? mx_a : 0;
    return;
  }
  const int S = d.nsamp[lc];
  const int slots = hs_hapgen_table_slots(n);
  const int DC = HS_HAPGEN_MAX_DISTINCT;
  uint64_t* keys = hs_hapgen_lds;                  // [slots]
  double* d_frac = (double*)(keys + slots);        // [DC]
  int32_t* lead = (int32_t*)(d_frac + DC);         // [slots] lowest read index of the slot's key
  int32_t* did = lead + slots;                     // [n] slot of the read, then its distinct string; -1 = not counted
  int32_t* byS = did + n;                          // [n] number of a leader's string until phase 5; then the counted reads in sample order
  int32_t* hist = byS + n;                         // [S] counted reads of a sample
  int32_t* scur = hist + S;                        // [S] where the sample's reads go in byS
  int32_t* d_rep = scur + S;                       // [DC] first read of the string
  int32_t* d_len = d_rep + DC, *d_src = d_len + DC, *d_reads = d_src + DC, *d_strong = d_reads + DC, *d_byrank = d_strong + DC, *d_sel = d_byrank + DC;
  int32_t* d_opt = d_sel + DC;                     // [DC+8] string of option o (o >= 1)
  int32_t* sc = d_opt + DC + 8;                    // [64] scalars: 0..3 scan partials
  enum { SC_REDO = 8, SC_READS = 9, SC_MINLEN = 10, SC_PRE = 11, SC_SUF = 12, SC_SEQ = 13, SC_SAMP = 14 };

  // ---- 1: an empty table
  for (int i = t; i < slots; i += HG_NT){ keys[i] = HS_POOL_EMPTY_KEY; lead[i] = INT32_MAX; }
  for (int i = t; i < S; i += HG_NT) hist[i] = 0;
  for (int i = t; i < DC; i += HG_NT){ d_reads[i] = 0; d_rep[i] = 0; d_len[i] = 0; d_src[i] = 0; }
  if (t < 64) sc[t] = t == SC_MINLEN ? INT32_MAX : (t == SC_PRE || t == SC_SUF) ? 0x1F : 0;
  __syncthreads();
  // ---- 2: every counted read finds or claims the slot of its hash (at most half the slots are ever taken: the probe ends)
  for (int r = t; r < n; r += HG_NT){
    int s = -1;
    if (d.ext_len[r0 + r] >= 0){
      const uint64_t h = d.hash[r0 + r];
      s = (int)(h & (uint64_t)(slots - 1));
      for (int probe = 0; probe < slots; probe++){
        const unsigned long long prev = atomicCAS((unsigned long long*)&keys[s], (unsigned long long)HS_POOL_EMPTY_KEY, (unsigned long long)h);
        if (prev == HS_POOL_EMPTY_KEY || prev == h) break;
        s = (s + 1) & (slots - 1);
      }
      atomicMin(&lead[s], r);
      atomicAdd(&hist[d.sample[r0 + r]], 1);
      atomicAdd(&sc[SC_READS], 1);
    }
    did[r] = s;
  }
  __syncthreads();
  // ---- 3: the strings are numbered as their first reads appear: a scan over the leader flags in read order
  int D = 0;
  for (int base = 0; base < n; base += HG_NT){
    const int r = base + t;
    const int flag = (r < n && did[r] >= 0 && lead[did[r]] == r) ? 1 : 0;
    int tot;
    const int ex = hg_wg_excl_scan(flag, sc, tot);
    if (flag){
      byS[r] = D + ex;
      if (D + ex < DC){ d_rep[D + ex] = r; d_len[D + ex] = d.ext_len[r0 + r]; d_src[D + ex] = d.boff[r0 + r] + d.ext_off[r0 + r]; }
    }
    D += tot;
  }
  __syncthreads();
  if (D > DC){                                                        // (D is the same in every thread)
    if (t < HS_HAPGEN_LRES) res[t] = t == HS_HG_REDO ? 2 : t == HS_HG_MIN ? mn_a : t == HS_HG_MAX ? mx_a : 0;
    return;
  }
  // ---- 4: a wavefront per read: the member against its leader, byte for byte, folded
  for (int r = wave; r < n; r += HG_NT/64){
    const int s = did[r];
    if (s < 0) continue;
    const int L = lead[s];
    if (L == r) continue;
    const int len = d.ext_len[r0 + r];
    bool diff = len != d.ext_len[r0 + L];
    if (!diff){
      const char* a = d.bases + d.boff[r0 + r] + d.ext_off[r0 + r];
      const char* b = d.bases + d.boff[r0 + L] + d.ext_off[r0 + L];
      for (int i = lane; i < len; i += 64) diff = diff || hs_hapgen_fold(a[i]) != hs_hapgen_fold(b[i]);
    }
    if (__ballot(diff) != 0 && lane == 0) sc[SC_REDO] = 1;
  }
  __syncthreads();
  // ---- 5: the string of every read, reads per string
  int my[HS_HAPGEN_LDS_READS/HG_NT];
#pragma unroll
  for (int k = 0; k < HS_HAPGEN_LDS_READS/HG_NT; k++){
    const int r = k*HG_NT + t;
    my[k] = (r < n && did[r] >= 0) ? byS[lead[did[r]]] : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < HS_HAPGEN_LDS_READS/HG_NT; k++){
    const int r = k*HG_NT + t;
    if (r < n){ did[r] = my[k]; if (my[k] >= 0) atomicAdd(&d_reads[my[k]], 1); }
  }
  // ---- 6: the samples' reads: where each sample's run starts in byS, the samples that have any
  int s_sum = 0;
  for (int base = 0; base < S; base += HG_NT){
    const int s = base + t;
    const int c = s < S ? hist[s] : 0;
    int tot;
    const int ex = hg_wg_excl_scan(c, sc, tot);
    if (s < S){ scur[s] = s_sum + ex; if (c > 0) atomicAdd(&sc[SC_SAMP], 1); }
    s_sum += tot;
  }
  __syncthreads();
  for (int r = t; r < n; r += HG_NT)
    if (did[r] >= 0) byS[atomicAdd(&scur[d.sample[r0 + r]], 1)] = r;      // (the order inside a sample changes no count)
  __syncthreads();
  const int tot_reads = sc[SC_READS], tot_samples = sc[SC_SAMP];
  // ---- 7: a thread per string: its reads sample after sample, ascending — the order sample_counts is summed in (:180-184)
  for (int q = t; q < D; q += HG_NT){
    int strong = 0, cur = -1, c = 0; double frac = 0.0;
    for (int i = 0; i <= tot_reads; i++){
      const int r = i < tot_reads ? byS[i] : -1;
      const int s = i < tot_reads ? d.sample[r0 + r] : -2;
      if (s != cur){
        if (c > 0){
          const int sr = hist[cur];
          if ((double)c >= 2.0 && (double)c >= 0.2*sr) strong++;     // :181
          frac += c*1.0/sr;                                            // :183
        }
        cur = s; c = 0;
      }
      if (i < tot_reads && did[r] == q) c++;
    }
    d_strong[q] = strong; d_frac[q] = frac;
  }
  // ---- 8: the rank of every string in (length, bytes) order; which are selected; which is the reference
  const char* ref = d.window + d.woff[lc] + (HS_HAPGEN_WIN_PAD - HS_HAPGEN_LEFT_PAD);
  const int ref_len = rp0 - rs0 + HS_HAPGEN_LEFT_PAD + HS_HAPGEN_RIGHT_PAD;
  __syncthreads();
  for (int q = t; q < D; q += HG_NT){
    const char* a = d.bases + d_src[q]; const int la = d_len[q];
    int rank = 0;
    for (int e = 0; e < D; e++) rank += (e != q && hg_cmp(d.bases + d_src[e], d_len[e], a, la) < 0) ? 1 : 0;
    d_byrank[rank] = q;                                               // (distinct strings: the ranks are a permutation)
    const bool sel = d_strong[q] >= 1 || d_frac[q] > 0.05*tot_samples || (double)d_reads[q] > 0.05*tot_reads;      // :207-226
    d_sel[q] = (sel && hg_cmp(a, la, ref, ref_len) != 0) ? 1 : 0;
    const int g = r0 + rank;
    d.dist_len[g] = la; d.dist_rep[g] = r0 + d_rep[q]; d.dist_reads[g] = d_reads[q]; d.dist_strong[g] = d_strong[q]; d.dist_frac[g] = d_frac[q];
  }
  __syncthreads();
  // ---- 9: the options of block 1: the reference, then the selected strings in rank order
  int nopts = 1;
  for (int base = 0; base < D; base += HG_NT){
    const int k = base + t;
    const int q = k < D ? d_byrank[k] : 0;
    const int flag = k < D ? d_sel[q] : 0;
    int tot;
    const int ex = hg_wg_excl_scan(flag, sc, tot);
    if (flag){ d_opt[nopts + ex] = q; atomicMin(&sc[SC_MINLEN], d_len[q]); }
    nopts += tot;
  }
  __syncthreads();
  // ---- 10: trim: the shortest option, the common prefix and suffix as far as trim can use them (5 positions: a bit each)
  const int min_len = min(sc[SC_MINLEN], ref_len);
  const int ideal = 3*d.period[lc];
  const int lim = min_len > ideal ? min(HS_HAPGEN_LEFT_PAD, min_len - ideal) : 0;
  for (int o = 1 + t; o < nopts && lim > 0; o += HG_NT){
    const int q = d_opt[o];
    const char* a = d.bases + d_src[q]; const int la = d_len[q];
    int pre = 0, suf = 0;
    for (int i = 0; i < lim; i++){
      pre |= (hs_hapgen_fold(a[i]) == hs_hapgen_fold(ref[i]) ? 1 : 0) << i;
      suf |= (hs_hapgen_fold(a[la - 1 - i]) == hs_hapgen_fold(ref[ref_len - 1 - i]) ? 1 : 0) << i;
    }
    atomicAnd(&sc[SC_PRE], pre); atomicAnd(&sc[SC_SUF], suf);
  }
  __syncthreads();
  int lt = 0, rt = 0;
  {
    int cp = 0, cs = 0;
    while (cp < lim && ((sc[SC_PRE] >> cp) & 1)) cp++;
    while (cs < lim && ((sc[SC_SUF] >> cs) & 1)) cs++;
    hs_hapgen_trim(min_len, ideal, cp, cs, &lt, &rt);
  }
  // ---- 11: the blocks and where the options' bytes come from
  const int b1s = rs0 - HS_HAPGEN_LEFT_PAD + lt, b1e = rp0 + HS_HAPGEN_RIGHT_PAD - rt;
  const int b0s = min(b1s - 10, max(b1s - HS_HAPGEN_REF_FLANK, mn_a)), b2e = max(b1e + 10, min(b1e + HS_HAPGEN_REF_FLANK, mx_a));      // :349-350
  const int ob = r0 + lc;
  int bytes = 0;
  for (int o = t; o < nopts; o += HG_NT){
    int src, len;
    if (o == 0){ src = -1 - (d.woff[lc] + HS_HAPGEN_WIN_PAD - HS_HAPGEN_LEFT_PAD + lt); len = ref_len - lt - rt; }
    else { const int q = d_opt[o]; src = d_src[q] + lt; len = d_len[q] - lt - rt; }
    d.osrc[ob + o] = src; d.olen[ob + o] = len;
    bytes += len;
  }
  if (bytes) atomicAdd(&sc[SC_SEQ], bytes);
  __syncthreads();
  if (t == 0){
    res[HS_HG_STATUS] = 0; res[HS_HG_REDO] = sc[SC_REDO]; res[HS_HG_B0S] = b0s; res[HS_HG_B1S] = b1s; res[HS_HG_B1E] = b1e; res[HS_HG_B2E] = b2e;
    res[HS_HG_NOPTS] = nopts; res[HS_HG_SEQ] = sc[SC_SEQ] + (b1s - b0s) + (b2e - b1e); res[HS_HG_SPAN] = tot_reads; res[HS_HG_SAMP] = tot_samples;
    res[HS_HG_DIST] = D; res[HS_HG_LT] = lt; res[HS_HG_RT] = rt; res[HS_HG_MIN] = mn_a; res[HS_HG_MAX] = mx_a; res[15] = 0;
  }
}

// a locus whose blocks the device wrote
__device__ __forceinline__ bool hg_done(const int32_t* res){ return res[HS_HG_STATUS] == 0 && res[HS_HG_REDO] == 0; }

extern "C" __global__ void __launch_bounds__(HG_NT) hs_hapgen_scan_kernel(const hs_hapgen_dev_t d){
  __shared__ int32_t part[4];
  const int t = threadIdx.x;
  int o_sum = 0, q_sum = 0;
  for (int base = 0; base < d.nl; base += HG_NT){
    const int l = base + t;
    const int32_t* res = d.lres + HS_HAPGEN_LRES*(l < d.nl ? l : 0);
    const bool ok = l < d.nl && hg_done(res);
    const int no = ok ? res[HS_HG_NOPTS] + 2 : 0, qb = ok ? res[HS_HG_SEQ] : 0;
    int tot_o, tot_q;
    const int eo = hg_wg_excl_scan(no, part, tot_o);
    const int eq = hg_wg_excl_scan(qb, part, tot_q);
    if (l < d.nl){ d.l_opt[l] = o_sum + eo; d.l_seq[l] = q_sum + eq; }
    o_sum += tot_o; q_sum += tot_q;
  }
  if (t == 0){ d.l_opt[d.nl] = o_sum; d.l_seq[d.nl] = q_sum; d.opt_off[o_sum] = q_sum; }
}

extern "C" __global__ void __launch_bounds__(HG_NT) hs_hapgen_copy_kernel(const hs_hapgen_dev_t d){
  __shared__ int32_t part[4];
  __shared__ int32_t e_dst[HS_HAPGEN_MAX_DISTINCT + 8], e_src[HS_HAPGEN_MAX_DISTINCT + 8], e_len[HS_HAPGEN_MAX_DISTINCT + 8];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lc = blockIdx.x;
  const int32_t* res = d.lres + HS_HAPGEN_LRES*lc;
  if (!hg_done(res)) return;
  const int nopts = res[HS_HG_NOPTS], ne = nopts + 2;                 // entries: block 0, the options of block 1, block 2
  const int g0 = d.l_opt[lc], ob = d.lread_off[lc] + lc;
  const int w0 = d.woff[lc] - (d.rs0[lc] - HS_HAPGEN_WIN_PAD);        // window offset of a reference coordinate: w0 + coordinate
  int q = d.l_seq[lc];
  for (int base = 0; base < ne; base += HG_NT){
    const int e = base + t;
    int src = 0, len = 0;
    if (e == 0){ src = -1 - (w0 + res[HS_HG_B0S]); len = res[HS_HG_B1S] - res[HS_HG_B0S]; }
    else if (e == ne - 1){ src = -1 - (w0 + res[HS_HG_B1E]); len = res[HS_HG_B2E] - res[HS_HG_B1E]; }
    else if (e < ne){ src = d.osrc[ob + e - 1]; len = d.olen[ob + e - 1]; }
    int tot;
    const int ex = hg_wg_excl_scan(len, part, tot);
    if (e < ne){ e_dst[e] = q + ex; e_src[e] = src; e_len[e] = len; d.opt_off[g0 + e] = q + ex; }
    q += tot;
  }
  __syncthreads();
  for (int e = wave; e < ne; e += HG_NT/64){
    const int src = e_src[e], len = e_len[e];
    const char* p = src >= 0 ? d.bases + src : d.window + (-1 - src);
    char* dst = d.seq + e_dst[e];
    for (int i = lane; i < len; i += 64) dst[i] = hs_hapgen_fold(p[i]);
  }
}
static_assert(HS_HAPGEN_LDS_READS % HS_HAPGEN_THREADS == 0, "phase 5 of hs_hapgen_group_kernel keeps LDS_READS / THREADS reads per thread");
static_assert(HS_HAPGEN_MAX_DISTINCT + 3 <= HS_HAPGEN_MAX_DISTINCT + 8, "entries of hs_hapgen_copy_kernel");

// ------------------------------------------------------------------------------------------------------------------------ host side
using hipstr::api_fail;

thread_local hipstr::ChunkLast t_last;

int64_t hapgen_ws_bytes(double ws_mib){ return hipstr::chunk_budget(ws_mib, "HIPSTR_HAPGEN_WS_MIB", (double)HS_HAPGEN_WS_MIB, (double)HS_HAPGEN_MAX_LOCUS_BYTES); }

// per locus: the route (1 = device) and the workspace it takes
void hapgen_costs(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, std::vector<uint8_t>& dev, std::vector<int64_t>& cost){
  const int nl = b->n_loci;
  dev.assign((size_t)nl, 0); cost.assign((size_t)nl, 0);
  for (int l = 0; l < nl; l++){
    const int r0 = b->read_off[l], r1 = b->read_off[l+1];
    const int64_t bases = r1 > r0 ? (int64_t)b->base_off[r1] - b->base_off[r0] : 0, runs = r1 > r0 ? (int64_t)b->cigar_off[r1] - b->cigar_off[r0] : 0;
    const int64_t bytes = hs_hapgen_locus_bytes(r1 - r0, bases, runs, (int64_t)rq->win_off[l+1] - rq->win_off[l]);
    dev[l] = hs_hapgen_on_device(r1 - r0, rq->n_samples[l], bytes) ? 1 : 0;
    cost[l] = dev[l] ? bytes : HS_HAPGEN_LOCUS_FIXED;
  }
}

// outputs for a call of check() alone: never written
struct NoOutputs {
  int32_t x = 0; char c = 0; hipstr_hapgen_out_t o;
  NoOutputs(){
    memset(&o, 0, sizeof o);
    o.status = o.blk_start = o.blk_end = o.blk_nopts = o.opt_off = o.n_spanning = o.n_samples_spanning = o.n_distinct = o.left_trim = o.right_trim = o.min_aln_start =
      o.max_aln_stop = &x; o.seq = &c;
  }
};

int hapgen_fail(const char* who, const std::string& err){ return api_fail(std::string(who) + ": " + err); }

int hapgen_device(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, const int32_t* stop_all, hipstr_hapgen_out_t* out){
  const int nl = b->n_loci;
  hipstr::Ctx* ctx = hipstr::api_current_ctx();
  if (!ctx) return 1;
  if (hipstr::api_bind(ctx)) return 1;
  hipStream_t st = hipstr::ctx_stream(ctx);
  hipstr::ChunkLast last;
  t_last = last;                                  // a call that fails on the way reports zeros, not the call before it
  int hash_bits = 64;
  if (const char* e = getenv("HIPSTR_DEBUG_HAPGEN_HASH_BITS")){ const int v = atoi(e); if (v >= 1 && v < 64) hash_bits = v; }
  const bool timing = getenv("HIPSTR_HAPGEN_TIMING") != NULL;
  const int64_t budget = hapgen_ws_bytes(0.0);
  std::vector<uint8_t> dev; std::vector<int64_t> cost;
  if (nl) hapgen_costs(b, rq, dev, cost);
  hipstr_hg::Sink sink{out, 0, 0, 0};
  out->opt_off[0] = 0;
  const int n0 = nl ? b->read_off[0] : 0;
  const int32_t* stop = stop_all - n0;
  std::vector<int32_t> lread;
  for (int l0 = 0; l0 < nl; ){
    const int l1 = hs_pool_chunk_end(cost.data(), l0, nl, budget), nlc = l1 - l0;
    lread.assign((size_t)nlc + 1, 0);
    int64_t n64 = 0, B = 0, NC = 0, W = 0; int max_reads = 0, max_samp = 0;
    for (int l = l0; l < l1; l++){
      const int r0 = b->read_off[l], r1 = b->read_off[l+1];
      if (dev[l] && r1 > r0){
        n64 += r1 - r0; B += (int64_t)b->base_off[r1] - b->base_off[r0]; NC += (int64_t)b->cigar_off[r1] - b->cigar_off[r0];
        max_reads = std::max(max_reads, r1 - r0); max_samp = std::max(max_samp, rq->n_samples[l]);
        W += (int64_t)rq->win_off[l+1] - rq->win_off[l];
      }
      lread[(size_t)(l - l0) + 1] = (int32_t)n64;
    }
    if (2*B + 2*W > INT32_MAX || n64 + 3*(int64_t)nlc + 1 > INT32_MAX) return api_fail("hipstr_hapgen: a chunk of more than 2^31 bytes (lower HIPSTR_HAPGEN_WS_MIB)");
    const size_t n = (size_t)n64, NL = (size_t)nlc;
    hipstr::ChunkBlocks K(ctx, st);
    size_t o_lres = 0, o_eo = 0, o_el = 0, o_dl = 0, o_dr = 0, o_dn = 0, o_ds = 0, o_df = 0, o_oo = 0, o_seq = 0;
    std::vector<int32_t> l_first_opt;
    if (n > 0){
      last.v[3]++; last.v[4] += (int64_t)n;
      // uploaded | workspace | results
      const size_t u_start = K.take(n*4), u_stop = K.take(n*4), u_boff = K.take(n*4), u_coff = K.take((n + 1)*4), u_samp = K.take(n*4), u_rl = K.take(n*4),
                   u_use = K.take(n), u_clen = K.take((size_t)NC*4), u_cop = K.take((size_t)NC), u_bases = K.take((size_t)B), u_lro = K.take((NL + 1)*4),
                   u_rs0 = K.take(NL*4), u_rp0 = K.take(NL*4), u_per = K.take(NL*4), u_ns = K.take(NL*4), u_cf = K.take(NL*4), u_woff = K.take((NL + 1)*4),
                   u_win = K.take((size_t)W), u_bnd = K.take(NL*16);
      K.end_upload();
      const size_t w_hash = K.take(n*8), w_osrc = K.take((n + NL)*4), w_olen = K.take((n + NL)*4), w_lopt = K.take((NL + 1)*4), w_lseq = K.take((NL + 1)*4);
      K.begin_results();
      o_lres = K.take(NL*HS_HAPGEN_LRES*4); o_eo = K.take(n*4); o_el = K.take(n*4); o_dl = K.take(n*4); o_dr = K.take(n*4); o_dn = K.take(n*4); o_ds = K.take(n*4);
      o_df = K.take(n*8); o_oo = K.take((n + 3*NL + 1)*4); o_seq = K.take((size_t)(B + W));
      if (K.reserve()) return 1;
      const auto t0 = std::chrono::steady_clock::now();
      {
        char* U = K.pin_up;
        int32_t* h_start = (int32_t*)(U + u_start), *h_stop = (int32_t*)(U + u_stop), *h_boff = (int32_t*)(U + u_boff), *h_coff = (int32_t*)(U + u_coff),
               * h_samp = (int32_t*)(U + u_samp), *h_rl = (int32_t*)(U + u_rl), *h_clen = (int32_t*)(U + u_clen), *h_rs0 = (int32_t*)(U + u_rs0),
               * h_rp0 = (int32_t*)(U + u_rp0), *h_per = (int32_t*)(U + u_per), *h_ns = (int32_t*)(U + u_ns), *h_cf = (int32_t*)(U + u_cf),
               * h_woff = (int32_t*)(U + u_woff), *h_bnd = (int32_t*)(U + u_bnd);
        uint8_t* h_use = (uint8_t*)(U + u_use);
        memcpy(U + u_lro, lread.data(), (NL + 1)*4);
        size_t i = 0; int64_t boff = 0, coff = 0, woff = 0;
        for (int l = l0; l < l1; l++){
          const int lc = l - l0, r0 = b->read_off[l], r1 = b->read_off[l+1];
          const bool up = dev[l] && r1 > r0;
          h_rs0[lc] = rq->region_start[l]; h_rp0[lc] = rq->region_stop[l]; h_per[lc] = rq->period[l]; h_ns[lc] = rq->n_samples[l];
          h_cf[lc] = hs_hapgen_status(rq->region_start[l], rq->region_stop[l], rq->chrom_len[l], INT64_MIN/2, INT64_MAX/2) == 1 ? 1 : 0;
          h_bnd[4*lc] = INT32_MAX; h_bnd[4*lc+1] = INT32_MIN; h_bnd[4*lc+2] = INT32_MAX; h_bnd[4*lc+3] = INT32_MIN;
          h_woff[lc] = (int32_t)woff;
          if (!up) continue;
          const int64_t wl = (int64_t)rq->win_off[l+1] - rq->win_off[l];
          if (wl) memcpy(U + u_win + woff, rq->window + rq->win_off[l], (size_t)wl);
          woff += wl;
          const int64_t nb = (int64_t)b->base_off[r1] - b->base_off[r0], ncg = (int64_t)b->cigar_off[r1] - b->cigar_off[r0];
          if (nb) memcpy(U + u_bases + boff, b->bases + b->base_off[r0], (size_t)nb);
          if (ncg){ memcpy(U + u_cop + coff, b->cigar_op + b->cigar_off[r0], (size_t)ncg); memcpy(h_clen + coff, b->cigar_len + b->cigar_off[r0], (size_t)ncg*4); }
          for (int r = r0; r < r1; r++, i++){
            h_start[i] = b->read_start[r]; h_stop[i] = stop[r]; h_boff[i] = (int32_t)(boff + (b->base_off[r] - b->base_off[r0]));
            h_coff[i] = (int32_t)(coff + (b->cigar_off[r] - b->cigar_off[r0])); h_samp[i] = rq->sample_label[r]; h_rl[i] = lc;
            h_use[i] = (!rq->use_read || rq->use_read[r]) ? 1 : 0;
          }
          boff += nb; coff += ncg;
        }
        h_coff[n] = (int32_t)coff; h_woff[nlc] = (int32_t)woff;
      }
      last.t[3] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      hs_hapgen_dev_t d; memset(&d, 0, sizeof d);
      char* D = K.dev;
      d.start = (const int32_t*)(D + u_start); d.stop = (const int32_t*)(D + u_stop); d.boff = (const int32_t*)(D + u_boff); d.coff = (const int32_t*)(D + u_coff);
      d.sample = (const int32_t*)(D + u_samp); d.rlocus = (const int32_t*)(D + u_rl); d.use = (const uint8_t*)(D + u_use); d.clen = (const int32_t*)(D + u_clen);
      d.cop = D + u_cop; d.bases = D + u_bases; d.lread_off = (const int32_t*)(D + u_lro); d.rs0 = (const int32_t*)(D + u_rs0); d.rp0 = (const int32_t*)(D + u_rp0);
      d.period = (const int32_t*)(D + u_per); d.nsamp = (const int32_t*)(D + u_ns); d.chrom_fail = (const int32_t*)(D + u_cf); d.woff = (const int32_t*)(D + u_woff);
      d.window = D + u_win; d.bounds = (int32_t*)(D + u_bnd);
      d.hash = (uint64_t*)(D + w_hash); d.osrc = (int32_t*)(D + w_osrc); d.olen = (int32_t*)(D + w_olen); d.l_opt = (int32_t*)(D + w_lopt); d.l_seq = (int32_t*)(D + w_lseq);
      d.lres = (int32_t*)(D + o_lres); d.ext_off = (int32_t*)(D + o_eo); d.ext_len = (int32_t*)(D + o_el); d.dist_len = (int32_t*)(D + o_dl); d.dist_rep = (int32_t*)(D + o_dr);
      d.dist_reads = (int32_t*)(D + o_dn); d.dist_strong = (int32_t*)(D + o_ds); d.dist_frac = (double*)(D + o_df); d.opt_off = (int32_t*)(D + o_oo); d.seq = D + o_seq;
      d.n = (int32_t)n; d.nl = nlc; d.hash_bits = hash_bits;
      const size_t lds = hs_hapgen_lds_bytes(max_reads, max_samp);
      // (the largest size there is, the same in every call: calls of several threads cannot lower it under one another's launch)
      HS_HIP(hipFuncSetAttribute((const void*)hs_hapgen_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)hs_hapgen_lds_bytes(HS_HAPGEN_LDS_READS, HS_HAPGEN_MAX_SAMPLES)));
      if (K.upload(timing)) return 1;
      hipLaunchKernelGGL(hs_hapgen_extract_kernel, dim3((unsigned)((n + HG_NT - 1)/HG_NT)), dim3(HG_NT), 0, st, d);
      hipLaunchKernelGGL(hs_hapgen_hash_kernel, dim3((unsigned)((n + HG_NT/64 - 1)/(HG_NT/64))), dim3(HG_NT), 0, st, d);
      hipLaunchKernelGGL(hs_hapgen_group_kernel, dim3((unsigned)nlc), dim3(HG_NT), lds, st, d);
      hipLaunchKernelGGL(hs_hapgen_scan_kernel, dim3(1), dim3(HG_NT), 0, st, d);
      hipLaunchKernelGGL(hs_hapgen_copy_kernel, dim3((unsigned)nlc), dim3(HG_NT), 0, st, d);
      HS_HIP(hipGetLastError());
      if (K.fetch(timing, &last.t[0])) return 1;
      last.t[1] += (double)K.up_bytes; last.t[2] += (double)K.res_bytes();
      // where a device locus' options start in the chunk's opt_off: the options of the finished loci in front of it
      l_first_opt.assign(NL + 1, 0);
      const int32_t* lres = K.host<int32_t>(o_lres);
      for (int lc = 0; lc < nlc; lc++){
        const int32_t* res = lres + HS_HAPGEN_LRES*lc;
        const bool done = lread[lc+1] > lread[lc] && res[HS_HG_STATUS] == 0 && res[HS_HG_REDO] == 0;
        l_first_opt[lc+1] = l_first_opt[lc] + (done ? res[HS_HG_NOPTS] + 2 : 0);
      }
    }
    for (int l = l0; l < l1; l++){
      const int lc = l - l0, r0 = b->read_off[l], nr = b->read_off[l+1] - r0;
      if (!dev[l]){ last.v[1]++; hipstr_hg::locus_host(b, rq, stop_all, l, sink); continue; }
      if (nr == 0){ last.v[0]++; hipstr_hg::locus_host(b, rq, stop_all, l, sink); continue; }
      const int32_t* res = K.host<int32_t>(o_lres) + HS_HAPGEN_LRES*lc;
      if (res[HS_HG_REDO] == 2){ last.v[1]++; hipstr_hg::locus_host(b, rq, stop_all, l, sink); continue; }
      if (res[HS_HG_REDO]){ last.v[2]++; hipstr_hg::locus_host(b, rq, stop_all, l, sink); continue; }
      last.v[0]++;
      const int cr0 = lread[lc];
      out->status[l] = res[HS_HG_STATUS]; out->min_aln_start[l] = res[HS_HG_MIN]; out->max_aln_stop[l] = res[HS_HG_MAX];
      out->n_spanning[l] = res[HS_HG_SPAN]; out->n_samples_spanning[l] = res[HS_HG_SAMP]; out->n_distinct[l] = res[HS_HG_DIST];
      out->left_trim[l] = res[HS_HG_LT]; out->right_trim[l] = res[HS_HG_RT];
      if (out->ext_off) memcpy(out->ext_off + r0, K.host<int32_t>(o_eo) + cr0, (size_t)nr*4);
      if (out->ext_len) memcpy(out->ext_len + r0, K.host<int32_t>(o_el) + cr0, (size_t)nr*4);
      if (res[HS_HG_STATUS] != 0){
        for (int k = 0; k < 3; k++) out->blk_start[3*l+k] = out->blk_end[3*l+k] = out->blk_nopts[3*l+k] = 0;
        continue;
      }
      const int nopts = res[HS_HG_NOPTS], D = res[HS_HG_DIST];
      out->blk_start[3*l] = res[HS_HG_B0S]; out->blk_end[3*l] = res[HS_HG_B1S]; out->blk_nopts[3*l] = 1;
      out->blk_start[3*l+1] = res[HS_HG_B1S]; out->blk_end[3*l+1] = res[HS_HG_B1E]; out->blk_nopts[3*l+1] = nopts;
      out->blk_start[3*l+2] = res[HS_HG_B1E]; out->blk_end[3*l+2] = res[HS_HG_B2E]; out->blk_nopts[3*l+2] = 1;
      const int32_t* co = K.host<int32_t>(o_oo) + l_first_opt[lc];
      const int ne = nopts + 2, q0 = co[0], qn = co[ne] - q0;
      for (int e = 0; e < ne; e++) out->opt_off[sink.opts + e + 1] = (int32_t)(sink.seq + (co[e+1] - q0));
      if (qn) memcpy(out->seq + sink.seq, K.host<char>(o_seq) + q0, (size_t)qn);
      sink.opts += ne; sink.seq += qn;
      if (out->dist_len) memcpy(out->dist_len + sink.dist, K.host<int32_t>(o_dl) + cr0, (size_t)D*4);
      if (out->dist_reads) memcpy(out->dist_reads + sink.dist, K.host<int32_t>(o_dn) + cr0, (size_t)D*4);
      if (out->dist_strong) memcpy(out->dist_strong + sink.dist, K.host<int32_t>(o_ds) + cr0, (size_t)D*4);
      if (out->dist_frac) memcpy(out->dist_frac + sink.dist, K.host<double>(o_df) + cr0, (size_t)D*8);
      if (out->dist_rep){ const int32_t* dr = K.host<int32_t>(o_dr) + cr0; for (int k = 0; k < D; k++) out->dist_rep[sink.dist + k] = dr[k] - cr0 + r0; }
      sink.dist += D;
    }
    l0 = l1;
  }
  t_last = last;
  return 0;
}

}  // namespace

extern "C" int hipstr_hapgen_host(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, hipstr_hapgen_out_t* out){
  std::vector<int32_t> stop; std::string err;
  if (hipstr_hg::check(b, rq, out, false, stop, err)) return hapgen_fail("hipstr_hapgen_host", err);
  hipstr_hg::hapgen_host(b, rq, stop.data(), out);
  return 0;
}

extern "C" int hipstr_hapgen(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, hipstr_hapgen_out_t* out){
  std::vector<int32_t> stop; std::string err;
  if (hipstr_hg::check(b, rq, out, false, stop, err)) return hapgen_fail("hipstr_hapgen", err);
  return hapgen_device(b, rq, stop.data(), out);
}

extern "C" const char* hipstr_hapgen_status_message(int32_t status){
  return status == 0 ? "" : status == 1 ? "Haplotype blocks are too near to the chromosome ends" : status == 2 ? "No spanning alignments" : NULL;
}

extern "C" hipstr_hapgen_batch_t* hipstr_hapgen_batch(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, uint32_t flags){
  if (!b || !rq){ api_fail("hipstr_hapgen_batch: null argument"); return NULL; }
  if (flags & ~(uint32_t)HIPSTR_HAPGEN_ON_HOST){ api_fail("hipstr_hapgen_batch: unknown flag"); return NULL; }
  if (b->n_loci > 0 && !b->quals){ api_fail("hipstr_hapgen_batch: null table in a batch with loci"); return NULL; }
  std::vector<int32_t> stop;
  { NoOutputs none; std::string err; if (hipstr_hg::check(b, rq, &none.o, true, stop, err)){ hapgen_fail("hipstr_hapgen_batch", err); return NULL; } }
  hipstr_hg::Arrays A(b, rq);                                          // (sized from tables the check has been through)
  if (flags & HIPSTR_HAPGEN_ON_HOST) hipstr_hg::hapgen_host(b, rq, stop.data(), &A.out);
  else if (hapgen_device(b, rq, stop.data(), &A.out)) return NULL;
  return hipstr_hg::assemble_batch(b, rq, &A.out);
}
extern "C" const hipstr_batch_t* hipstr_hapgen_batch_batch(const hipstr_hapgen_batch_t* h){ return h ? &h->batch : NULL; }
extern "C" const int32_t* hipstr_hapgen_batch_locus(const hipstr_hapgen_batch_t* h){ return h ? h->locus : NULL; }
extern "C" const int32_t* hipstr_hapgen_batch_status(const hipstr_hapgen_batch_t* h){ return h ? h->status : NULL; }
extern "C" void hipstr_hapgen_batch_free(hipstr_hapgen_batch_t* h){ delete h; }

#ifndef HIPSTR_NO_DEBUG_ABI
extern "C" int hipstr_debug_hapgen_last(int64_t out[8]){
  if (!out) return api_fail("hipstr_debug_hapgen_last: null argument");
  memcpy(out, t_last.v, sizeof t_last.v);
  return 0;
}
extern "C" int hipstr_debug_hapgen_last_timing(double out[4]){
  if (!out) return api_fail("hipstr_debug_hapgen_last_timing: null argument");
  memcpy(out, t_last.t, sizeof t_last.t);
  return 0;
}

extern "C" int hipstr_debug_hapgen_plan(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, double ws_mib, char* json, int cap){
  if (!b || !rq){ api_fail("hipstr_debug_hapgen_plan: null argument"); return -1; }
  { NoOutputs none; std::vector<int32_t> stop; std::string err; if (hipstr_hg::check(b, rq, &none.o, false, stop, err)){ hapgen_fail("hipstr_debug_hapgen_plan", err); return -1; } }
  const int nl = b->n_loci;
  const int64_t budget = hapgen_ws_bytes(ws_mib);
  std::vector<uint8_t> dev; std::vector<int64_t> cost;
  if (nl) hapgen_costs(b, rq, dev, cost);
  std::string s = "{\"thresholds\": {";
  const std::pair<const char*, int64_t> th[] = {
    {"HS_HAPGEN_THREADS", HS_HAPGEN_THREADS}, {"HS_HAPGEN_LDS_READS", HS_HAPGEN_LDS_READS}, {"HS_HAPGEN_MAX_SAMPLES", HS_HAPGEN_MAX_SAMPLES},
    {"HS_HAPGEN_MAX_DISTINCT", HS_HAPGEN_MAX_DISTINCT}, {"HS_HAPGEN_HASH_STEP", HS_HAPGEN_HASH_STEP}, {"HS_HAPGEN_MIN_SLOTS", HS_HAPGEN_MIN_SLOTS},
    {"HS_HAPGEN_WS_MIB", HS_HAPGEN_WS_MIB}, {"HS_HAPGEN_READ_FIXED", HS_HAPGEN_READ_FIXED}, {"HS_HAPGEN_LOCUS_FIXED", HS_HAPGEN_LOCUS_FIXED},
    {"HS_HAPGEN_MAX_LOCUS_BYTES", HS_HAPGEN_MAX_LOCUS_BYTES} };
  for (size_t i = 0; i < sizeof th/sizeof th[0]; i++){ if (i) s += ", "; s += std::string("\"") + th[i].first + "\": " + std::to_string(th[i].second); }
  s += "}, \"budget_bytes\": " + std::to_string(budget) + ", \"max_lds_bytes\": " + std::to_string((int64_t)hs_hapgen_lds_bytes(HS_HAPGEN_LDS_READS, HS_HAPGEN_MAX_SAMPLES)) +
       ", \"routes\": [\"device\", \"host\"], \"chunks\": [";
  bool hit[2] = { false, false };
  for (int l0 = 0; l0 < nl; ){
    const int l1 = hs_pool_chunk_end(cost.data(), l0, nl, budget);
    int64_t reads = 0, bytes = 0, nd = 0, nh = 0; int max_reads = 0, max_samp = 0;
    for (int l = l0; l < l1; l++){
      bytes += cost[l];
      if (!dev[l]){ nh++; hit[1] = true; continue; }
      nd++; hit[0] = true;
      const int nr = b->read_off[l+1] - b->read_off[l];
      reads += nr; max_reads = std::max(max_reads, nr); if (nr) max_samp = std::max(max_samp, rq->n_samples[l]);
    }
    if (l0) s += ", ";
    s += "{\"l0\": " + std::to_string(l0) + ", \"l1\": " + std::to_string(l1) + ", \"reads\": " + std::to_string(reads) + ", \"bytes\": " + std::to_string(bytes) +
         ", \"device_loci\": " + std::to_string(nd) + ", \"host_loci\": " + std::to_string(nh) + ", \"lds_bytes\": " +
         std::to_string(reads ? (int64_t)hs_hapgen_lds_bytes(max_reads, max_samp) : 0) + "}";
    l0 = l1;
  }
  s += "], \"routes_hit\": [";
  if (hit[0]) s += "\"device\"";
  if (hit[1]) s += std::string(hit[0] ? ", " : "") + "\"host\"";
  s += "]}";
  if (json && cap > 0){ const size_t k = std::min((size_t)cap - 1, s.size()); memcpy(json, s.data(), k); json[k] = 0; }
  return (int)s.size();
}
#endif  // HIPSTR_NO_DEBUG_ABI
