// trace.hip — Viterbi traceback of one read against one fixed haplotype on gfx950.
//
// Replaces HapAligner::trace_optimal_aln (HapAligner.cpp:711-722): process_read(retrace_aln = true) on ONE haplotype
// (HapAligner.cpp:573-709) = full M/I/D matrices of the left and the right problem, compute_aln_logprob with its
// arg-max seed position (HapAligner.cpp:163-231), HapAligner::retrace (HapAligner.cpp:363-571) from that position, and
// stitch_alignment_trace (AlignmentTraceback.cpp:55-144).
//
//   hs_trace_fill<C>   one wavefront per (request, side) runs a systolic anti-diagonal flank sweep (a traceback is one
//                      read against one allele: nothing but its own columns to put on the lanes).  The reference keeps the full M/I/D matrices and lets retrace compare neighbours; every such
//                      comparison only involves operands the sweep has in registers when it computes the cell, so the sweep
//                      takes retrace's three decisions right there (with its 0.001-nat, direction-dependent tie rules) and
//                      HBM receives ONE BYTE per cell instead of 24 (compact rows: the interior rows of the STR block, which
//                      nothing ever reads, do not exist), plus the last column of M for the seed arg-max.  The STR row is
//                      evaluated one read column per lane by replaying the host-enumerated visiting lists, remembering the
//                      best artifact size and position (HapAligner.cpp:81-97, StutterAlignerClass.cpp:92-95,138-141).
//   hs_trace_walk      one wavefront per request: seed arg-max + log-sum-exp over the lanes, then lane 0 walks the
//                      left matrices and lane 1 the right ones, emitting the operation strings.
//
// trace_optimal_aln positions the haplotype with go_to(), which clears last_changed_, so NOTHING is reused: rows are built
// under the allele's own homopolymer context (prep.h fresh_flank_rows), unlike the forward pass.
// The host then replays the operation strings into the flat hipstr_trace_out_t (the bookkeeping of retrace that touches
// no matrix: flank sequences, SNPs, indels, STR sequence) and stitches them with the haplotype-to-reference strings.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "layout.h"
#include "device_common.h"
#include "prep.h"
#include "api_internal.h"

struct hs_tside_t {               // one side of one request
  int32_t base_off, len, seed;    // the read in the base/quality pools
  int32_t side;                   // 0 = left problem (forward haplotype), 1 = right problem (reversed read and haplotype)
  int32_t n;                      // read columns on this side
  int32_t lead_off, F0;           // rows of the leading flank in this orientation
  int32_t trail_off, F2;
  int32_t stropt;
  int32_t art_off;                // ints: art_size[n] | art_pos[n]
  int32_t ops_off, ops_cap;
  int32_t pad_;
  int32_t lc_off;                 // doubles: last column of M per compact row (F0 + 1 + F2; row F0 is the STR block's last row)
  int32_t pad2_;
  int64_t dec_off;                // bytes: retrace's decisions per cell, (F0 + 1 + F2) x n: bits 0-1 from M, bit 2 from D, bit 3 from I
};

struct hs_tdev_t {
  const hs_tside_t*  sides;       // [2*n_req]: left, right of each request
  const int32_t*     items;       // side indices grouped by columns-per-lane class
  const hs_row_t*    rows;
  const hs_stropt_t* stropts;
  const hs_visit_t*  visits;
  const double*      f64pool;
  const char*        chars;
  const char*        bases;
  const char*        quals;
  const double *int_log, *qual_correct, *qual_error, *m2m, *m2i;
  double             log_thresh;
  uint8_t*           dec;
  double*            lastcol;
  int32_t*           arts;
  char*              ops;
  double*            side_prob;   // [2*n_req]
  double*            ll;          // [n_req]
  int32_t*           max_index;   // [n_req]
  int32_t*           n_ops;       // [2*n_req]
  int32_t*           str_size;    // [2*n_req] artifact size taken in the STR block, or HIPSTR_NO_STR_DATA
  int32_t*           str_pos;     // [2*n_req]
};

namespace {

constexpr double TRACE_LL_TOL = 0.001;     // HapAligner.cpp:345

template <int C> struct TraceLdsStore {     // LDS of one fill wavefront, sized by its columns-per-lane class (n <= 64*C)
  double blc[64*C], blw[64*C];
  double prev[64*C];                       // M of the row before the STR block
  double mr[64*C];                         // M of the STR block's last row
  double Mt[64*C];                         // StutterAlignerClass match table
  double Dl[64*C*HS_MAXREP];
  double In[64*C*HS_MAXREP];
  double terms[HS_NART*64];
  uint8_t rd[64*C];
  uint8_t blk[HS_MAX_STR_BP + 1];
};
struct TraceLds {                          // view of a TraceLdsStore<C>
  double *blc, *blw, *prev, *mr, *Mt, *Dl, *In, *terms;
  uint8_t *rd, *blk;
};

__device__ __forceinline__ double emit_l(const TraceLds& L, int x, uint8_t c){ return L.rd[x] == c ? L.blc[x] : L.blw[x]; }

// Closed form for a "simple" visiting list (hs_stropt_t::shape = U0 >= 0, the same evaluator as the forward pass, hmm_kernels.hip
// simple_eval): every pushed value is lp0 plus a constant.  Pushes, in the reference's order: lp0 | [0 < lim] ln(U0) + lp0 (run of U0
// equal configurations, only if U0 > 0) | lp0 once per plain offset in [U0, lim) | [stop < tail] ln(tail - stop) + lp0.  The running
// likelihood never changes along such a list, so the best position is the start (right-aligned) or the last offset visited
// (left-aligned: ties move it, StutterAlignerClass.cpp:92-95, 138-141) = `stop`.
__device__ __forceinline__ double trace_simple(const hs_tdev_t& d, double lp0, int lim, int U0, int tail, bool left_align, int& best_pos){
  const bool skip = (U0 > 0) && (lim > 0);
  const int nplain = max(0, lim - U0);
  const int stop = (lim <= 0) ? 0 : ((U0 > 0 && lim <= U0) ? U0 : lim);
  const bool has_tail = stop < tail;
  const double v_skip = d.int_log[U0] + lp0;
  const double v_tail = d.int_log[max(tail - stop, 0)] + lp0;
  double mx = lp0;
  if (skip) mx = fmax(mx, v_skip);
  if (has_tail) mx = fmax(mx, v_tail);
  double tot = 0.0;
  { const double dd = lp0 - mx; if (dd > d.log_thresh) tot += (double)(1 + nplain) * (double)f_fasterexp((float)dd); }
  if (skip){ const double dd = v_skip - mx; if (dd > d.log_thresh) tot += (double)f_fasterexp((float)dd); }
  if (has_tail){ const double dd = v_tail - mx; if (dd > d.log_thresh) tot += (double)f_fasterexp((float)dd); }
  best_pos = left_align ? stop : 0;
  return mx + (double)f_fasterlog((float)tot);
}

// StutterAlignerClass::align_pcr_insertion_reverse (StutterAlignerClass.cpp:59-104) for one read column.
__device__ double trace_ins(const hs_tdev_t& d, const TraceLds& L, const hs_stropt_t& so, const double* f64, int n, int len, int j, int D,
                            bool left_align, int& best_pos){
  const int B = so.B, p = so.period, off = n-1-j;
  const double lp0 = f64[HS_NART] + L.In[HS_MAXREP*off + D/p - 1] + (len > D ? L.Mt[off+D] : 0.0);
  const int lim = min(max(len-D, 0), B);
  if (so.shape[HS_MAXREP] >= 0) return trace_simple(d, lp0, lim, so.shape[HS_MAXREP], B, left_align, best_pos);
  Lse lse;
  double best = lp0; best_pos = 0;
  for (int pass = 0; pass < 2; pass++){
    double lp = lp0;
    lse.start(pass, lp);
    lse.push(pass, lp, d.log_thresh);
    const hs_visit_t* e = d.visits + so.ins_off;
    int ni;
    for (;; e++){
      const uint64_t meta = e->meta;
      ni = (int)(meta & 0xffff);
      if (ni >= lim) break;
      const int U = (int)((meta >> 16) & 0xffff);
      int pos = 1 + ni;
      double v;
      if ((meta >> 48) & 1) v = lp;
      else if (U == 0){
        const uint8_t ca = (uint8_t)(meta >> 32), cb = (uint8_t)(meta >> 40);
        for (int idx = -ni-p; idx >= -ni-D; idx -= p){
          lp -= emit_l(L, j+idx, ca);
          lp += emit_l(L, j+idx, cb);
        }
        v = lp;
      } else { v = e->logU + lp; pos = ni + U; }
      lse.push(pass, v, d.log_thresh);
      if (pass == 0 && (lp > best || (left_align && lp == best))){ best_pos = pos; best = lp; }
    }
    if (ni < B) lse.push(pass, d.int_log[B-ni] + lp, d.log_thresh);
  }
  return lse.finish();
}

// StutterAlignerClass::align_pcr_deletion_reverse (StutterAlignerClass.cpp:106-150) for one read column.
__device__ double trace_del(const hs_tdev_t& d, const TraceLds& L, const hs_stropt_t& so, const double* f64, int n, int len, int j, int D,
                            bool left_align, int& best_pos){
  const int B = so.B, p = so.period, off = n-1-j, q = -D/p - 1;
  double lp0 = f64[HS_NART+1+q];
  if (off + D >= 0) lp0 += L.Mt[off+D] - L.Dl[(off+D)*HS_MAXREP + q];
  else for (int k = 0; k > -len; k--) lp0 += emit_l(L, j+k, L.blk[B-1+k+D]);
  if (so.shape[q] >= 0) return trace_simple(d, lp0, len, so.shape[q], B+D, left_align, best_pos);
  Lse lse;
  double best = lp0; best_pos = 0;
  for (int pass = 0; pass < 2; pass++){
    double lp = lp0;
    lse.start(pass, lp);
    lse.push(pass, lp, d.log_thresh);
    const hs_visit_t* e = d.visits + so.del_off[q];
    int ni;
    for (;; e++){
      const uint64_t meta = e->meta;
      ni = (int)(meta & 0xffff);
      if (ni >= len) break;
      const int U = (int)((meta >> 16) & 0xffff);
      int pos = 1 + ni;
      double v;
      if (U == 0){
        const uint8_t ca = (uint8_t)(meta >> 32), cb = (uint8_t)(meta >> 40);
        lp -= emit_l(L, j-ni, ca);
        lp += emit_l(L, j-ni, cb);
        v = lp;
      } else { v = e->logU + lp; pos = ni + U; }
      lse.push(pass, v, d.log_thresh);
      if (pass == 0 && (lp > best || (left_align && lp == best))){ best_pos = pos; best = lp; }
    }
    if (ni < B+D) lse.push(pass, d.int_log[B+D-ni] + lp, d.log_thresh);
  }
  return lse.finish();
}

__device__ __forceinline__ int tri_idx(bool rev, double v1, double v2, double v3){       // HapAligner.cpp:346-358
  if (!rev){ if (v1 > v2+TRACE_LL_TOL) return (v1 > v3+TRACE_LL_TOL ? 0 : 2); return (v2 > v3+TRACE_LL_TOL ? 1 : 2); }
  if (v3 > v2+TRACE_LL_TOL) return (v3 > v1+TRACE_LL_TOL ? 2 : 0);
  return (v2 > v1+TRACE_LL_TOL ? 1 : 0);
}
__device__ __forceinline__ int pair_idx(bool rev, double v1, double v2){                 // HapAligner.cpp:360-361
  if (!rev) return (v1 > v2+TRACE_LL_TOL ? 0 : 1);
  return (v2 > v1+TRACE_LL_TOL ? 1 : 0);
}

// ------------------------------------------------------------------ decisions of one (request, side)
template <int C>
__device__ __forceinline__ void trace_fill_body(TraceLdsStore<C>& store, const hs_tdev_t* __restrict__ dp, int item_begin){
  TraceLds L;
  L.blc = store.blc; L.blw = store.blw; L.prev = store.prev; L.mr = store.mr; L.Mt = store.Mt; L.Dl = store.Dl; L.In = store.In;
  L.terms = store.terms; L.rd = store.rd; L.blk = store.blk;
  const hs_tdev_t& d = *dp;
  const int lane = threadIdx.x;
  const int si = uni(d.items[item_begin + blockIdx.x]);
  const hs_tside_t* S = d.sides + si;
  const int n = uni(S->n), len = uni(S->len), base_off = uni(S->base_off), side = uni(S->side);
  const int F0 = uni(S->F0), F2 = uni(S->F2);
  uint8_t* dec = d.dec + uni(S->dec_off);
  double* lastcol = d.lastcol + uni(S->lc_off);
  const bool rev = side != 0;
  const int nl = (n + C - 1) / C, lastlane = (n - 1) / C;
#ifdef HS_TRACE_TIME        // s_memtime per stage of the first few wavefronts (experiment builds)
  unsigned long long tt[6]; int ti = 0; tt[ti++] = __builtin_amdgcn_s_memtime();
#define HS_TTICK() (tt[ti++] = __builtin_amdgcn_s_memtime())
#else
#define HS_TTICK() ((void)0)
#endif

  uint8_t rd[C]; double blc[C], blw[C];
#pragma unroll
  for (int k = 0; k < C; k++){
    const int j = min(lane*C + k, n-1);
    const int src = base_off + (side ? len - 1 - j : j);
    const uint8_t q = (uint8_t)d.quals[src];
    rd[k] = (uint8_t)d.bases[src];
    blc[k] = d.qual_correct[q]; blw[k] = d.qual_error[q];
    if (lane*C + k < n){ L.rd[j] = rd[k]; L.blc[j] = blc[k]; L.blw[j] = blw[k]; }
  }
  const double tab_m2m = d.m2m[lane & 15], tab_m2i = d.m2i[lane & 15];

  double Mrow[C], Drow[C];
  // rows 1.. of a flank block enter at lane 0, one per step; lane t works on row (step - t); every cell is stored
  auto sweep = [&](const hs_row_t* nr, int nrows){
    const int steps = nrows + nl - 1;
    int chunk = 0;
    uint32_t rowv = (lane < nrows) ? nr[lane] : 0u;
    double oM = 0, oD = 0, oI = 0, om2m = 0, om2i = 0;
    int oMeta = 0;
    for (int st = 0; st < steps; st++){
      int meta0 = 0; double f_m2m = 0, f_m2i = 0;
      if (st < nrows){
        if (st - chunk == 64){ chunk += 64; rowv = (chunk + lane < nrows) ? nr[chunk + lane] : 0u; }
        meta0 = rdlane((int)rowv, st - chunk);
        const int h = (meta0 >> 8) & 15;
        f_m2m = rdlane(tab_m2m, h); f_m2i = rdlane(tab_m2i, h);
      }
      const int meta = shr1(meta0, oMeta);
      const double m2m = shr1(f_m2m, om2m), m2i = shr1(f_m2i, om2i);
      double mdiag = shr1(0.0, oM), ddiag = shr1(0.0, oD), ileft = shr1(0.0, oI);
      if (meta < 0){
        const uint8_t hc = (uint8_t)(meta & 0xff);
        const int64_t ro = (int64_t)((meta >> 12) & 0xfff) * n;
        oM = Mrow[C-1]; oD = Drow[C-1];
#pragma unroll
        for (int kk = 0; kk < C; kk++){
          const double e = (rd[kk] == hc) ? blc[kk] : blw[kk];
          const double c0v = ileft + m2i, c1v = mdiag + m2m, c2v = ddiag + m2i;
          double nM = e + fmax(c0v, fmax(c1v, c2v));
          double nI = blc[kk] + fmax(mdiag + T_I2M, ileft + T_I2I);
          const double dm = Mrow[kk] + T_D2M, ddl = Drow[kk] + T_D2D, ii = ileft + T_I2I, im = mdiag + T_I2M;
          const double nD = fmax(dm, ddl);
          // retrace's choices at this cell (HapAligner.cpp:536-566): from M among (I left, D diag, M diag), from D and from I
          const int code = tri_idx(rev, c0v, c2v, c1v) | (pair_idx(rev, ddl, dm) << 2) | (pair_idx(rev, ii, im) << 3);
          if (kk == 0 && lane == 0){ nM = e; nI = blc[kk]; }     // HapAligner.cpp:123-126
          mdiag = Mrow[kk]; ddiag = Drow[kk]; ileft = nI;
          Mrow[kk] = nM; Drow[kk] = nD;
          const int j = lane*C + kk;
          if (j < n) dec[ro + j] = (uint8_t)code;
          if (j == n-1) lastcol[(meta >> 12) & 0xfff] = nM;
        }
        oI = ileft;
      }
      oMeta = meta; om2m = m2m; om2i = m2i;
    }
  };

  // ---- matrix row 0 (HapAligner.cpp:33-42) and the leading flank
  const hs_row_t* lead = d.rows + uni(S->lead_off);
  {
    const uint8_t c0 = (uint8_t)(uni((int)lead[0]) & 0xff);
    double pre[C];
#pragma unroll
    for (int kk = 0; kk < C; kk++) pre[kk] = 0.0;
    double carry = 0.0;
    for (int t = 0; t < nl; t++){
      const double cin = shr1(0.0, carry);
      if (lane == t){
        double run = (t == 0) ? 0.0 : cin;
#pragma unroll
        for (int kk = 0; kk < C; kk++){ pre[kk] = run; if (lane*C + kk < n) run += blc[kk]; }
        carry = run;
      }
    }
#pragma unroll
    for (int kk = 0; kk < C; kk++){
      Mrow[kk] = ((rd[kk] == c0) ? blc[kk] : blw[kk]) + pre[kk];
      Drow[kk] = IMP;
      if (lane*C + kk == n-1) lastcol[0] = Mrow[kk];
    }
    if (lane == lastlane) d.side_prob[si] = carry;
  }
  if (F0 > 1) sweep(lead + 1, F0 - 1);
#pragma unroll
  for (int kk = 0; kk < C; kk++){ const int j = lane*C + kk; if (j < n) L.prev[j] = Mrow[kk]; }
  HS_TTICK();

  // ---- STR block (HapAligner.cpp:62-109)
  const hs_stropt_t so = d.stropts[uni(S->stropt)];
  const int B = so.B, p = so.period, nd = so.nd;
  const double* f64 = d.f64pool + so.f64_off;
  for (int x = lane; x < B; x += 64) L.blk[x] = (uint8_t)d.chars[so.seq_off + x];
  __syncthreads();
  // StutterAlignerClass::load_read (StutterAlignerClass.cpp:12-53), one table position per lane
  {
    const int maxdel = nd*p, maxins = HS_MAXREP*p;
    for (int i = lane; i < n; i += 64){
      const int e = n-1-i;
      double lp = 0.0;
      int j;
      const int lim = min(n-i, maxdel);
      for (j = 0; j < lim; j++){
        lp += emit_l(L, e-j, L.blk[B-1-j]);
        if ((j+1) % p == 0) L.Dl[i*HS_MAXREP + (j+1)/p - 1] = lp;
      }
      const int lim2 = min(n-i, B);
      for (j = maxdel; j < lim2; j++) lp += emit_l(L, e-j, L.blk[B-1-j]);
      L.Mt[i] = lp;
      double li = 0.0;
      const int lim3 = min(maxins, n-i);
      for (j = 0; j < lim3; j++){
        if (j % p < B) li += emit_l(L, e-j, L.blk[B-1-(j%p)]);
        else           li += L.blc[e-j];
        if ((j+1) % p == 0) L.In[i*HS_MAXREP + (j+1)/p - 1] = li;
      }
      for (; j < maxins; j++) if ((j+1) % p == 0) L.In[i*HS_MAXREP + (j+1)/p - 1] = li;
    }
  }
  __syncthreads();
  HS_TTICK();
  {
    const bool left_align = (side == 0);        // forward: left-align the artifact, reverse: right-align (HapAligner.cpp:69-71)
    int32_t* art_size = d.arts + uni(S->art_off);
    int32_t* art_pos = art_size + n;
    const int64_t ro = (int64_t)F0 * n;
    for (int j = lane; j < n; j += 64){
      int bsize = -10000, bpos = -1;
      double best_ll = IMP;
      for (int t = 0; t < HS_NART; t++){
        const int art = (t - HS_MAXREP)*p;
        const int alen = min(B+art, j+1);
        double term = IMP;
        int apos = -1;
        if (alen >= 0){
          double pr;
          if (art == 0) pr = L.Mt[n-1-j];
          else if (art > 0) pr = trace_ins(d, L, so, f64, n, alen, j, art, left_align, apos);
          else pr = trace_del(d, L, so, f64, n, alen, j, art, left_align, apos);
          const double pre = (j-alen < 0) ? 0.0 : L.prev[j-alen];
          term = f64[t] + pr + pre;
        }
        L.terms[t*64 + lane] = term;
        if (term > best_ll){ bsize = art; bpos = apos; best_ll = term; }
      }
      Lse lse;
      for (int pass = 0; pass < 2; pass++){
        lse.start(pass, L.terms[lane]);
        for (int t = 0; t < HS_NART; t++) lse.push(pass, L.terms[t*64 + lane], d.log_thresh);
      }
      const double v = lse.finish();
      L.mr[j] = v;
      if (j == n-1) lastcol[F0] = v;
      art_size[j] = bsize; art_pos[j] = bpos;
    }
  }
  __syncthreads();
  HS_TTICK();

  // ---- trailing flank: "stutter block must be followed by a match" (HapAligner.cpp:122-139), then the plain recurrence
  const hs_row_t* trail = d.rows + uni(S->trail_off);
  {
    const int t0row = uni((int)trail[0]);
    const uint8_t c0 = (uint8_t)(t0row & 0xff);
    const int h0 = (t0row >> 8) & 15;
    const double a_m2m = d.m2m[h0], a_m2i = d.m2i[h0];
    const int64_t ro = (int64_t)(F0 + 1) * n;
#pragma unroll
    for (int kk = 0; kk < C; kk++){
      const int j = min(lane*C + kk, n-1);
      const double e = (rd[kk] == c0) ? blc[kk] : blw[kk];
      const double mleft = L.mr[max(j - 1, 0)];                 // M of the STR block's last row, previous column
      Mrow[kk] = (j == 0) ? e : e + mleft;
      Drow[kk] = IMP;
      // the neighbours retrace would compare here: I of this row and D of the STR row are IMPOSSIBLE (HapAligner.cpp:130-139)
      const int code = tri_idx(rev, IMP + a_m2i, IMP + a_m2i, mleft + a_m2m) | (pair_idx(rev, IMP + T_D2D, L.mr[j] + T_D2M) << 2)
                     | (pair_idx(rev, IMP + T_I2I, mleft + T_I2M) << 3);
      if (lane*C + kk < n) dec[ro + j] = (uint8_t)code;
      if (lane*C + kk == n-1) lastcol[F0 + 1] = Mrow[kk];
    }
  }
  if (F2 > 1) sweep(trail + 1, F2 - 1);
#ifdef HS_TRACE_TIME
  HS_TTICK();
  if (lane == 0 && blockIdx.x < 4) printf("trace fill side %d (n %d, rows %d + %d, B %d, C %d): lead %llu tables %llu STR row %llu trail %llu cycles\n", si, n, F0, F2, B, C,
                                          tt[1]-tt[0], tt[2]-tt[1], tt[3]-tt[2], tt[4]-tt[3]);
#endif
}
// sides of up to 384 columns (C <= 6): the wavefront's tables are static LDS (under the 64 KiB a kernel may declare)
template <int C>
__global__ void __launch_bounds__(64) hs_trace_fill(const hs_tdev_t* __restrict__ dp, int item_begin){
  __shared__ TraceLdsStore<C> store;
  trace_fill_body<C>(store, dp, item_begin);
}
// The requests of ONE locus are a hundred wavefronts spread over two or three column classes: as launches of their own on side streams the
// classes did not reliably run side by side (end of round 4, rocprofv3 timeline of a 100-request call: 143 us | 245 us beside it | 233 us
// BEHIND it — two of the three streams shared a hardware queue), and a fill kernel is a chain of ~300 dependent steps whatever its size.
// One launch for the classes 1-6 instead: a workgroup picks its class from the launch order's class boundaries and takes the front of the
// largest class's LDS block.  Registers and LDS are the largest class's — irrelevant for a call that fills a fraction of the device; calls
// of many loci keep one launch per class.
struct hs_tcls_t { int32_t end[6]; };          // launch-order index one past the last side of class 1 .. 6
__global__ void __launch_bounds__(64) hs_trace_fill_mixed(const hs_tdev_t* __restrict__ dp, hs_tcls_t cls){
  __shared__ TraceLdsStore<6> store;
  const int b = (int)blockIdx.x;
  if (b < cls.end[0])      trace_fill_body<1>(*(TraceLdsStore<1>*)&store, dp, 0);
  else if (b < cls.end[1]) trace_fill_body<2>(*(TraceLdsStore<2>*)&store, dp, 0);
  else if (b < cls.end[2]) trace_fill_body<3>(*(TraceLdsStore<3>*)&store, dp, 0);
  else if (b < cls.end[3]) trace_fill_body<4>(*(TraceLdsStore<4>*)&store, dp, 0);
  else if (b < cls.end[4]) trace_fill_body<5>(*(TraceLdsStore<5>*)&store, dp, 0);
  else                     trace_fill_body<6>(store, dp, 0);
}
// longer sides, up to the forward pass' 1024 columns (C = 8, 12, 16: 75-146 KiB of tables): dynamic LDS, sized by the launch
// (hipFuncAttributeMaxDynamicSharedMemorySize).  Same body: a read of this length is rare in HipSTR's short-read data and takes the
// lower occupancy; what matters is that the drop-in does not refuse a read the forward pass accepted.
extern __shared__ double hs_trace_dyn_lds[];
template <int C>
__global__ void __launch_bounds__(64) hs_trace_fill_long(const hs_tdev_t* __restrict__ dp, int item_begin){
  trace_fill_body<C>(*(TraceLdsStore<C>*)hs_trace_dyn_lds, dp, item_begin);
}
template <int C> int launch_fill_long(int cnt, hipStream_t ks, const hs_tdev_t* d_args, int first){
  // the attribute belongs to the function on the CURRENT device (hipstr_multi_*: several devices in one process), so it is set on every
  // launch, like api.hip does for the STR kernels: a host-side call of well under a microsecond next to a rare, long kernel
  if (hipFuncSetAttribute((const void*)hs_trace_fill_long<C>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(TraceLdsStore<C>)) != hipSuccess) return 1;
  hipLaunchKernelGGL(hs_trace_fill_long<C>, dim3(cnt), dim3(64), sizeof(TraceLdsStore<C>), ks, d_args, first);
  return 0;
}

// ------------------------------------------------------------------ seed arg-max, total likelihood and the walk
// HapAligner::retrace (HapAligner.cpp:363-571): only the decisions; the bookkeeping is replayed on the host from `ops`.
// dec: the side's decision bytes — the wavefront's LDS copy when the side fits HS_WALK_LDS (a walk is a chain of a few hundred dependent
// one-byte loads: 60 ns each from LDS, ~700 ns from L2 / HBM), else the matrix in the workspace
__device__ void trace_walk(const hs_tdev_t& d, int si, int B, int max_index, const uint8_t* dec){
  const hs_tside_t* S = d.sides + si;
  const bool rev = S->side != 0;
  const int n = S->n, F0 = S->F0, F2 = S->F2;
  const int32_t* art_size = d.arts + S->art_off;
  const int32_t* art_pos = art_size + n;
  char* ops = d.ops + S->ops_off;
  const int cap = S->ops_cap;
  int k = 0;
  auto push = [&](char c){ if (k < cap) ops[k] = c; k++; };
  d.str_size[si] = HIPSTR_NO_STR_DATA; d.str_pos[si] = -1;
  if (max_index == 0){            // HapAligner.cpp:646-648
    for (int i = 0; i < n; i++) push('S');
    d.n_ops[si] = k;
    return;
  }
  const int blen[3] = { F0, B, F2 };
  int sblock = 0, scoord = max_index;
  for (int b = 0; b < 3; b++){ if (scoord < blen[b]){ sblock = b; break; } scoord -= blen[b]; }
  int block, base;
  if (scoord == 0){ block = sblock-1; base = blen[block]-1; } else { block = sblock; base = scoord-1; }
  const int row = max_index - 1;
  int u = row < F0 ? row : (row < F0+B ? F0 : row - B + 1);
  int seq = n-1, c = n-1, type = 0;           // 0 match, 1 deletion, 2 insertion
  while (block >= 0){
    if (block == 1){
      const int size = art_size[seq], apos = art_pos[seq];
      d.str_size[si] = size; d.str_pos[si] = apos;
      int i = 0;
      for (; i < min(seq+1, apos); i++) push('M');
      if (size < 0) for (int x = 0; x < -size; x++) push('D');
      else for (; i < min(seq+1, apos+size); i++) push('I');
      for (; i < min(B+size, seq+1); i++) push('M');
      if (B + size >= seq+1) break;            // the read does not span the STR block
      u = F0 - 1; c -= B + size; seq -= B + size; type = 0;
    } else {
      const hs_row_t* rows = d.rows + (block == 0 ? S->lead_off : S->trail_off);
      bool done = false;
      while (base >= 0 && seq >= 0){
        const int h = (rows[base] >> 8) & 15;
        push(type == 0 ? 'M' : (type == 1 ? 'D' : 'I'));
        if (type == 0){ seq--; base--; } else if (type == 1) base--; else seq--;
        if (seq == -1 || (base == -1 && block == 0)){
          while (seq != -1){ push('S'); seq--; }
          done = true;
          break;
        }
        const int code = dec[(int64_t)u*n + c];                  // taken by the sweep when it computed cell (u, c)
        if (type == 0){
          const int best = code & 3;
          if (best == 0){ type = 2; c -= 1; }
          else { type = (best == 1) ? 1 : 0; u--; c--; }
        } else if (type == 1){
          type = ((code >> 2) & 1) == 0 ? 1 : 0; u--;
        } else {
          if (((code >> 3) & 1) == 0) c--;
          else { type = 0; u--; c--; }
        }
      }
      if (done) break;
    }
    block--;
    if (block >= 0) base = blen[block] - 1;
  }
  d.n_ops[si] = k;
}

#define HS_WALK_LDS 24576          // bytes of decisions per side a walk keeps in LDS (150-bp reads x 60-row flanks: 9 KB)
// decision bytes of a side, and whether hs_trace_walk copies them to LDS (hipstr_debug_trace_plan reports the same)
__host__ __device__ inline int hs_trace_side_bytes(int F0, int F2, int n){ return (F0 + 1 + F2)*n; }
__host__ __device__ inline bool hs_walk_in_lds(int bytes){ return bytes <= HS_WALK_LDS; }
__global__ void __launch_bounds__(64) hs_trace_walk(const hs_tdev_t* __restrict__ dp, int req_begin){
  const hs_tdev_t& d = *dp;
  const int lane = threadIdx.x;
  const int q = req_begin + blockIdx.x;
  const hs_tside_t* SL = d.sides + 2*q;
  const hs_tside_t* SR = SL + 1;
  const int nL = uni(SL->n), nR = uni(SR->n), F0 = uni(SL->F0), F2 = uni(SL->F2);
  const int B = uni(d.stropts[uni(SL->stropt)].B);
  const int H = F0 + B + F2;
  const double* LM = d.lastcol + uni(SL->lc_off);          // last column of M per compact row
  const double* RM = d.lastcol + uni(SR->lc_off);
  const int sp = uni(SL->base_off) + uni(SL->seed);
  const uint8_t sc = (uint8_t)d.bases[sp];
  const uint8_t sq = (uint8_t)d.quals[sp];
  const double lc = d.qual_correct[sq], lw = d.qual_error[sq];
  const double prior = -d.int_log[F0 + F2];
  const double spL = d.side_prob[2*q], spR = d.side_prob[2*q+1];
  auto cL = [&](int r){ return r < F0 ? r : (r < F0+B ? F0 : r - B + 1); };
  auto cR = [&](int r){ return r < F2 ? r : (r < F2+B ? F2 : r - B + 1); };
  auto term = [&](int x){       // compute_aln_logprob (HapAligner.cpp:163-231), one seed position
    const uint32_t rw = x < F0 ? d.rows[SL->lead_off + x] : d.rows[SL->trail_off + x - F0 - B];
    const double pe = prior + (sc == (uint8_t)(rw & 0xff) ? lc : lw);
    if (x == 0)   return (pe + spL) + RM[cR(H-2)];
    if (x == H-1) return (pe + spR) + LM[cL(H-2)];
    return (pe + LM[cL(x-1)]) + RM[cR(H-2-x)];
  };
  // the reference pushes x = 0, x = H-1, then the interior positions in order, keeping the FIRST maximum (HapAligner.cpp:184-222)
  double bv = -__builtin_huge_val(); int brank = 0x7fffffff;
  for (int kk = lane; kk < F0 + F2; kk += 64){
    const int x = kk < F0 ? kk : kk + B;
    const double v = term(x);
    const int rank = x == 0 ? 0 : (x == H-1 ? 1 : x + 1);
    if (v > bv || (v == bv && rank < brank)){ bv = v; brank = rank; }
  }
  const double mx = wave_max_d(bv);
  const int rank = (int)-wave_max_d(-(double)(bv == mx ? brank : 0x7fffffff));
  const int max_index = rank == 0 ? 0 : (rank == 1 ? H-1 : rank - 1);
  double tot = 0.0;
  for (int kk = lane; kk < F0 + F2; kk += 64){
    const int x = kk < F0 ? kk : kk + B;
    const double df = term(x) - mx;
    if (df > d.log_thresh) tot += (double)f_fasterexp((float)df);
  }
  tot = wave_sum_d(tot);
  if (lane == 0){ d.ll[q] = mx + (double)f_fasterlog((float)tot); d.max_index[q] = max_index; }
  // the two sides' decision bytes into LDS, 16 bytes per lane and step (hipstr_hmm_trace aligns the matrices to 16 bytes)
  __shared__ uint4 s_dec[2][HS_WALK_LDS/16];
  const uint8_t* decp[2];
#pragma unroll
  for (int sd = 0; sd < 2; sd++){
    const hs_tside_t* S = SL + sd;
    const int bytes = hs_trace_side_bytes(uni(S->F0), uni(S->F2), uni(S->n));
    const uint8_t* g = d.dec + uni(S->dec_off);
    if (hs_walk_in_lds(bytes)){
      const uint4* g4 = (const uint4*)g;
      for (int i = lane; i < (bytes + 15)/16; i += 64) s_dec[sd][i] = g4[i];
      decp[sd] = (const uint8_t*)s_dec[sd];
    } else decp[sd] = g;
  }
  wave_lds_sync();
  if (lane == 0) trace_walk(d, 2*q, B, max_index, decp[0]);
  else if (lane == 1) trace_walk(d, 2*q+1, B, H-1-max_index, decp[1]);
}

// ------------------------------------------------------------------ records assembled on the device (hipstr_hmm_trace_ex)
// The bookkeeping half of HapAligner::retrace (HapAligner.cpp:363-571, 642-707) and stitch_alignment_trace (AlignmentTraceback.cpp:7-52,
// 55-144) from what hs_trace_walk left in the chunk's result block: the same replay as replay_side / the stitch loop of the host path, by
// one lane per request out of LDS, then an exclusive scan per pool and a compaction into dense pools the host copies out whole.
//   hs_trace_assemble  one wavefront per request: stages the two sides' ops, the read, its SNP-eligible flags (qual_correct of the device's
//                      table against MIN_SNP_LOG_PROB_CORRECT), the flank bases (low byte of the rows) and the hap_to_ref string into LDS;
//                      lane 0 replays.  Flank and STR sequences are runs of the read in read order (the left side's pieces are reversed
//                      back, the right side walks a reversed read), so they leave as (start, length) and the compaction copies them from
//                      the read; indels, SNPs, CIGAR pairs and the alignment string go to the request's slots, every write checked.
//   hs_trace_scan      one wavefront per pool: running offsets over the chunk's requests, seeded with the earlier chunks' totals.
//   hs_trace_compact   one wavefront per request: pieces into the dense pools, a lane per element.
#define HS_ASM_LDS 8192            // bytes of staging per request the assemble kernel keeps in LDS (a 150-bp read with 60-base flanks: ~2 KB)
#define HS_ASM_POOLS 7             // hap_aln, str_seq, flank_seq (two pieces per request), indel, snp, cigar, aln_str
struct hs_areq_t {                 // one request of the assemble kernels
  int32_t loc;                     // locus: row of blk_start / blk_end
  int32_t h2r_off, h2r_len;        // its hap_to_ref string in the pool; length -1: no stitch
  int32_t indel_cap, snp_cap, fa_cap;          // entries of its slots (fa_cap: stitched string, CIGAR pairs, alignment string)
  int64_t indel_off, snp_off, fa_off;          // its slots in the staging arrays
};
struct hs_adev_t {
  const hs_areq_t* reqs;
  const int32_t *blk_start, *blk_end;          // [3*n_loci] each
  const char* h2r;
  int32_t *st_indel_pos, *st_indel_size, *st_snp_pos, *st_cig_len;      // staging, by slot
  char *st_snp_base, *st_fa, *st_cig_op, *st_aln;
  int32_t *lens, *excl, *rng, *fail;           // [8*nq] piece lengths / chunk-relative starts (pool p at hs_asm_pool_at(p, nq)), [3*nq] read offset of str_seq, flank 0, flank 2
  int64_t* totals;                             // result block from here on: [HS_ASM_POOLS] running totals, then the first failed request
  int32_t* first_fail;
  int32_t *stutter_size, *flank_ins, *flank_del, *aln_start, *aln_stop;   // [nq]
  int32_t* incl;                               // [8*nq] the caller's *_off[q+1]
  int32_t *p_indel_pos, *p_indel_size, *p_snp_pos, *p_cig_len;           // dense pools of the chunk
  char *p_hap_aln, *p_str_seq, *p_flank, *p_snp_base, *p_cig_op, *p_aln;
  int64_t base[HS_ASM_POOLS];                  // totals of the earlier chunks
  int64_t dense_cap[HS_ASM_POOLS];             // elements of each dense pool
  int32_t nq;
};
__host__ __device__ inline int hs_asm_pool_at(int p, int nq){ return (p < 3 ? p : p + 1)*nq; }      // flank_seq has 2*nq entries
__host__ __device__ inline int hs_asm_pool_n(int p, int nq){ return p == 2 ? 2*nq : nq; }
// bytes a request stages: ops of both sides | read | SNP flags | flank bases of both orientations | hap_to_ref | stitched string
__host__ __device__ inline int hs_asm_lds_bytes(int capL, int capR, int len, int F0, int F2, int hlen, int fa_cap){
  return capL + capR + 2*len + 2*(F0 + F2) + (hlen > 0 ? hlen : 0) + fa_cap;
}
__host__ __device__ inline bool hs_asm_in_lds(int bytes){ return bytes <= HS_ASM_LDS; }

__device__ __forceinline__ int wave_scan_i(int v){       // inclusive prefix sum over the wavefront: wave_sum_d's DPP steps, every lane kept
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false); v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false); v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}

constexpr double DEV_MIN_SNP_LOG_PROB_CORRECT = -0.0043648054;     // HapAligner.cpp:24

struct AsmView {                   // what the replay reads: the wavefront's LDS copies, or the originals in HBM
  const char* ops[2]; int cnt[2];
  const char* read;                // the read, forward
  const uint8_t* good;             // per base: qual_correct > MIN_SNP_LOG_PROB_CORRECT; NULL: from the tables
  const char* hc[2][2];            // flank bases per side: leading, trailing block; NULL: from the rows
  const char* h2r;
  char* fa;                        // stitched string, fa_cap bytes
};

__device__ void trace_assemble_serial(const hs_tdev_t& d, const hs_adev_t& a, int q, const AsmView& V){
  const int MATCH = 0, DEL = 1, INS = 2, NONE = -1;
  const hs_tside_t* SL = d.sides + 2*q;
  const hs_areq_t R = a.reqs[q];
  const int nq = a.nq;
  const int len = SL->len, sb = SL->seed, base_off = SL->base_off;
  const int F0 = SL->F0, F2 = SL->F2, B = d.stropts[SL->stropt].B, H = F0 + B + F2;
  const int max_index = d.max_index[q];
  bool ok = true;
  int n_indel = 0, n_snp = 0, flank_ins = 0, flank_del = 0;
  int stutter = HIPSTR_NO_STR_DATA, str_s = 0, str_n = 0;
  int fl_s[2] = {0, 0}, fl_n[2] = {0, 0};                   // flank_seq(0), flank_seq(2) as runs of the read
  auto add_flank = [&](int out_block, int s, int n){        // appends must continue the run: anything else is an inconsistent string
    const int i = out_block >> 1;
    if (n <= 0) return;
    if (fl_n[i] == 0) fl_s[i] = s; else if (fl_s[i] + fl_n[i] != s) ok = false;
    fl_n[i] += n;
  };
  auto push_indel = [&](int32_t pos, int32_t size){
    if (n_indel < R.indel_cap){ a.st_indel_pos[R.indel_off + n_indel] = pos; a.st_indel_size[R.indel_off + n_indel] = size; } else ok = false;
    n_indel++;
  };
  auto push_snp = [&](int32_t pos, char c){
    if (n_snp < R.snp_cap){ a.st_snp_pos[R.snp_off + n_snp] = pos; a.st_snp_base[R.snp_off + n_snp] = c; } else ok = false;
    n_snp++;
  };
  const int blen3[3] = { F0, B, F2 };
  int seed_block = 0;
  for (int x = 0, crd = max_index; x < 3; x++){ if (crd < blen3[x]){ seed_block = x; break; } crd -= blen3[x]; }
  // left retrace, then the seed base joins the flank it sits in, then the right retrace (HapAligner.cpp:642-684)
  for (int sd = 0; sd < 2 && ok; sd++){
    const hs_tside_t* S = SL + sd;
    const bool rev = sd != 0;
    const int cnt = V.cnt[sd];
    if (cnt < 0 || cnt > S->ops_cap){ ok = false; break; }
    if (sd == 1 && seed_block != 1) add_flank(seed_block, sb, 1);
    const int mx = sd ? H-1-max_index : max_index;
    if (mx == 0) continue;                                  // this side is all soft clips
    const int n = S->n;
    const int sblen[3] = { S->F0, B, S->F2 };
    int blk = 0, crd = mx;
    for (int x = 0; x < 3; x++){ if (crd < sblen[x]){ blk = x; break; } crd -= sblen[x]; }
    int block, base;
    if (crd == 0){ block = blk-1; base = block >= 0 ? sblen[block]-1 : -1; } else { block = blk; base = crd-1; }
    const int size = d.str_size[2*q+sd], apos = d.str_pos[2*q+sd];
    const char* ops = V.ops[sd];
    auto rdc = [&](int x){ return V.read[rev ? len-1-x : x]; };             // the side's read (reversed for the right problem)
    int seq = n-1, k = 0;
    bool done = false;
    while (block >= 0 && ok && !done){
      const int blen = sblen[block];
      if (block == 1){
        int i = max(0, min(seq+1, apos));
        k += i;
        if (size < 0) k += -size;
        else { const int e = min(seq+1, apos+size); if (e > i){ k += e-i; i = e; } }
        { const int e = min(blen+size, seq+1); if (e > i){ k += e-i; i = e; } }
        stutter = size; str_n = i; str_s = rev ? len-1-seq : seq-i+1;       // rd[seq], rd[seq-1], ..: a run of the read either way
        if (blen + size >= seq+1){ done = true; break; }                   // the read does not span the STR block
        seq -= blen + size;
      } else {
        int prev = NONE;
        const int fb = rev ? 2-block : block;                               // side_block_start
        int32_t pos = ((!rev || fb == 1) ? a.blk_start[3*R.loc + fb] : a.blk_end[3*R.loc + fb]-1) + (rev ? -base : base);
        const int32_t inc = rev ? 1 : -1;
        int indel_seq = -1; int32_t indel_position = -1;
        const int seq_hi = seq;
        const int which = block == 0 ? 0 : 1;
        const hs_row_t* rows = d.rows + (block == 0 ? S->lead_off : S->trail_off);
        auto flush = [&](){ add_flank(fb, rev ? len-1-seq_hi : seq+1, seq_hi - seq); };
        while (base >= 0 && seq >= 0){
          if (k >= cnt){ ok = false; break; }
          const char oc = ops[k++];
          const int type = oc == 'M' ? MATCH : (oc == 'D' ? DEL : (oc == 'I' ? INS : NONE));
          if (type == NONE){ ok = false; break; }
          if (type != prev){
            if (prev == DEL){
              if (rev) push_indel(indel_position, indel_position - pos);
              else     push_indel(pos+1, pos - indel_position);
            } else if (prev == INS)
              push_indel(indel_position + (rev ? 0 : 1), (int32_t)(indel_seq - seq));
            if (type == DEL || type == INS){ indel_seq = seq; indel_position = pos; }
            prev = type;
          }
          if (type == MATCH){
            const char rc = rdc(seq);
            const char hcv = V.hc[sd][which] ? V.hc[sd][which][base] : (char)(rows[base] & 0xff);
            if (hcv != rc){
              const int ri = rev ? len-1-seq : seq;
              const bool good = V.good ? V.good[ri] != 0 : d.qual_correct[(uint8_t)d.quals[base_off + ri]] > DEV_MIN_SNP_LOG_PROB_CORRECT;
              if (good) push_snp(pos, rc);
            }
            seq--; base--; pos += inc;
          } else if (type == DEL){ flank_del++; base--; pos += inc; }
          else { flank_ins++; seq--; }
          if (seq == -1 || (base == -1 && block == 0)){
            k += seq + 1;                      // soft clips
            done = true;
            break;
          }
        }
        if (ok) flush();
      }
      if (done) break;
      block--;
      if (block >= 0) base = sblen[block] - 1;
    }
    if (k != cnt) ok = false;
  }
  const int cntL = V.cnt[0], cntR = V.cnt[1];
  const int nfull = cntL + 1 + cntR;                        // hap_aln = reversed left ops + 'M' + right ops
  int n_cig = 0, n_aln = 0;
  int32_t start = 0, stop = 0;
  if (ok && R.h2r_len >= 0){
    // ---- stitch_alignment_trace (AlignmentTraceback.cpp:55-144)
    const char* h2r = V.h2r; const int hlen = R.h2r_len;
    auto fullc = [&](int i){ return i < cntL ? V.ops[0][cntL-1-i] : (i == cntL ? 'M' : V.ops[1][i-cntL-1]); };
    int hap_index = max_index, hai = 0; int32_t seed_pos = a.blk_start[3*R.loc];
    while (hap_index > 0 && hai < hlen){
      const char c = h2r[hai];
      if (c == 'M' || c == 'I') hap_index--;
      if (c == 'M' || c == 'D') seed_pos++;
      hai++;
    }
    while (hai < hlen && h2r[hai] == 'D') hai++;
    int sbase = sb, rai = 0;
    while (sbase > 0 && rai < nfull){
      const char c = fullc(rai);
      if (c == 'M' || c == 'I' || c == 'S') sbase--;
      rai++;
    }
    while (rai < nfull && fullc(rai) == 'D') rai++;
    // every character stitch_dir emits spends a read base or a hap_to_ref character: the left part is at most sb + hai long and is written
    // backwards from there, which is the reversal the reference does afterwards
    const int mid = sb + hai;
    auto stitch_dir = [&](int h_index, int r_index, int inc, int wpos){      // AlignmentTraceback.cpp:7-52
      int w = 0;
      while (r_index >= 0 && r_index < nfull){
        const char rc = fullc(r_index);
        char out = 0;
        if (rc == 'S'){ out = 'S'; r_index += inc; }
        else {
          if (h_index < 0 || h_index >= hlen) break;
          const char hcv = h2r[h_index];
          if (hcv == 'D'){
            if (rc == 'I'){ out = 'M'; r_index += inc; h_index += inc; }
            else { out = 'D'; h_index += inc; }
          }
          else if (rc == 'I'){ out = 'I'; r_index += inc; }
          else if (rc == 'D'){
            if (hcv == 'M') out = 'D';
            r_index += inc; h_index += inc;
          }
          else { out = hcv; r_index += inc; h_index += inc; }
        }
        if (out){
          const int p = wpos + inc*w;
          if (p >= 0 && p < R.fa_cap) V.fa[p] = out; else ok = false;
          w++;
        }
      }
      return w;
    };
    const int nla = stitch_dir(hai-1, rai-1, -1, mid-1);
    const int nra = stitch_dir(hai+1, rai+1, 1, mid+1);
    if (mid < R.fa_cap) V.fa[mid] = 'M'; else ok = false;
    if (ok){
      const char* fa = V.fa + (mid - nla);
      const int nfa = nla + 1 + nra;
      start = stop = seed_pos;
      bool lead = true; char cc = 0; int num = 0, ri = 0;
      auto push_cig = [&](char c, int32_t m){
        if (n_cig < R.fa_cap){ a.st_cig_op[R.fa_off + n_cig] = c; a.st_cig_len[R.fa_off + n_cig] = m; } else ok = false;
        n_cig++;
      };
      auto push_aln = [&](char c){ if (n_aln < R.fa_cap) a.st_aln[R.fa_off + n_aln] = c; else ok = false; n_aln++; };
      for (int i = 0; i < nfa; i++){
        char ch = fa[i];
        if (lead){ if (ch == 'I') ch = 'S'; else lead = false; }          // leading 'I' -> 'S'
        if (ch == 'D' || ch == 'M'){ if (i < nla) start--; else if (i > nla) stop++; }
        if (i == 0){ cc = ch; num = 1; }
        else if (ch != cc){ push_cig(cc, num); cc = ch; num = 1; }
        else num++;
        if (ch == 'S') ri++;
        else if (ch == 'M' || ch == 'I'){ if (ri < len) push_aln(V.read[ri]); else ok = false; ri++; }
        else push_aln('-');
      }
      push_cig(cc, num);
    }
  }
  if (str_s < 0 || str_s + str_n > len) ok = false;
  for (int i = 0; i < 2; i++) if (fl_s[i] < 0 || fl_s[i] + fl_n[i] > len) ok = false;
  if (!ok){ n_indel = n_snp = n_cig = n_aln = str_n = fl_n[0] = fl_n[1] = 0; }
  a.fail[q] = ok ? 0 : 1;
  a.lens[hs_asm_pool_at(0, nq) + q] = ok ? nfull : 0;
  a.lens[hs_asm_pool_at(1, nq) + q] = str_n;
  a.lens[hs_asm_pool_at(2, nq) + 2*q] = fl_n[0]; a.lens[hs_asm_pool_at(2, nq) + 2*q+1] = fl_n[1];
  a.lens[hs_asm_pool_at(3, nq) + q] = n_indel;
  a.lens[hs_asm_pool_at(4, nq) + q] = n_snp;
  a.lens[hs_asm_pool_at(5, nq) + q] = n_cig;
  a.lens[hs_asm_pool_at(6, nq) + q] = n_aln;
  a.rng[q] = str_s; a.rng[nq + q] = fl_s[0]; a.rng[2*nq + q] = fl_s[1];
  a.stutter_size[q] = stutter; a.flank_ins[q] = flank_ins; a.flank_del[q] = flank_del;
  a.aln_start[q] = start; a.aln_stop[q] = stop;
}

__global__ void __launch_bounds__(64) hs_trace_assemble(const hs_tdev_t* __restrict__ dp, hs_adev_t a){
  const hs_tdev_t& d = *dp;
  const int lane = threadIdx.x;
  const int q = blockIdx.x;
  const hs_tside_t* SL = d.sides + 2*q;
  const hs_areq_t* R = a.reqs + q;
  const int len = uni(SL->len), base_off = uni(SL->base_off), hlen = uni(R->h2r_len), fa_cap = uni(R->fa_cap);
  __shared__ char s_buf[HS_ASM_LDS];
  AsmView V;
  V.cnt[0] = uni(d.n_ops[2*q]); V.cnt[1] = uni(d.n_ops[2*q+1]);
  if (hs_asm_in_lds(hs_asm_lds_bytes(uni(SL->ops_cap), uni(SL[1].ops_cap), len, uni(SL->F0), uni(SL->F2), hlen, fa_cap))){
    // (pieces in hs_asm_lds_bytes' order, so they end inside s_buf; every copy is clamped to its piece)
    int at = 0;
    for (int sd = 0; sd < 2; sd++){
      const hs_tside_t* S = SL + sd;
      const int cap = uni(S->ops_cap), m = min(max(V.cnt[sd], 0), cap);
      const char* g = d.ops + uni(S->ops_off);
      for (int i = lane; i < m; i += 64) s_buf[at + i] = g[i];
      V.ops[sd] = s_buf + at; at += cap;
    }
    for (int i = lane; i < len; i += 64){
      s_buf[at + i] = d.bases[base_off + i];
      s_buf[at + len + i] = d.qual_correct[(uint8_t)d.quals[base_off + i]] > DEV_MIN_SNP_LOG_PROB_CORRECT ? 1 : 0;
    }
    V.read = s_buf + at; V.good = (const uint8_t*)(s_buf + at + len); at += 2*len;
    for (int sd = 0; sd < 2; sd++){
      const hs_tside_t* S = SL + sd;
      const int f0 = uni(S->F0), f2 = uni(S->F2);
      const hs_row_t* lead = d.rows + uni(S->lead_off); const hs_row_t* trail = d.rows + uni(S->trail_off);
      for (int i = lane; i < f0; i += 64) s_buf[at + i] = (char)(lead[i] & 0xff);
      for (int i = lane; i < f2; i += 64) s_buf[at + f0 + i] = (char)(trail[i] & 0xff);
      V.hc[sd][0] = s_buf + at; V.hc[sd][1] = s_buf + at + f0; at += f0 + f2;
    }
    if (hlen > 0){
      const char* g = a.h2r + uni(R->h2r_off);
      for (int i = lane; i < hlen; i += 64) s_buf[at + i] = g[i];
    }
    V.h2r = s_buf + at; at += max(hlen, 0);
    V.fa = s_buf + at;
  } else {
    V.ops[0] = d.ops + uni(SL->ops_off); V.ops[1] = d.ops + uni(SL[1].ops_off);
    V.read = d.bases + base_off; V.good = NULL;
    V.hc[0][0] = V.hc[0][1] = V.hc[1][0] = V.hc[1][1] = NULL;
    V.h2r = a.h2r + uni(R->h2r_off);
    V.fa = a.st_fa + uni(R->fa_off);
  }
  wave_lds_sync();
  if (lane == 0) trace_assemble_serial(d, a, q, V);
}

// running offsets of one pool per wavefront; wavefront HS_ASM_POOLS finds the first failed request
__global__ void __launch_bounds__(64) hs_trace_scan(hs_adev_t a){
  const int lane = threadIdx.x, p = blockIdx.x, nq = a.nq;
  if (p == HS_ASM_POOLS){
    int first = 0x7fffffff;
    for (int i0 = 0; i0 < nq; i0 += 64){
      const int i = i0 + lane;
      first = min(first, wave_min_i((i < nq && a.fail[i]) ? i : 0x7fffffff));
    }
    if (lane == 0) *a.first_fail = first == 0x7fffffff ? -1 : first;
    return;
  }
  const int n = hs_asm_pool_n(p, nq);
  const int32_t* lens = a.lens + hs_asm_pool_at(p, nq);
  int32_t* excl = a.excl + hs_asm_pool_at(p, nq);
  int32_t* incl = a.incl + hs_asm_pool_at(p, nq);
  int64_t carry = 0;                                        // chunk-relative
  for (int i0 = 0; i0 < n; i0 += 64){
    const int i = i0 + lane;
    const int v = i < n ? lens[i] : 0;
    const int s = wave_scan_i(v);
    if (i < n){ excl[i] = (int32_t)(carry + s - v); incl[i] = (int32_t)(a.base[p] + carry + s); }
    carry += rdlane(s, 63);
  }
  if (lane == 0) a.totals[p] = a.base[p] + carry;
}

__global__ void __launch_bounds__(64) hs_trace_compact(const hs_tdev_t* __restrict__ dp, hs_adev_t a){
  const hs_tdev_t& d = *dp;
  const int lane = threadIdx.x, q = blockIdx.x, nq = a.nq;
  if (uni(a.fail[q])) return;
  const hs_tside_t* SL = d.sides + 2*q;
  const hs_areq_t* R = a.reqs + q;
  auto len_of = [&](int p, int i){ return uni(a.lens[hs_asm_pool_at(p, nq) + i]); };
  auto at_of = [&](int p, int i){ return (int64_t)uni(a.excl[hs_asm_pool_at(p, nq) + i]); };
  // a piece that would end past its dense pool is dropped whole (cannot happen: a piece is at most its slot, the pools are the slots' sum)
  auto fits = [&](int p, int64_t at, int n){ return at >= 0 && at + n <= a.dense_cap[p]; };
  {
    const int cntL = uni(d.n_ops[2*q]), n = len_of(0, q); const int64_t at = at_of(0, q);
    const char* oL = d.ops + uni(SL->ops_off); const char* oR = d.ops + uni(SL[1].ops_off);
    if (fits(0, at, n)) for (int i = lane; i < n; i += 64) a.p_hap_aln[at + i] = i < cntL ? oL[cntL-1-i] : (i == cntL ? 'M' : oR[i-cntL-1]);
  }
  const char* read = d.bases + uni(SL->base_off);
  {
    const int n = len_of(1, q), s = uni(a.rng[q]); const int64_t at = at_of(1, q);
    if (fits(1, at, n)) for (int i = lane; i < n; i += 64) a.p_str_seq[at + i] = read[s + i];
  }
  for (int f = 0; f < 2; f++){
    const int n = len_of(2, 2*q+f), s = uni(a.rng[(1+f)*nq + q]); const int64_t at = at_of(2, 2*q+f);
    if (fits(2, at, n)) for (int i = lane; i < n; i += 64) a.p_flank[at + i] = read[s + i];
  }
  {
    const int n = len_of(3, q); const int64_t at = at_of(3, q), from = uni(R->indel_off);
    if (fits(3, at, n)) for (int i = lane; i < n; i += 64){ a.p_indel_pos[at + i] = a.st_indel_pos[from + i]; a.p_indel_size[at + i] = a.st_indel_size[from + i]; }
  }
  {
    const int n = len_of(4, q); const int64_t at = at_of(4, q), from = uni(R->snp_off);
    if (fits(4, at, n)) for (int i = lane; i < n; i += 64){ a.p_snp_pos[at + i] = a.st_snp_pos[from + i]; a.p_snp_base[at + i] = a.st_snp_base[from + i]; }
  }
  {
    const int n = len_of(5, q); const int64_t at = at_of(5, q), from = uni(R->fa_off);
    if (fits(5, at, n)) for (int i = lane; i < n; i += 64){ a.p_cig_op[at + i] = a.st_cig_op[from + i]; a.p_cig_len[at + i] = a.st_cig_len[from + i]; }
  }
  {
    const int n = len_of(6, q); const int64_t at = at_of(6, q), from = uni(R->fa_off);
    if (fits(6, at, n)) for (int i = lane; i < n; i += 64) a.p_aln[at + i] = a.st_aln[from + i];
  }
}

// ------------------------------------------------------------------ host side

// ---- launch decisions: the one place each is taken.  hipstr_hmm_trace_seeded calls them, hipstr_debug_trace_plan reports them
// (tests/test_stage_routes.py pins a case on each side of every limit)
#define HS_TRACE_STATIC_CLASSES 6        // column classes whose tables are static LDS (hs_trace_fill<1..6>, hs_trace_fill_mixed)
#define HS_TRACE_MIXED_MAX_REQ 4096      // a chunk of more requests launches the static classes one by one
#define HS_TRACE_BUDGET_MIB 256          // decision bytes per chunk unless the call could need more (then the device is asked) or HIPSTR_TRACE_WS_MIB says
int trace_col_class(int n){ return (n + 63)/64; }                           // columns per lane of a side of n columns: 1 .. HS_MAX_COLS
// the fill kernel of a class: hs_trace_fill<cl> up to HS_TRACE_STATIC_CLASSES, then hs_trace_fill_long<8 | 12 | 16>
int trace_fill_cols(int cl){ return cl <= HS_TRACE_STATIC_CLASSES ? cl : (cl <= 8 ? 8 : (cl <= 12 ? 12 : 16)); }
// small call, several static classes: one launch (hs_trace_fill_mixed)
bool trace_mixed_launch(int n_static_classes, int nq){ return n_static_classes > 1 && nq <= HS_TRACE_MIXED_MAX_REQ; }
// only the requested reads' bases travel when they are less than half of the batch's
bool trace_compact_reads(int64_t wanted, int64_t total_bases){ return wanted > 0 && wanted*2 < total_bases; }
const char* trace_side_refusal(int s, int len){
  return (s > 64*HS_MAX_COLS || len-s-1 > 64*HS_MAX_COLS) ? "traceback of a read side longer than 1024 bases is not supported" : NULL;
}
static_assert(64*HS_MAX_COLS == 1024, "the refusal message names the limit");
// workspace bytes of a side (16-byte pieces: hs_trace_walk copies a matrix to LDS in uint4s) and of a request
int64_t trace_side_ws(int F0, int F2, int n){ return ((int64_t)(F0 + 1 + F2)*n + 15) & ~(int64_t)15; }
bool trace_asks_device(int64_t rough_bytes){ return rough_bytes > ((int64_t)HS_TRACE_BUDGET_MIB << 20); }
int64_t trace_env_budget(int64_t budget){
  if (const char* e = getenv("HIPSTR_TRACE_WS_MIB")) budget = std::max<int64_t>(1, atoll(e)) << 20;
  return budget;
}
// the chunk that starts at request q0: requests while their matrices fit the budget
int trace_chunk_end(const std::vector<int64_t>& need, int q0, int64_t budget){
  int q1 = q0; int64_t mat = 0;
  while (q1 < (int)need.size() && mat + need[q1] <= budget){ mat += need[q1]; q1++; }
  return q1;
}
// operation characters a side can emit: its read columns, the haplotype's rows and the largest artifact
int trace_ops_cap(int n, int F0, int F2, int B, int period){ return n + F0 + F2 + B + 2*HS_MAXREP*period + 16; }
// slots of a device-assembled request (hipstr_hmm_trace_ex), from bounds alone.  hap_aln: both sides' ops and the seed's 'M'.  seq: str_seq
// and each flank_seq piece are runs of the read.  snp: one per read base at most.  indel: a record closes a run of 'I' or 'D'; in a flank
// block runs alternate, every run that is not 'D' spends a read base, and a side walks two flank blocks, so there are at most len + 2 + 2
// deletion runs and len insertion runs.  stitched (the stitched string, its CIGAR pairs and the alignment string): every character
// stitch_dir emits spends a read base or a hap_to_ref character; 0 without hap_to_ref (hlen < 0).
struct TraceAsmCaps { int hap_aln, seq, indel, snp, stitched, lds_bytes; };
TraceAsmCaps trace_asm_caps(int capL, int capR, int len, int F0, int F2, int hlen){
  TraceAsmCaps c;
  c.hap_aln = capL + capR + 1; c.seq = len; c.indel = 2*len + 4; c.snp = len; c.stitched = hlen < 0 ? 0 : len + hlen;
  c.lds_bytes = hs_asm_lds_bytes(capL, capR, len, F0, F2, hlen, c.stitched);
  return c;
}
// the seed of a request: the caller's or the host's; NULL or the refusal
const char* trace_seed_of(const hipstr_batch_t* b, int l, int r, const int32_t* req_seed, int q, int& s){
  const bool given = req_seed && req_seed[q] != HIPSTR_SEED_AUTO;       // trace_optimal_aln's seed_base argument (HapAligner.h:93)
  s = given ? req_seed[q] : hipstr::calc_seed_base(b, l, r);
  if (s == -2) return "Invalid alignment seed or unrecognized CIGAR char (HapAligner.cpp:309,316)";
  if (s < 0) return "read without a seed base cannot be traced (HapAligner.cpp:586-594)";
  const int len = b->base_off[r+1] - b->base_off[r];
  if (given && (s < 1 || s > len - 2)) return "seed base must leave at least one base on either side (HapAligner.cpp:316)";
  return trace_side_refusal(s, len);
}

// two side streams + their events per (host thread, device), created at first use and kept
struct AllelePrep {
  std::string seq[2][3];          // block sequences per orientation, in side order
  int lead_off[2], trail_off[2], stropt[2];
  int32_t h2r_off = 0, h2r_len = -1;      // its hap_to_ref string in the pool a device-assembled call uploads
};

struct TraceAcc {                 // what AlignmentTrace accumulates (AlignmentTraceback.h:27-34)
  bool str_set = false; int stutter_size = 0; std::string str_seq;
  std::string flank[3];
  int flank_ins = 0, flank_del = 0;
  std::vector<std::pair<int32_t,int32_t>> indels;
  std::vector<std::pair<int32_t,char>> snps;
};

// start coordinate a (possibly reversed) haplotype block reports: HapBlock::reverse() builds HapBlock(end_-1, start_-1, ..),
// RepeatBlock::reverse() keeps (start_, end_) (HapBlock.h:123-133, RepeatBlock.h:48-58)
int32_t side_block_start(const hipstr_batch_t* b, int locus, bool rev, int bi){
  const int fb = rev ? 2-bi : bi;
  if (!rev || fb == 1) return b->blk_start[3*locus + fb];
  return b->blk_end[3*locus + fb]-1;
}

const double MIN_SNP_LOG_PROB_CORRECT = -0.0043648054;     // HapAligner.cpp:24

// The matrix-free half of HapAligner::retrace (HapAligner.cpp:363-571): the device decided the move at every step
// (`ops`); this replays them to collect flank sequences, SNPs, indels and the STR sequence.  rd/lc: the side's read
// (reversed for the right problem).  Returns false if the operation string is inconsistent.
bool replay_side(const hipstr_batch_t* b, int locus, const std::string sseq[3], bool rev, const std::string& rd, const std::vector<double>& lc,
                 const std::string& ops, int size, int apos, int block, int base, TraceAcc& tr){
  const int MATCH = 0, DEL = 1, INS = 2, NONE = -1;
  const int n = rd.size();
  int seq = n-1;
  size_t k = 0;
  while (block >= 0){
    const std::string& bs = sseq[block];
    const int blen = bs.size();
    if (block == 1){
      std::string ss;
      int i = 0;
      for (; i < std::min(seq+1, apos); i++){ ss.push_back(rd[seq-i]); k++; }
      if (size < 0) k += -size;
      else for (; i < std::min(seq+1, apos+size); i++){ ss.push_back(rd[seq-i]); k++; }
      for (; i < std::min(blen+size, seq+1); i++){ ss.push_back(rd[seq-i]); k++; }
      if (!rev) std::reverse(ss.begin(), ss.end());
      tr.str_set = true; tr.stutter_size = size; tr.str_seq = ss;
      if (blen + size >= seq+1) return k == ops.size();
      seq -= blen + size;
    } else {
      int prev = NONE;
      int32_t pos = side_block_start(b, locus, rev, block) + (rev ? -base : base);
      const int32_t inc = rev ? 1 : -1;
      int indel_seq = -1; int32_t indel_position = -1;
      std::string fs;
      const int out_block = rev ? 2-block : block;
      auto flush = [&](){ if (!rev) std::reverse(fs.begin(), fs.end()); tr.flank[out_block] += fs; };
      while (base >= 0 && seq >= 0){
        if (k >= ops.size()) return false;
        const char oc = ops[k++];
        const int type = oc == 'M' ? MATCH : (oc == 'D' ? DEL : (oc == 'I' ? INS : NONE));
        if (type == NONE) return false;
        if (type != prev){
          if (prev == DEL){
            if (rev) tr.indels.push_back(std::make_pair(indel_position, indel_position - pos));
            else     tr.indels.push_back(std::make_pair(pos+1, pos - indel_position));
          } else if (prev == INS)
            tr.indels.push_back(std::make_pair(indel_position + (rev ? 0 : 1), (int32_t)(indel_seq - seq)));
          if (type == DEL || type == INS){ indel_seq = seq; indel_position = pos; }
          prev = type;
        }
        if (type == MATCH){
          if (bs[base] != rd[seq] && lc[seq] > MIN_SNP_LOG_PROB_CORRECT) tr.snps.push_back(std::make_pair(pos, rd[seq]));
          fs.push_back(rd[seq]); seq--; base--; pos += inc;
        } else if (type == DEL){ tr.flank_del++; base--; pos += inc; }
        else { tr.flank_ins++; fs.push_back(rd[seq]); seq--; }
        if (seq == -1 || (base == -1 && block == 0)){
          k += seq + 1;                        // soft clips
          flush();
          return k == ops.size();
        }
      }
      flush();
    }
    block--;
    if (block >= 0) base = (int)sseq[block].size() - 1;
  }
  return k == ops.size();
}

// AlignmentTraceback.cpp:7-52
void stitch_dir(const char* hap_aln, int hlen, const std::string& read_aln, int h_index, int r_index, int inc, std::string& out){
  const int rlen = read_aln.size();
  while (r_index >= 0 && r_index < rlen){
    if (read_aln[r_index] == 'S'){ out.push_back('S'); r_index += inc; continue; }
    if (h_index < 0 || h_index >= hlen) return;
    if (hap_aln[h_index] == 'D'){
      if (read_aln[r_index] == 'I'){ out.push_back('M'); r_index += inc; h_index += inc; }
      else { out.push_back('D'); h_index += inc; }
    }
    else if (read_aln[r_index] == 'I'){ out.push_back('I'); r_index += inc; }
    else if (read_aln[r_index] == 'D'){
      if (hap_aln[h_index] == 'M') out.push_back('D');
      r_index += inc; h_index += inc;
    }
    else { out.push_back(hap_aln[h_index]); r_index += inc; h_index += inc; }
  }
}

struct ReqOut {                    // one request's results, built by a worker thread, copied into the flat pools in order
  bool ok = true;
  std::string hap_aln, aln_str;
  TraceAcc acc;
  int32_t aln_start = 0, aln_stop = 0;
  std::vector<std::pair<char,int32_t>> cigar;
};

// ---- the resident result (api_internal.h: hipstr_trace_dev): where every array lies in the handle's one block.  A chunk's segment has the
// same layout for the chunk's requests and elements, so the segment of a call of one chunk IS the result.
const int TD_ARR_POOL[HS_TRACE_DEV_ARRAYS] = HS_TRACE_DEV_ARR_POOL_LIST;
const int TD_ARR_ESZ[HS_TRACE_DEV_ARRAYS]  = HS_TRACE_DEV_ARR_ESZ_LIST;
// the fetch group (HIPSTR_TRACE_F_*) of every pool
const uint32_t TD_POOL_BIT[HS_TRACE_DEV_POOLS] = { HIPSTR_TRACE_F_HAP_ALN, HIPSTR_TRACE_F_STR_SEQ, HIPSTR_TRACE_F_FLANKS, HIPSTR_TRACE_F_INDELS, HIPSTR_TRACE_F_SNPS,
                                                   HIPSTR_TRACE_F_STITCH, HIPSTR_TRACE_F_STITCH };
static_assert(HS_TRACE_DEV_POOLS == HS_ASM_POOLS, "a resident pool per assembled pool");
struct TraceDevLayout {
  size_t ll, mxi, scal[5], off[HS_TRACE_DEV_POOLS], arr[HS_TRACE_DEV_ARRAYS], bytes;
  TraceDevLayout(size_t n, const int64_t tot[HS_TRACE_DEV_POOLS]){
    hipstr::BlockPieces P;
    ll = P.take(n*8); mxi = P.take(n*4);
    for (int i = 0; i < 5; i++) scal[i] = P.take(n*4);
    for (int p = 0; p < HS_TRACE_DEV_POOLS; p++) off[p] = P.take(((size_t)hs_asm_pool_n(p, (int)n) + 1)*4);
    for (int a = 0; a < HS_TRACE_DEV_ARRAYS; a++) arr[a] = P.take((size_t)tot[TD_ARR_POOL[a]]*TD_ARR_ESZ[a]);
    bytes = P.tot;
  }
};
// a handle of n requests and these totals on a fresh block of the context's cache; NULL + last error
hipstr_trace_dev* trace_dev_new(hipstr::Ctx* ctx, hipStream_t st, int32_t n, const int64_t tot[HS_TRACE_DEV_POOLS]){
  const TraceDevLayout L((size_t)n, tot);
  char* blk = (char*)hipstr::dev_alloc(ctx, L.bytes);
  if (!blk) return NULL;
  hipstr_trace_dev* td = new hipstr_trace_dev();
  td->ctx = ctx; td->stream = st; td->n_req = n; td->block = blk;
  for (int p = 0; p < HS_TRACE_DEV_POOLS; p++){ td->totals[p] = tot[p]; td->off[p] = (int32_t*)(blk + L.off[p]); }
  td->ll = (double*)(blk + L.ll); td->max_index = (int32_t*)(blk + L.mxi);
  for (int i = 0; i < 5; i++) td->scal[i] = (int32_t*)(blk + L.scal[i]);
  for (int a = 0; a < HS_TRACE_DEV_ARRAYS; a++) td->arr[a] = blk + L.arr[a];
  return td;
}
void trace_dev_drop(hipstr_trace_dev* td){ if (td){ if (td->block) hipstr::dev_free(td->ctx, td->block); delete td; } }
// the segments of a call's chunks: given back when the call leaves, after everything it queued on them has run
struct TraceSegs {
  std::vector<hipstr_trace_dev*> v; std::vector<int> q0; hipStream_t st = NULL;
  ~TraceSegs(){ if (!v.empty()) hipStreamSynchronize(st); for (hipstr_trace_dev* s : v) trace_dev_drop(s); }
};

// Device arrays home: one copy per array into its place of a pinned block, one wait, then onto the caller's pages.  What the device-assembled
// call does with a chunk's pools and hipstr_trace_dev_fetch with the chosen arrays.
struct HomePiece { const void* dev; size_t bytes; void* dst; size_t pin_off; };
int copy_home(hipStream_t st, char* pin, const std::vector<HomePiece>& v){
  for (const HomePiece& h : v) if (h.bytes) HS_HIP(hipMemcpyAsync(pin + h.pin_off, h.dev, h.bytes, hipMemcpyDeviceToHost, st));
  HS_HIP(hipstr::wait_stream(st));
  for (const HomePiece& h : v) if (h.bytes) memcpy(h.dst, pin + h.pin_off, h.bytes);
  return 0;
}

// ---- the guards of the entry points below: a block or a handle goes back on every way out, after the stream that may still work on it
// (ResultBlocks' rule, api_internal.h: on the normal path the stream has been waited for already and the wait costs a few microseconds)
struct PinBlock {
  hipstr::Ctx* ctx; hipStream_t st; char* p;
  PinBlock(hipstr::Ctx* c, hipStream_t s, size_t bytes) : ctx(c), st(s), p((char*)hipstr::pin_alloc(c, bytes)) {}
  PinBlock(const PinBlock&) = delete;
  ~PinBlock(){ if (p){ hipStreamSynchronize(st); hipstr::pin_free(ctx, p); } }
};
struct TraceDevGuard {             // a handle under construction: release() hands it to the caller
  hipstr_trace_dev* t; hipStream_t st;
  ~TraceDevGuard(){ if (t){ hipStreamSynchronize(st); trace_dev_drop(t); } }
  hipstr_trace_dev* release(){ hipstr_trace_dev* r = t; t = NULL; return r; }
};
hipError_t d2d(hipStream_t st, void* dst, const void* src, size_t nb){ return nb ? hipMemcpyAsync(dst, src, nb, hipMemcpyDeviceToDevice, st) : hipSuccess; }

// ---- the arrays of a hipstr_trace_out_t, enumerated once: scalars, offsets in pool order, arrays in TD_ARR_POOL's order.  (The struct is
// all pointers, so a const one serves as a source as well.)
struct TraceOutView {
  double* ll; int32_t* max_index;
  int32_t* scal[5]; int32_t* off[HS_TRACE_DEV_POOLS]; void* arr[HS_TRACE_DEV_ARRAYS];
  explicit TraceOutView(const hipstr_trace_out_t* t)
    : ll(t->ll), max_index(t->max_index), scal{t->stutter_size, t->flank_ins, t->flank_del, t->aln_start, t->aln_stop},
      off{t->hap_aln_off, t->str_seq_off, t->flank_seq_off, t->indel_off, t->snp_off, t->cigar_off, t->aln_str_off},
      arr{t->hap_aln, t->str_seq, t->flank_seq, t->indel_pos, t->indel_size, t->snp_pos, t->snp_base, t->cigar_op, t->cigar_len, t->aln_str} {}
};
// the dense pools of a device-assembled chunk, in the same order
struct AsmDense { const char* p[HS_TRACE_DEV_ARRAYS]; };
AsmDense asm_dense(const hs_adev_t& a){
  return AsmDense{{a.p_hap_aln, a.p_str_seq, a.p_flank, (const char*)a.p_indel_pos, (const char*)a.p_indel_size, (const char*)a.p_snp_pos, a.p_snp_base,
                   a.p_cig_op, (const char*)a.p_cig_len, a.p_aln}};
}

// ---- what a request list means: the one walk, for the call and for both plans.  It makes every refusal that depends on the batch and the
// list alone, in this order: per locus the period, then blocks without options; per request the read, the allele, the seed (trace_seed_of),
// and for a (locus, allele) pair not seen before its locus' stutter model (stutter_model.h:35-39), its blocks in order, then the flanks' total.
struct TracePair { int32_t locus, allele, opt[3], len[3]; };      // a distinct pair: the option (counted over the batch) and the bases of each block
struct TraceRequests {
  std::vector<int32_t> locus, seed, len, pair, compact_off;       // per request; compact_off: its read among the requested reads, first come first
  std::vector<TracePair> pairs;
  std::vector<int64_t> need;       // workspace bytes of a request: trace_side_ws of both sides
  int64_t rough = 0;               // bound of the call's decision bytes: what trace_asks_device judges
  int64_t wanted = 0;              // bases of the distinct reads requested: what trace_compact_reads judges
  int cols(int q, int sd) const { return sd ? len[q] - seed[q] - 1 : seed[q]; }       // read columns of a side
  int rows(int q, int sd, int x) const { return pairs[pair[q]].len[sd ? 2-x : x]; }   // bases of block x in the side's orientation
};
const char* trace_resolve(const hipstr_batch_t* b, int32_t n_req, const int32_t* req_read, const int32_t* req_allele, const int32_t* req_seed, TraceRequests& R){
  const int n_loci = b->n_loci, n_reads = b->read_off[n_loci];
  std::vector<int32_t> opt_base(n_loci + 1, 0);           // first option (over all blocks) of every locus
  for (int l = 0; l < n_loci; l++){
    if (b->period[l] < 1 || b->period[l] > 9) return "STR period must be in [1,9] (stutter_model.h:38)";
    int cnt = 0;
    for (int k = 0; k < 3; k++){
      if (b->blk_nopts[3*l+k] < 1) return "haplotype block without options";
      cnt += b->blk_nopts[3*l+k];
    }
    opt_base[l+1] = opt_base[l] + cnt;
  }
  R.locus.resize(n_req); R.seed.resize(n_req); R.len.resize(n_req); R.pair.resize(n_req); R.compact_off.resize(n_req); R.need.resize(n_req);
  std::map<int64_t, int> slot;                           // (locus, allele) -> entry of `pairs`
  std::vector<int32_t> at(n_req ? (size_t)n_reads : 0, -1);      // read -> offset among the requested reads
  for (int q = 0; q < n_req; q++){
    const int r = req_read[q], k = req_allele[q];
    if (r < 0 || r >= n_reads) return "request names a read outside the batch";
    const int l = (int)(std::upper_bound(b->read_off, b->read_off + n_loci + 1, r) - b->read_off) - 1;
    const int32_t* nopts = b->blk_nopts + 3*l;
    if (k < 0 || k >= nopts[0]*nopts[1]*nopts[2]) return "request names an allele outside its locus";
    int s;
    if (const char* why = trace_seed_of(b, l, r, req_seed, q, s)) return why;
    const int len = b->base_off[r+1] - b->base_off[r];
    R.locus[q] = l; R.seed[q] = s; R.len[q] = len;
    const int64_t key = ((int64_t)l << 32) | (uint32_t)k;
    std::map<int64_t, int>::iterator hit = slot.find(key);
    if (hit == slot.end()){
      if (const char* why = hipstr::stutter_model_refusal(b->stutter + 6*l)) return why;     // (a locus no request names is never read)
      TracePair p; p.locus = l; p.allele = k;
      int32_t oi[3];
      hipstr::allele_options(nopts, k, oi);
      for (int x = 0, cur = opt_base[l]; x < 3; cur += nopts[x], x++){
        p.opt[x] = cur + oi[x]; p.len[x] = b->opt_off[p.opt[x]+1] - b->opt_off[p.opt[x]];
        if (p.len[x] < 1) return x == 1 ? "empty STR allele is not supported" : "empty flank sequence";
        if (x == 1 && p.len[x] > HS_MAX_STR_BP) return "STR allele longer than 2047 bp is not supported";
      }
      if (p.len[0] + 1 + p.len[2] > 4095) return "flanks longer than 4094 bases in total are not supported";
      hit = slot.insert(std::make_pair(key, (int)R.pairs.size())).first;
      R.pairs.push_back(p);
    }
    R.pair[q] = hit->second;
    const TracePair& p = R.pairs[hit->second];
    R.need[q] = trace_side_ws(p.len[0], p.len[2], s) + trace_side_ws(p.len[2], p.len[0], len - s - 1);
    R.rough += (int64_t)(p.len[0] + p.len[2] + 2)*len;
    if (at[r] < 0){ at[r] = (int32_t)R.wanted; R.wanted += len; }
    R.compact_off[q] = at[r];
  }
  return NULL;
}
// the slots of a request of a device-assembled call (hlen: its hap_to_ref string's length, -1 without)
TraceAsmCaps trace_req_asm_caps(const hipstr_batch_t* b, const TraceRequests& R, int q, int hlen){
  const int F0 = R.rows(q, 0, 0), B = R.rows(q, 0, 1), F2 = R.rows(q, 0, 2), period = b->period[R.locus[q]];
  return trace_asm_caps(trace_ops_cap(R.cols(q, 0), F0, F2, B, period), trace_ops_cap(R.cols(q, 1), F2, F0, B, period), R.len[q], F0, F2, hlen);
}

// ---- the launches of a chunk: the one derivation, for the call and for the plan.  Sides are launched grouped by columns-per-lane class
// (`items`: chunk-relative side indices in that order); the static classes in one launch for the requests of a locus or two
// (hs_trace_fill_mixed), else a launch per class.
struct TraceLaunch { int cl, first, count; };       // the class (0: hs_trace_fill_mixed; its kernel otherwise: trace_fill_cols), first item, sides
struct TraceLaunches {
  std::vector<int32_t> items;
  int cnt[HS_MAX_COLS + 1];        // sides per class, [1 .. HS_MAX_COLS]
  bool mixed;
  std::vector<TraceLaunch> fills;
};
void trace_launches(const TraceRequests& R, int q0, int q1, TraceLaunches& L){
  L.items.clear(); L.fills.clear();
  int n_cls = 0, first[HS_MAX_COLS + 1];
  for (int cl = 1; cl <= HS_MAX_COLS; cl++){
    first[cl] = (int)L.items.size();
    for (int si = 0; si < 2*(q1 - q0); si++) if (trace_col_class(R.cols(q0 + si/2, si & 1)) == cl) L.items.push_back(si);
    L.cnt[cl] = (int)L.items.size() - first[cl];
    n_cls += cl <= HS_TRACE_STATIC_CLASSES && L.cnt[cl] > 0;
  }
  L.mixed = trace_mixed_launch(n_cls, q1 - q0);
  if (L.mixed) L.fills.push_back(TraceLaunch{0, 0, first[HS_TRACE_STATIC_CLASSES + 1]});
  for (int cl = L.mixed ? HS_TRACE_STATIC_CLASSES + 1 : 1; cl <= HS_MAX_COLS; cl++)
    if (L.cnt[cl]) L.fills.push_back(TraceLaunch{cl, first[cl], L.cnt[cl]});
}
// an entry of the list on its way; 0, or 1 + last error
int trace_launch_fill(const TraceLaunches& L, const TraceLaunch& f, hipStream_t ks, const hs_tdev_t* d_args){
  static void (*const fill[HS_TRACE_STATIC_CLASSES])(const hs_tdev_t*, int) = { hs_trace_fill<1>, hs_trace_fill<2>, hs_trace_fill<3>, hs_trace_fill<4>, hs_trace_fill<5>, hs_trace_fill<6> };
  const int cols = trace_fill_cols(f.cl);
  int bad = 0;
  if (f.cl == 0){
    hs_tcls_t cls;
    for (int cl = 1, end = 0; cl <= HS_TRACE_STATIC_CLASSES; cl++){ end += L.cnt[cl]; cls.end[cl-1] = end; }
    hipLaunchKernelGGL(hs_trace_fill_mixed, dim3(f.count), dim3(64), 0, ks, d_args, cls);
  }
  else if (cols <= HS_TRACE_STATIC_CLASSES) hipLaunchKernelGGL(fill[cols-1], dim3(f.count), dim3(64), 0, ks, d_args, f.first);
  else bad = cols == 8 ? launch_fill_long<8>(f.count, ks, d_args, f.first) : cols == 12 ? launch_fill_long<12>(f.count, ks, d_args, f.first) : launch_fill_long<16>(f.count, ks, d_args, f.first);
  return bad ? hipstr::api_fail("hipFuncSetAttribute (traceback LDS) failed") : 0;
}

// ================================================================== the traceback call, stage by stage
// What every stage reads: the caller's arguments and the context's tables.
struct TraceCtx {
  const hipstr_batch_t* b; int32_t n_req; const int32_t *req_read, *req_allele; const char* const* hap_to_ref;
  bool on_device, timing;
  hipstr::ApiTables T; const hipstr::HostTables* HT;
};
// HIPSTR_TRACE_TIMING: the call's milliseconds by stage; lap() is the time since the last lap
struct TraceTimes {
  std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
  double prep = 0, fixed = 0, upload = 0, kernel = 0, d2h = 0, replay = 0, total = 0;
  double lap(){ const auto t = std::chrono::steady_clock::now(); const double d = std::chrono::duration<double, std::milli>(t - last).count(); last = t; total += d; return d; }
};

// ---- stage 2: the alleles of the distinct pairs: block strings in both orientations, rows under the allele's own homopolymer context,
// STR options; with hap_to_ref (a device-assembled call) the pool of the pairs' strings.  NULL or the refusal.
struct AllelePreps {
  std::vector<AllelePrep> v;       // by pair
  std::vector<hs_row_t> rows;
  hipstr::Prepared P;              // only its STR-option pools are used
  std::string h2r_pool;
};
const char* trace_prepare_alleles(const hipstr_batch_t* b, const TraceRequests& R, const char* const* hap_to_ref, AllelePreps& A){
  A.v.resize(R.pairs.size());
  for (size_t i = 0; i < R.pairs.size(); i++){
    const TracePair& p = R.pairs[i]; AllelePrep& ap = A.v[i];
    for (int x = 0; x < 3; x++){
      ap.seq[0][x].assign(b->seq + b->opt_off[p.opt[x]], (size_t)p.len[x]);
      ap.seq[1][2-x].assign(ap.seq[0][x].rbegin(), ap.seq[0][x].rend());
    }
    for (int sd = 0; sd < 2; sd++){
      std::vector<hs_row_t> lead, trail;
      hipstr::fresh_flank_rows(ap.seq[sd], lead, trail);
      ap.lead_off[sd] = A.rows.size();  A.rows.insert(A.rows.end(), lead.begin(), lead.end());
      ap.trail_off[sd] = A.rows.size(); A.rows.insert(A.rows.end(), trail.begin(), trail.end());
      ap.stropt[sd] = A.P.stropts.size();
      hipstr::append_stropt(ap.seq[sd][1], b->period[p.locus], b->stutter + 6*p.locus, A.P);
    }
    if (hap_to_ref){
      const char* s2 = hap_to_ref[b->hap_off[p.locus] + p.allele];
      ap.h2r_off = (int32_t)A.h2r_pool.size(); ap.h2r_len = (int32_t)strlen(s2);
      A.h2r_pool.append(s2, (size_t)ap.h2r_len);
      if (A.h2r_pool.size() > 0x7fffffff) return "too many requests for one call; split the request list";
    }
  }
  return NULL;
}

// What the fill and walk kernels leave — score, seed position, operation counts, artifact size and position per side, the operation
// strings — is one device block with the layout of the pinned block it is copied to: one copy per chunk.
struct TraceResBlock { size_t ll = 0, mxi = 0, nops = 0, ssz = 0, spos = 0, ops = 0, end = 0; char* d = NULL; };
// The records of a device-assembled chunk, again with the layout of the pinned block: totals and the first failure | five scalars per
// request | the running offsets | int32 pools | char pools.
struct TraceAsmBlock { size_t scal = 0, incl = 0, i32 = 0, chr = 0, end = 0; char* d = NULL; };
// What stages 3 and 4 leave for the chunks.
struct TraceWork {
  hipstr::HostArena st_arena;      // stage 3
  bool compact_reads = false;
  int64_t budget;                  // stage 4: bytes of decision matrices per chunk
  std::vector<hs_tside_t> sides;
  int max_nq = 0;
  hs_tdev_t hc = {};               // the static tables (stage 3) and the workspace
  TraceResBlock res;
  std::vector<TraceAsmCaps> acaps; // device assembly: slots per request, the staging and the result block
  TraceAsmBlock aout;
  hs_adev_t ad = {};               // blk_start, blk_end, h2r (stage 3); staging and the result block's pieces
};
// ---- stage 3: everything that does not change from chunk to chunk, in one pinned block and one copy: the alleles' tables and the reads'
// bases and qualities — only those of the requested reads when they are a small part of the batch (a few loci of a large batch: the whole
// batch's 150 MB cost more than the call's kernels); a device-assembled call adds the block coordinates and the hap_to_ref pool.
int trace_upload_static(const TraceCtx& C, const TraceRequests& R, const AllelePreps& A, TraceWork& W){
  const hipstr_batch_t* b = C.b;
  const int n_loci = b->n_loci, total_bases = b->base_off[b->read_off[n_loci]];
  std::vector<char> up_bases, up_quals;
  W.compact_reads = trace_compact_reads(R.wanted, total_bases);
  if (W.compact_reads){
    up_bases.resize((size_t)R.wanted); up_quals.resize((size_t)R.wanted);
    for (int q = 0; q < C.n_req; q++){
      const int r = C.req_read[q];
      memcpy(up_bases.data() + R.compact_off[q], b->bases + b->base_off[r], (size_t)R.len[q]);
      memcpy(up_quals.data() + R.compact_off[q], b->quals + b->base_off[r], (size_t)R.len[q]);
    }
  }
  const char* const src_bases = W.compact_reads ? up_bases.data() : b->bases;
  const char* const src_quals = W.compact_reads ? up_quals.data() : b->quals;
  const size_t n_up = W.compact_reads ? up_bases.size() : (size_t)total_bases;
  hipstr::HostArena& ar = W.st_arena; const hipstr::Prepared& P = A.P; const bool dv = C.on_device;
  const size_t o_bs = dv ? ar.add(b->blk_start, 3*(size_t)n_loci*sizeof(int32_t)) : 0, o_be = dv ? ar.add(b->blk_end, 3*(size_t)n_loci*sizeof(int32_t)) : 0,
               o_h2r = dv ? ar.add(A.h2r_pool.data(), A.h2r_pool.size()) : 0;
  const size_t o_rows = ar.add(A.rows.data(), A.rows.size()*sizeof(hs_row_t)), o_so = ar.add(P.stropts.data(), P.stropts.size()*sizeof(hs_stropt_t)),
               o_vis = ar.add(P.visits.data(), P.visits.size()*sizeof(hs_visit_t)), o_f64 = ar.add(P.f64pool.data(), P.f64pool.size()*sizeof(double)),
               o_chars = ar.add(P.chars.data(), P.chars.size()), o_bases = ar.add(src_bases, n_up), o_quals = ar.add(src_quals, n_up);
  if (ar.reserve(C.T.ctx)) return hipstr::api_fail("out of device or pinned host memory");
  if (ar.send(C.T.stream)) return 1;
  hs_tdev_t& h = W.hc;
  h.rows = ar.at<hs_row_t>(o_rows); h.stropts = ar.at<hs_stropt_t>(o_so); h.visits = ar.at<hs_visit_t>(o_vis);
  h.f64pool = ar.at<double>(o_f64); h.chars = ar.at<char>(o_chars); h.bases = ar.at<char>(o_bases); h.quals = ar.at<char>(o_quals);
  if (dv){ W.ad.blk_start = ar.at<int32_t>(o_bs); W.ad.blk_end = ar.at<int32_t>(o_be); W.ad.h2r = ar.at<char>(o_h2r); }
  h.int_log = C.T.int_log; h.qual_correct = C.T.qual_correct; h.qual_error = C.T.qual_error; h.m2m = C.T.m2m; h.m2i = C.T.m2i;
  h.log_thresh = C.HT->log_thresh;
  return 0;
}

// device assembly: slots per request, the staging and the result block sized for the largest chunk
int trace_alloc_assembly(const TraceCtx& C, const TraceRequests& R, const AllelePreps& A, hipstr::ScratchBufs& dev, TraceWork& W){
  const int n_req = C.n_req;
  W.acaps.resize(n_req);
  for (int q = 0; q < n_req; q++) W.acaps[q] = trace_req_asm_caps(C.b, R, q, A.v[R.pair[q]].h2r_len);
  int64_t mx_cap[5] = {0, 0, 0, 0, 0};                  // per chunk at most: hap_aln, seq, indel, snp, stitched entries
  for (int q0 = 0; q0 < n_req; ){
    const int q1 = trace_chunk_end(R.need, q0, W.budget);
    int64_t c[5] = {0, 0, 0, 0, 0};
    for (int q = q0; q < q1; q++){ const TraceAsmCaps& a = W.acaps[q]; c[0] += a.hap_aln; c[1] += a.seq; c[2] += a.indel; c[3] += a.snp; c[4] += a.stitched; }
    for (int i = 0; i < 5; i++) mx_cap[i] = std::max(mx_cap[i], c[i]);
    q0 = q1;
  }
  for (int i = 0; i < 5; i++) if (2*mx_cap[i] > 0x7fffffff) return hipstr::api_fail("too many requests for one call; split the request list");
  const size_t nqm = (size_t)W.max_nq, n_in = (size_t)mx_cap[2], n_sn = (size_t)mx_cap[3], n_fa = (size_t)mx_cap[4];
  hs_adev_t& ad = W.ad; TraceAsmBlock& B = W.aout;
  if (dev.alloc(&ad.st_indel_pos, n_in) || dev.alloc(&ad.st_indel_size, n_in) || dev.alloc(&ad.st_snp_pos, n_sn) || dev.alloc(&ad.st_cig_len, n_fa) ||
      dev.alloc(&ad.st_snp_base, n_sn) || dev.alloc(&ad.st_fa, n_fa) || dev.alloc(&ad.st_cig_op, n_fa) || dev.alloc(&ad.st_aln, n_fa) ||
      dev.alloc(&ad.lens, 8*nqm) || dev.alloc(&ad.excl, 8*nqm) || dev.alloc(&ad.rng, 3*nqm) || dev.alloc(&ad.fail, nqm)) return 1;
  B.scal = 64; B.incl = B.scal + 5*nqm*4; B.i32 = B.incl + 8*nqm*4;
  B.chr = B.i32 + (2*n_in + n_sn + n_fa)*4;
  B.end = B.chr + (size_t)mx_cap[0] + 3*(size_t)mx_cap[1] + n_sn + 2*n_fa;
  if (dev.alloc(&B.d, B.end)) return 1;
  ad.totals = (int64_t*)B.d; ad.first_fail = (int32_t*)(B.d + HS_ASM_POOLS*8);
  int32_t* sc = (int32_t*)(B.d + B.scal);
  ad.stutter_size = sc; ad.flank_ins = sc + nqm; ad.flank_del = sc + 2*nqm; ad.aln_start = sc + 3*nqm; ad.aln_stop = sc + 4*nqm;
  ad.incl = (int32_t*)(B.d + B.incl);
  int32_t* pi = (int32_t*)(B.d + B.i32);
  ad.p_indel_pos = pi; ad.p_indel_size = pi + n_in; ad.p_snp_pos = pi + 2*n_in; ad.p_cig_len = pi + 2*n_in + n_sn;
  char* pc = B.d + B.chr;
  ad.p_hap_aln = pc; ad.p_str_seq = pc + mx_cap[0]; ad.p_flank = ad.p_str_seq + mx_cap[1]; ad.p_snp_base = ad.p_flank + 2*mx_cap[1];
  ad.p_cig_op = ad.p_snp_base + n_sn; ad.p_aln = ad.p_cig_op + n_fa;
  ad.dense_cap[0] = mx_cap[0]; ad.dense_cap[1] = mx_cap[1]; ad.dense_cap[2] = 2*mx_cap[1]; ad.dense_cap[3] = mx_cap[2]; ad.dense_cap[4] = mx_cap[3];
  ad.dense_cap[5] = ad.dense_cap[6] = mx_cap[4];
  return 0;
}
// ---- stage 4: the budget of a chunk, the sides, and the workspace and result blocks sized for the largest chunk once and reused
// (the query costs as much as a small call's kernels: only a call whose matrices could exceed 256 MiB asks — an upper bound from the
//  longest read and the flank lengths of the first allele is enough to tell)
int trace_workspace(const TraceCtx& C, const TraceRequests& R, const AllelePreps& A, hipstr::ScratchBufs& dev, TraceWork& W){
  W.budget = (int64_t)HS_TRACE_BUDGET_MIB << 20;
  if (trace_asks_device(R.rough)){
    size_t free_b = 0, total_b = 0;
    HS_HIP(hipMemGetInfo(&free_b, &total_b));
    W.budget = std::min<int64_t>((int64_t)8 << 30, (int64_t)(free_b / 4));
  }
  W.budget = trace_env_budget(W.budget);
  W.sides.resize(2*(size_t)C.n_req);
  for (int q = 0; q < C.n_req; q++){
    const AllelePrep& ap = A.v[R.pair[q]];
    for (int sd = 0; sd < 2; sd++){
      hs_tside_t& S = W.sides[2*q+sd];
      memset(&S, 0, sizeof S);
      S.base_off = W.compact_reads ? R.compact_off[q] : C.b->base_off[C.req_read[q]]; S.len = R.len[q]; S.seed = R.seed[q]; S.side = sd;
      S.n = R.cols(q, sd);
      S.lead_off = ap.lead_off[sd]; S.F0 = R.rows(q, sd, 0);
      S.trail_off = ap.trail_off[sd]; S.F2 = R.rows(q, sd, 2);
      S.stropt = ap.stropt[sd];
      S.ops_cap = trace_ops_cap(S.n, S.F0, S.F2, R.rows(q, sd, 1), C.b->period[R.locus[q]]);
    }
    if (R.need[q] > W.budget) return hipstr::api_fail("one traceback needs more workspace than the device offers");
  }
  // workspaces are sized for the largest chunk once and reused
  const std::vector<hs_tside_t>& sides = W.sides;
  int64_t max_mat = 0, max_art = 0, max_ops = 0, max_lc = 0;
  {
    int64_t mat = 0, art = 0, ops = 0, lc = 0; int nq = 0;
    for (int q = 0; q < C.n_req; q++){
      if (mat + R.need[q] > W.budget){ mat = art = ops = lc = 0; nq = 0; }
      mat += R.need[q]; art += 2*(int64_t)(sides[2*q].n + sides[2*q+1].n); ops += sides[2*q].ops_cap + sides[2*q+1].ops_cap; nq++;
      lc += 2*(int64_t)(sides[2*q].F0 + 1 + sides[2*q].F2);
      max_mat = std::max(max_mat, mat); max_art = std::max(max_art, art); max_ops = std::max(max_ops, ops); max_lc = std::max(max_lc, lc);
      W.max_nq = std::max(W.max_nq, nq);
    }
  }
  if (max_art > 0x7fffffff || max_ops > 0x7fffffff || max_lc > 0x7fffffff) return hipstr::api_fail("too many requests for one call; split the request list");
  hs_tdev_t& hc = W.hc; TraceResBlock& B = W.res;
  if (dev.alloc(&hc.dec, max_mat) || dev.alloc(&hc.lastcol, max_lc) || dev.alloc(&hc.arts, max_art) || dev.alloc(&hc.side_prob, 2*(size_t)W.max_nq)) return 1;
  const size_t nqm = (size_t)W.max_nq;
  B.mxi = B.ll + nqm*8; B.nops = B.mxi + nqm*4; B.ssz = B.nops + 2*nqm*4; B.spos = B.ssz + 2*nqm*4;
  B.ops = (B.spos + 2*nqm*4 + 15) & ~(size_t)15; B.end = B.ops + (size_t)(max_ops ? max_ops : 1);
  if (dev.alloc(&B.d, B.end)) return 1;
  hc.ll = (double*)(B.d + B.ll); hc.max_index = (int32_t*)(B.d + B.mxi); hc.n_ops = (int32_t*)(B.d + B.nops);
  hc.str_size = (int32_t*)(B.d + B.ssz); hc.str_pos = (int32_t*)(B.d + B.spos); hc.ops = B.d + B.ops;
  return C.on_device ? trace_alloc_assembly(C, R, A, dev, W) : 0;
}


// ---- stage 5, per chunk: lay out the sides, upload, launch, then one of the three finishers
struct TraceEvents { hipEvent_t e[2] = {NULL, NULL}; ~TraceEvents(){ for (hipEvent_t x : e) if (x) hipEventDestroy(x); } };
struct TraceChunk {
  int q0, q1, nq; int64_t n_ops = 0;
  TraceLaunches L;
  hipstr::HostArena arena;         // this chunk's sides, launch order and argument block
  const hs_tdev_t* d_args = NULL;
  hs_adev_t ac;                    // device assembly: the call's pointers, this chunk's requests, the totals of the chunks done
  TraceEvents ev;                  // around the assembly kernels, when the call is timed
  TraceChunk(int a, int b) : q0(a), q1(b), nq(b - a) {}
};
int trace_chunk_upload(const TraceCtx& C, const TraceRequests& R, const AllelePreps& A, TraceWork& W, const int64_t pool_total[HS_ASM_POOLS], TraceChunk& Ch){
  const int q0 = Ch.q0, q1 = Ch.q1, nq = Ch.nq;
  int64_t mat = 0, n_art = 0, n_ops = 0, n_lc = 0;
  for (int q = q0; q < q1; q++){
    for (int sd = 0; sd < 2; sd++){
      hs_tside_t& S = W.sides[2*q+sd];
      S.dec_off = mat; mat += trace_side_ws(S.F0, S.F2, S.n);
      S.lc_off = (int32_t)n_lc; n_lc += S.F0 + 1 + S.F2;
      S.art_off = (int32_t)n_art; n_art += 2*S.n;
      S.ops_off = (int32_t)n_ops; n_ops += S.ops_cap;
    }
  }
  Ch.n_ops = n_ops;
  trace_launches(R, q0, q1, Ch.L);
  hs_tdev_t hcc = W.hc;
  std::vector<hs_areq_t> areqs;
  if (C.on_device){
    areqs.resize(nq);
    int64_t at_in = 0, at_sn = 0, at_fa = 0;
    for (int q = q0; q < q1; q++){
      hs_areq_t& Q = areqs[q-q0]; const AllelePrep& ap = A.v[R.pair[q]]; const TraceAsmCaps& c = W.acaps[q];
      Q.loc = R.locus[q]; Q.h2r_off = ap.h2r_off; Q.h2r_len = ap.h2r_len;
      Q.indel_cap = c.indel; Q.snp_cap = c.snp; Q.fa_cap = c.stitched;
      Q.indel_off = at_in; Q.snp_off = at_sn; Q.fa_off = at_fa;
      at_in += c.indel; at_sn += c.snp; at_fa += c.stitched;
    }
  }
  hipstr::HostArena& ar = Ch.arena;
  const size_t o_sides = ar.add(W.sides.data() + 2*q0, 2*(size_t)nq*sizeof(hs_tside_t)), o_items = ar.add(Ch.L.items.data(), Ch.L.items.size()*sizeof(int32_t)),
               o_args = ar.add(&hcc, sizeof hcc), o_areq = C.on_device ? ar.add(areqs.data(), areqs.size()*sizeof(hs_areq_t)) : 0;
  // (the argument block points into the arena it travels in: sizes first, then the pointers, then the copy)
  if (ar.reserve(C.T.ctx)) return hipstr::api_fail("out of device or pinned host memory");
  hcc.sides = ar.at<hs_tside_t>(o_sides); hcc.items = ar.at<int32_t>(o_items);
  if (ar.send(C.T.stream)) return 1;
  Ch.d_args = ar.at<hs_tdev_t>(o_args);
  if (C.on_device){
    Ch.ac = W.ad;
    Ch.ac.reqs = ar.at<hs_areq_t>(o_areq); Ch.ac.nq = nq;
    for (int p = 0; p < HS_ASM_POOLS; p++) Ch.ac.base[p] = pool_total[p];
  }
  return 0;
}
// the fill kernels of the launch list, the walk; device assembly: assemble, offsets, compaction
int trace_chunk_launch(const TraceCtx& C, TraceChunk& Ch){
  const hipStream_t st = C.T.stream;
  for (const TraceLaunch& f : Ch.L.fills) if (trace_launch_fill(Ch.L, f, st, Ch.d_args)) return 1;
  hipLaunchKernelGGL(hs_trace_walk, dim3(Ch.nq), dim3(64), 0, st, Ch.d_args, 0);
  if (C.on_device){
    if (C.timing){ HS_HIP(hipEventCreate(&Ch.ev.e[0])); HS_HIP(hipEventCreate(&Ch.ev.e[1])); HS_HIP(hipEventRecord(Ch.ev.e[0], st)); }
    hipLaunchKernelGGL(hs_trace_assemble, dim3(Ch.nq), dim3(64), 0, st, Ch.d_args, Ch.ac);
    hipLaunchKernelGGL(hs_trace_scan, dim3(HS_ASM_POOLS + 1), dim3(64), 0, st, Ch.ac);
    hipLaunchKernelGGL(hs_trace_compact, dim3(Ch.nq), dim3(64), 0, st, Ch.d_args, Ch.ac);
    if (C.timing) HS_HIP(hipEventRecord(Ch.ev.e[1], st));
  }
  HS_HIP(hipGetLastError());
  return 0;
}

// ---- finisher 1: the operation strings come home and the host replays them (HapAligner.cpp:642-707) and stitches
struct ChunkFetched { const double* ll; const int32_t *mxi, *nops, *ssz, *spos; const char* ops; };      // a chunk's results in its pinned block
// one request: qi its place in the chunk, S its two sides
void replay_request(const TraceCtx& C, const TraceRequests& RQ, const AllelePrep& ap, const hs_tside_t* S, int q, const ChunkFetched& F, int qi, ReqOut& R){
  const hipstr_batch_t* b = C.b;
  const int r = C.req_read[q], sb = RQ.seed[q], l = RQ.locus[q], len = RQ.len[q];
  const char* bases = b->bases + b->base_off[r];
  const char* quals = b->quals + b->base_off[r];
  const int max_index = F.mxi[qi];
  const int blen3[3] = { (int)ap.seq[0][0].size(), (int)ap.seq[0][1].size(), (int)ap.seq[0][2].size() };
  const int H = blen3[0] + blen3[1] + blen3[2];
  // left retrace, then the seed base joins the flank it sits in, then the right retrace (HapAligner.cpp:642-684)
  std::string side_ops[2];
  int seed_block = 0;
  for (int x = 0, crd = max_index; x < 3; x++){ if (crd < blen3[x]){ seed_block = x; break; } crd -= blen3[x]; }
  for (int sd = 0; sd < 2 && R.ok; sd++){
    const int cnt = F.nops[2*qi+sd];
    if (cnt > S[sd].ops_cap){ R.ok = false; break; }
    side_ops[sd].assign(F.ops + S[sd].ops_off, cnt);
    if (sd == 1 && seed_block != 1) R.acc.flank[seed_block].push_back(bases[sb]);
    const int mx = sd ? H-1-max_index : max_index;
    if (mx == 0) continue;                         // this side is all soft clips
    const int n = S[sd].n;
    std::string rd(n, ' '); std::vector<double> lc(n);
    for (int j = 0; j < n; j++){
      const int src = sd ? len-1-j : j;
      rd[j] = bases[src]; lc[j] = C.HT->qual_correct[(uint8_t)quals[src]];
    }
    int blk = 0, crd = mx;
    for (int x = 0; x < 3; x++){ const int bl = ap.seq[sd][x].size(); if (crd < bl){ blk = x; break; } crd -= bl; }
    int block, base;
    if (crd == 0){ block = blk-1; base = (int)ap.seq[sd][block].size()-1; } else { block = blk; base = crd-1; }
    if (!replay_side(b, l, ap.seq[sd], sd != 0, rd, lc, side_ops[sd], F.ssz[2*qi+sd], F.spos[2*qi+sd], block, base, R.acc)) R.ok = false;
  }
  if (!R.ok) return;
  R.hap_aln.assign(side_ops[0].rbegin(), side_ops[0].rend());
  R.hap_aln.push_back('M');
  R.hap_aln += side_ops[1];
  if (C.hap_to_ref == NULL) return;
  // ---- stitch_alignment_trace (AlignmentTraceback.cpp:55-144)
  const std::string& full = R.hap_aln;
  const char* h2r = C.hap_to_ref[b->hap_off[l] + C.req_allele[q]];
  const int hlen = (int)strlen(h2r);
  int hap_index = max_index, hai = 0; int32_t seed_pos = b->blk_start[3*l];
  while (hap_index > 0 && hai < hlen){
    if (h2r[hai] == 'M' || h2r[hai] == 'I') hap_index--;
    if (h2r[hai] == 'M' || h2r[hai] == 'D') seed_pos++;
    hai++;
  }
  while (hai < hlen && h2r[hai] == 'D') hai++;
  int sbase = sb, rai = 0;
  while (sbase > 0 && rai < (int)full.size()){
    if (full[rai] == 'M' || full[rai] == 'I' || full[rai] == 'S') sbase--;
    rai++;
  }
  while (rai < (int)full.size() && full[rai] == 'D') rai++;
  std::string la, ra;
  stitch_dir(h2r, hlen, full, hai-1, rai-1, -1, la);
  std::reverse(la.begin(), la.end());
  stitch_dir(h2r, hlen, full, hai+1, rai+1, 1, ra);
  std::string fa = la + "M" + ra;
  for (size_t i = 0; i < fa.size(); i++){ if (fa[i] == 'I') fa[i] = 'S'; else break; }
  int32_t start = seed_pos, stop = seed_pos;
  for (char ch : la) if (ch == 'D' || ch == 'M') start--;
  for (char ch : ra) if (ch == 'D' || ch == 'M') stop++;
  R.aln_start = start; R.aln_stop = stop;
  char cc = fa[0]; int num = 1;
  for (size_t i = 1; i <= fa.size(); i++){
    if (i == fa.size() || fa[i] != cc){
      R.cigar.push_back(std::make_pair(cc, (int32_t)num));
      if (i < fa.size()){ cc = fa[i]; num = 1; }
    } else num++;
  }
  int ri = 0;
  for (char ch : fa){
    if (ch == 'S') ri++;
    else if (ch == 'M' || ch == 'I') R.aln_str.push_back(bases[ri++]);
    else R.aln_str.push_back('-');
  }
}
int finish_host_replay(const TraceCtx& C, const TraceRequests& RQ, const AllelePreps& A, const TraceWork& W, const TraceChunk& Ch, hipstr_trace_out_t* o, TraceTimes& tm){
  const int q0 = Ch.q0, q1 = Ch.q1, nq = Ch.nq; const TraceResBlock& B = W.res;
  // results through one pinned block (a pageable destination costs a staging copy per call and per array), in one copy behind the kernels
  PinBlock pin(C.T.ctx, C.T.stream, B.end);
  if (!pin.p) return hipstr::api_fail("out of pinned host memory");
  HS_HIP(hipMemcpyAsync(pin.p, B.d, B.ops + (size_t)(Ch.n_ops ? Ch.n_ops : 1), hipMemcpyDeviceToHost, C.T.stream));
  HS_HIP(hipstr::wait_stream(C.T.stream));
  const ChunkFetched F = { (const double*)(pin.p + B.ll), (const int32_t*)(pin.p + B.mxi), (const int32_t*)(pin.p + B.nops), (const int32_t*)(pin.p + B.ssz),
                           (const int32_t*)(pin.p + B.spos), pin.p + B.ops };
  tm.d2h += tm.lap();
  // request by request; independent, so spread over host threads.  The replay is ~1.7 us of string work per request; the host threads are
  // a persistent pool (a few microseconds to wake), so a locus' hundred requests are already worth sharing: blocks of 24 requests
  std::vector<ReqOut> res(nq);
  int nthreads = std::max(1, std::min(hipstr::host_threads(), nq / 24));
  if (const char* e = getenv("HIPSTR_TRACE_THREADS")) nthreads = std::max(1, std::min(atoi(e), std::max(1, nq / 16)));
  auto run_parallel = [&](const std::function<void(int,int)>& fn){
    if (nthreads <= 1){ fn(q0, q1); return; }
    hipstr::parallel_for(nthreads, nthreads, [&](int t){ fn(q0 + (int)((int64_t)nq*t/nthreads), q0 + (int)((int64_t)nq*(t+1)/nthreads)); });
  };
  const double ms_setup = tm.lap();
  run_parallel([&](int qa, int qb){ for (int q = qa; q < qb; q++) replay_request(C, RQ, A.v[RQ.pair[q]], &W.sides[2*q], q, F, q-q0, res[q-q0]); });
  const double ms_work = tm.lap();
  if (hipstr::api_profile_on()) hipstr::api_profile_add(hipstr::PB_TRACE_REPLAY, ms_work*1e-3);
  // ---- the caller's flat pools: offsets in request order (serial prefix sums), then the bytes (parallel again)
  const TraceOutView V(o);
  const int64_t cap = o->cap_chars;
  for (int q = q0; q < q1; q++){
    const ReqOut& R = res[q-q0];
    if (!R.ok) return hipstr::api_fail("internal error: inconsistent traceback operation string");
    const size_t f0 = R.acc.flank[0].size(), f2 = R.acc.flank[2].size();
    const size_t n[HS_ASM_POOLS] = { R.hap_aln.size(), R.acc.str_set ? R.acc.str_seq.size() : 0, f0 + f2, R.acc.indels.size(), R.acc.snps.size(), R.cigar.size(), R.aln_str.size() };
    bool full = false;
    for (int p = 0; p < HS_ASM_POOLS; p++){
      int32_t* at = V.off[p] + hs_asm_pool_n(p, q);
      full = full || (int64_t)at[0] + (int64_t)n[p] > cap;
      if (p == 2){ at[1] = at[0] + (int32_t)f0; at[2] = at[1] + (int32_t)f2; }
      else at[1] = at[0] + (int32_t)n[p];
    }
    if (full) return hipstr::api_fail("hipstr_trace_out_t pools are too small (cap_chars)");
  }
  const double ms_offsets = tm.lap();
  run_parallel([&](int qa, int qb){
    for (int q = qa; q < qb; q++){
      const ReqOut& R = res[q-q0];
      o->ll[q] = F.ll[q-q0]; o->max_index[q] = F.mxi[q-q0];
      memcpy(o->hap_aln + o->hap_aln_off[q], R.hap_aln.data(), R.hap_aln.size());
      o->stutter_size[q] = R.acc.str_set ? R.acc.stutter_size : HIPSTR_NO_STR_DATA;
      if (R.acc.str_set) memcpy(o->str_seq + o->str_seq_off[q], R.acc.str_seq.data(), R.acc.str_seq.size());
      memcpy(o->flank_seq + o->flank_seq_off[2*q], R.acc.flank[0].data(), R.acc.flank[0].size());
      memcpy(o->flank_seq + o->flank_seq_off[2*q+1], R.acc.flank[2].data(), R.acc.flank[2].size());
      o->flank_ins[q] = R.acc.flank_ins; o->flank_del[q] = R.acc.flank_del;
      for (size_t i = 0; i < R.acc.indels.size(); i++){ o->indel_pos[o->indel_off[q] + i] = R.acc.indels[i].first; o->indel_size[o->indel_off[q] + i] = R.acc.indels[i].second; }
      for (size_t i = 0; i < R.acc.snps.size(); i++){ o->snp_pos[o->snp_off[q] + i] = R.acc.snps[i].first; o->snp_base[o->snp_off[q] + i] = R.acc.snps[i].second; }
      o->aln_start[q] = R.aln_start; o->aln_stop[q] = R.aln_stop;
      for (size_t i = 0; i < R.cigar.size(); i++){ o->cigar_op[o->cigar_off[q] + i] = R.cigar[i].first; o->cigar_len[o->cigar_off[q] + i] = R.cigar[i].second; }
      memcpy(o->aln_str + o->aln_str_off[q], R.aln_str.data(), R.aln_str.size());
    }
  });
  const double ms_copy = tm.lap();
  // a request's results are a dozen small heap blocks: let the threads that made them give them back, not this one at scope exit
  run_parallel([&](int qa, int qb){ for (int q = qa; q < qb; q++){ ReqOut none; std::swap(none, res[q-q0]); } });
  const double ms_release = tm.lap();
  if (C.timing) fprintf(stderr, "  replay of %d: setup %.3f work %.3f offsets %.3f copy %.3f release %.3f (threads %d)\n", nq, ms_setup, ms_work, ms_offsets, ms_copy, ms_release, nthreads);
  tm.replay += ms_setup + ms_work + ms_offsets + ms_copy + ms_release;
  return 0;
}

// ---- finisher 2: the records were assembled on the device; the totals, then every pool and array in one copy each to the caller's buffers
int finish_to_caller(const TraceCtx& C, const TraceWork& W, const TraceChunk& Ch, int64_t pool_total[HS_ASM_POOLS], hipstr_trace_out_t* o, TraceTimes& tm){
  const int q0 = Ch.q0, nq = Ch.nq; const TraceResBlock& B = W.res; const TraceAsmBlock& AB = W.aout;
  PinBlock pin(C.T.ctx, C.T.stream, B.nops + AB.end);
  if (!pin.p) return hipstr::api_fail("out of pinned host memory");
  char* hout = pin.p + B.nops;
  HS_HIP(hipMemcpyAsync(pin.p, B.d, B.nops, hipMemcpyDeviceToHost, C.T.stream));                  // ll, max_index
  HS_HIP(hipMemcpyAsync(hout, AB.d, AB.i32, hipMemcpyDeviceToHost, C.T.stream));                  // totals, scalars, offsets
  HS_HIP(hipstr::wait_stream(C.T.stream));
  if (C.timing){
    float kms = 0; HS_HIP(hipEventElapsedTime(&kms, Ch.ev.e[0], Ch.ev.e[1]));
    fprintf(stderr, "  assemble + scan + compact of %d: %.3f ms on the device\n", nq, kms);
  }
  const int64_t* tot = (const int64_t*)hout;
  const int32_t first_fail = *(const int32_t*)(hout + HS_ASM_POOLS*8);
  const int32_t* incl = (const int32_t*)(hout + AB.incl);
  const int64_t cap = o->cap_chars;
  // the host path's order: request by request, an inconsistent operation string before a full pool
  int first_full = -1;
  { bool over = false; for (int p = 0; p < HS_ASM_POOLS; p++) over = over || tot[p] > cap;
    if (over) for (int q = 0; q < nq && first_full < 0; q++) for (int p = 0; p < HS_ASM_POOLS; p++){
      const int i = hs_asm_pool_at(p, nq) + (p == 2 ? 2*q+1 : q);
      // (the offsets are 32-bit: one that wrapped is past any capacity too)
      if (incl[i] > cap || incl[i] < 0){ first_full = q; break; }
    }
    if (over && first_full < 0) first_full = 0; }
  if (first_fail >= 0 && (first_full < 0 || first_fail <= first_full)) return hipstr::api_fail("internal error: inconsistent traceback operation string");
  if (first_full >= 0) return hipstr::api_fail("hipstr_trace_out_t pools are too small (cap_chars)");
  tm.d2h += tm.lap();
  const TraceOutView V(o); const AsmDense dense = asm_dense(W.ad);
  std::vector<HomePiece> home;
  for (int a = 0; a < HS_TRACE_DEV_ARRAYS; a++){
    const int p = TD_ARR_POOL[a]; const size_t esz = TD_ARR_ESZ[a];
    home.push_back(HomePiece{dense.p[a], (size_t)(tot[p] - pool_total[p])*esz, (char*)V.arr[a] + (size_t)pool_total[p]*esz, (size_t)(dense.p[a] - AB.d)});
  }
  if (copy_home(C.T.stream, hout, home)) return 1;
  memcpy(V.ll + q0, pin.p + B.ll, (size_t)nq*8); memcpy(V.max_index + q0, pin.p + B.mxi, (size_t)nq*4);
  const int32_t* sc = (const int32_t*)(hout + AB.scal);
  for (int i = 0; i < 5; i++) memcpy(V.scal[i] + q0, sc + (size_t)i*W.max_nq, (size_t)nq*4);
  for (int p = 0; p < HS_ASM_POOLS; p++)
    memcpy(V.off[p] + hs_asm_pool_n(p, q0) + 1, incl + hs_asm_pool_at(p, nq), (size_t)hs_asm_pool_n(p, nq)*4);
  for (int p = 0; p < HS_ASM_POOLS; p++) pool_total[p] = tot[p];
  tm.replay += tm.lap();
  return 0;
}

// ---- finisher 3: the records stay.  Only the totals block comes home; the chunk's dense pieces go device-to-device into a segment of
// exactly their size (the next chunk's kernels reuse the staging and result blocks: they queue behind these copies on the same stream)
int finish_resident(const TraceCtx& C, const TraceWork& W, const TraceChunk& Ch, int64_t pool_total[HS_ASM_POOLS], TraceSegs& segs){
  const int nq = Ch.nq; const hipStream_t st = C.T.stream;
  int64_t tot[HS_ASM_POOLS], cnt[HS_ASM_POOLS];
  {
    PinBlock tb(C.T.ctx, st, W.aout.scal);
    if (!tb.p) return hipstr::api_fail("out of pinned host memory");
    HS_HIP(hipMemcpyAsync(tb.p, W.aout.d, W.aout.scal, hipMemcpyDeviceToHost, st));
    HS_HIP(hipstr::wait_stream(st));
    if (*(const int32_t*)(tb.p + HS_ASM_POOLS*8) >= 0) return hipstr::api_fail("internal error: inconsistent traceback operation string");
    memcpy(tot, tb.p, sizeof tot);
  }
  for (int p = 0; p < HS_ASM_POOLS; p++){
    if (tot[p] > 0x7fffffff) return hipstr::api_fail("too many requests for one call; split the request list");      // (the offsets are 32-bit)
    cnt[p] = tot[p] - pool_total[p];
  }
  hipstr_trace_dev* sg = trace_dev_new(C.T.ctx, st, nq, cnt);
  if (!sg) return 1;
  segs.v.push_back(sg); segs.q0.push_back(Ch.q0);
  HS_HIP(d2d(st, sg->ll, W.hc.ll, (size_t)nq*8)); HS_HIP(d2d(st, sg->max_index, W.hc.max_index, (size_t)nq*4));
  for (int i = 0; i < 5; i++) HS_HIP(d2d(st, sg->scal[i], W.ad.stutter_size + (size_t)i*W.max_nq, (size_t)nq*4));
  for (int p = 0; p < HS_ASM_POOLS; p++){
    HS_HIP(hipMemsetAsync(sg->off[p], 0, 4, st));           // (the leading 0: the first chunk's is the result's)
    HS_HIP(d2d(st, sg->off[p] + 1, W.ad.incl + hs_asm_pool_at(p, nq), (size_t)hs_asm_pool_n(p, nq)*4));
  }
  const AsmDense dense = asm_dense(W.ad);
  for (int a = 0; a < HS_TRACE_DEV_ARRAYS; a++) HS_HIP(d2d(st, sg->arr[a], dense.p[a], (size_t)cnt[TD_ARR_POOL[a]]*TD_ARR_ESZ[a]));
  for (int p = 0; p < HS_ASM_POOLS; p++) pool_total[p] = tot[p];
  return 0;
}

// ---- stage 6, the resident form: the handle.  One chunk: its segment is the result, nothing is copied twice.  Several (or none: the empty
// call): the segments side by side in flat arrays, then the segments go back (TraceSegs).
int join_segments(const TraceCtx& C, TraceSegs& segs, const int64_t pool_total[HS_ASM_POOLS], hipstr_trace_dev** res){
  const hipStream_t st = C.T.stream;
  TraceDevGuard g{NULL, st};
  if (segs.v.size() == 1){ g.t = segs.v[0]; segs.v.clear(); }
  else {
    hipstr_trace_dev* td = g.t = trace_dev_new(C.T.ctx, st, C.n_req, pool_total);
    if (!td) return 1;
    int64_t at[HS_ASM_POOLS] = {0, 0, 0, 0, 0, 0, 0};
    for (int p = 0; p < HS_ASM_POOLS; p++) HS_HIP(hipMemsetAsync(td->off[p], 0, 4, st));
    for (size_t c = 0; c < segs.v.size(); c++){
      const hipstr_trace_dev* sg = segs.v[c]; const int q0 = segs.q0[c], nq = sg->n_req;
      HS_HIP(d2d(st, td->ll + q0, sg->ll, (size_t)nq*8)); HS_HIP(d2d(st, td->max_index + q0, sg->max_index, (size_t)nq*4));
      for (int i = 0; i < 5; i++) HS_HIP(d2d(st, td->scal[i] + q0, sg->scal[i], (size_t)nq*4));
      for (int p = 0; p < HS_ASM_POOLS; p++) HS_HIP(d2d(st, td->off[p] + hs_asm_pool_n(p, q0) + 1, sg->off[p] + 1, (size_t)hs_asm_pool_n(p, nq)*4));
      for (int a = 0; a < HS_TRACE_DEV_ARRAYS; a++){
        const int p = TD_ARR_POOL[a];
        HS_HIP(d2d(st, td->arr[a] + (size_t)at[p]*TD_ARR_ESZ[a], sg->arr[a], (size_t)sg->totals[p]*TD_ARR_ESZ[a]));
      }
      for (int p = 0; p < HS_ASM_POOLS; p++) at[p] += sg->totals[p];
    }
    HS_HIP(hipstr::wait_stream(st));
  }
  if (hipstr::wait_stream(st) != hipSuccess) return hipstr::api_fail("hipstr_hmm_trace_resident: the device failed");
  g.t->n_req = C.n_req; g.t->groups = HIPSTR_TRACE_F_ALL; g.t->checked = true;
  *res = g.release();
  return 0;
}

// flags 0: the host replays the operation strings; HIPSTR_TRACE_ASSEMBLE_DEVICE: hs_trace_assemble / _scan / _compact build the records, which
// go to the caller's buffers (o) or stay on the device (res: a handle, complete when the call returns)
int trace_call(const hipstr_batch_t* b, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
               const int32_t* req_seed, const char* const* hap_to_ref, uint32_t flags, hipstr_trace_out_t* o, hipstr_trace_dev** res){
  hipstr::ApiTimer prof_t(hipstr::PB_TRACE);
  using hipstr::api_fail;
  if (!b || (!o && !res) || n_req < 0 || (n_req > 0 && (!req_read || !req_allele))) return api_fail("null argument");
  if (b->n_loci < 1) return api_fail("hipstr_hmm_trace needs at least one locus");
  { std::string bad; if (hipstr::validate_tables(b, bad)) return api_fail(bad); }
  TraceCtx C = { b, n_req, req_read, req_allele, hap_to_ref, (flags & HIPSTR_TRACE_ASSEMBLE_DEVICE) != 0, getenv("HIPSTR_TRACE_TIMING") != NULL };
  TraceTimes tm;
  if (hipstr::api_device_tables(&C.T)) return 1;
  C.HT = &hipstr::host_tables();
  // ---- 1: what the request list means, or why it is refused
  TraceRequests R;
  if (const char* why = trace_resolve(b, n_req, req_read, req_allele, req_seed, R)) return api_fail(why);
  if (o){ const TraceOutView V(o); for (int p = 0; p < HS_TRACE_DEV_POOLS; p++) V.off[p][0] = 0; }
  int64_t pool_total[HS_ASM_POOLS] = {0, 0, 0, 0, 0, 0, 0};       // device assembly: totals of the chunks done
  TraceSegs segs; segs.st = C.T.stream;                          // resident result: a segment per chunk
  if (n_req == 0) return res ? join_segments(C, segs, pool_total, res) : 0;      // (no segments: a valid empty handle, the seven leading zeros)
  // ---- 2: the alleles of its distinct (locus, allele) pairs
  AllelePreps A;
  if (const char* why = trace_prepare_alleles(b, R, C.on_device ? hap_to_ref : NULL, A)) return api_fail(why);
  tm.prep = tm.lap();
  // ---- 3, 4: the static upload; the budget, the sides, the workspace
  hipstr::ScratchBufs dev;
  dev.runs_on(C.T.stream);
  TraceWork W;
  if (trace_upload_static(C, R, A, W) || trace_workspace(C, R, A, dev, W)) return 1;
  tm.fixed = tm.lap();
  // ---- 5: chunks of requests whose matrices fit the budget
  for (int q0 = 0; q0 < n_req; ){
    TraceChunk Ch(q0, trace_chunk_end(R.need, q0, W.budget));
    if (trace_chunk_upload(C, R, A, W, pool_total, Ch)) return 1;
    tm.upload += tm.lap();
    if (trace_chunk_launch(C, Ch)) return 1;
    tm.kernel += tm.lap();
    if (res ? finish_resident(C, W, Ch, pool_total, segs) : C.on_device ? finish_to_caller(C, W, Ch, pool_total, o, tm) : finish_host_replay(C, R, A, W, Ch, o, tm)) return 1;
    q0 = Ch.q1;
  }
  // ---- 6
  if (res && join_segments(C, segs, pool_total, res)) return 1;
  if (C.timing)
    fprintf(stderr, "hipstr_hmm_trace: %d requests; prep %.3f ms, static upload+alloc %.3f, chunk upload %.3f, kernels %.3f, d2h %.3f, replay %.3f, total %.3f\n",
            n_req, tm.prep, tm.fixed, tm.upload, tm.kernel, tm.d2h, tm.replay, (tm.lap(), tm.total));
  return 0;
}

}  // namespace

// what trace_cache.hip builds its gathered handles with (api_internal.h)
hipstr_trace_dev* hipstr::trace_dev_make(hipstr::Ctx* ctx, hipStream_t st, int32_t n, const int64_t tot[HS_TRACE_DEV_POOLS]){ return trace_dev_new(ctx, st, n, tot); }
void hipstr::trace_dev_release(hipstr_trace_dev* td){ trace_dev_drop(td); }

extern "C" int hipstr_hmm_trace(const hipstr_batch_t* b, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                                const char* const* hap_to_ref, hipstr_trace_out_t* o){
  return hipstr_hmm_trace_seeded(b, n_req, req_read, req_allele, NULL, hap_to_ref, o);
}

extern "C" int hipstr_hmm_trace_seeded(const hipstr_batch_t* b, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                                       const int32_t* req_seed, const char* const* hap_to_ref, hipstr_trace_out_t* o){
  return trace_call(b, n_req, req_read, req_allele, req_seed, hap_to_ref, 0u, o, NULL);
}

extern "C" int hipstr_hmm_trace_ex(const hipstr_batch_t* b, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                                   const int32_t* req_seed, const char* const* hap_to_ref, uint32_t flags, hipstr_trace_out_t* o){
  if (flags & ~(uint32_t)HIPSTR_TRACE_ASSEMBLE_DEVICE) return hipstr::api_fail("hipstr_hmm_trace_ex: unknown flag bits");
  return trace_call(b, n_req, req_read, req_allele, req_seed, hap_to_ref, flags, o, NULL);
}

extern "C" int hipstr_hmm_trace_resident(const hipstr_batch_t* b, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                                         const int32_t* req_seed, const char* const* hap_to_ref, uint32_t flags, hipstr_trace_dev_t** td){
  if (td) *td = NULL;
  if (!td) return hipstr::api_fail("null argument");
  if (flags) return hipstr::api_fail("hipstr_hmm_trace_resident: unknown flag bits");
  return trace_call(b, n_req, req_read, req_allele, req_seed, hap_to_ref, HIPSTR_TRACE_ASSEMBLE_DEVICE, NULL, td);
}

// ---- the resident result's own entry points
extern "C" int hipstr_trace_dev_sizes(const hipstr_trace_dev_t* td, int32_t* n_req, int64_t totals[7]){
  if (!td || !n_req || !totals) return hipstr::api_fail("null argument");
  *n_req = td->n_req;
  for (int p = 0; p < HS_TRACE_DEV_POOLS; p++) totals[p] = td->totals[p];
  return 0;
}

extern "C" int hipstr_trace_dev_fetch(hipstr_trace_dev_t* td, uint32_t fields, hipstr_trace_out_t* o){
  using hipstr::api_fail;
  if (fields & ~(uint32_t)HIPSTR_TRACE_F_ALL) return api_fail("hipstr_trace_dev_fetch: unknown field bits");
  if (!td || !o) return api_fail("null argument");
  if (fields & ~td->groups) return api_fail("hipstr_trace_dev_fetch: the handle does not hold a chosen group");
  const size_t n = (size_t)td->n_req;
  const TraceOutView V(o);
  std::vector<HomePiece> home; size_t pin_bytes = 0; bool null_dst = false;
  auto want = [&](const void* dev, size_t nb, void* dst){
    if (nb && !dst) null_dst = true;
    home.push_back(HomePiece{dev, nb, dst, pin_bytes}); pin_bytes = (pin_bytes + nb + 255) & ~(size_t)255;
  };
  if (fields & HIPSTR_TRACE_F_SCALARS){
    want(td->ll, n*8, V.ll); want(td->max_index, n*4, V.max_index);
    for (int i = 0; i < 5; i++) want(td->scal[i], n*4, V.scal[i]);
  }
  for (int p = 0; p < HS_TRACE_DEV_POOLS; p++){
    if (!(fields & TD_POOL_BIT[p])) continue;
    if (td->totals[p] > (int64_t)o->cap_chars) return api_fail("hipstr_trace_out_t pools are too small (cap_chars)");
    want(td->off[p], ((size_t)hs_asm_pool_n(p, (int)n) + 1)*4, V.off[p]);
    for (int a = 0; a < HS_TRACE_DEV_ARRAYS; a++) if (TD_ARR_POOL[a] == p) want(td->arr[a], (size_t)td->totals[p]*TD_ARR_ESZ[a], V.arr[a]);
  }
  if (null_dst) return api_fail("null output array");
  if (pin_bytes == 0) return 0;
  if (hipstr::api_bind(td->ctx)) return 1;
  PinBlock pin(td->ctx, td->stream, pin_bytes);
  if (!pin.p) return api_fail("out of pinned host memory");
  return copy_home(td->stream, pin.p, home);
}

extern "C" void hipstr_trace_dev_free(hipstr_trace_dev_t* td){
  if (!td) return;
  if (td->block && hipstr::api_bind(td->ctx) == 0) hipStreamSynchronize(td->stream);     // a fetch that left early may still be copying
  trace_dev_drop(td);
}

#ifndef HIPSTR_NO_DEBUG_ABI
// Diagnostics: a resident result built from host arrays, for the fabricated cases of the census and the read counts.  An array that is NULL
// is absent (its group cannot be fetched, a consumer that needs it refuses); nothing is checked here: the consumers do that.
extern "C" int hipstr_debug_trace_dev_from_host(const hipstr_trace_out_t* tr, int32_t n_req, hipstr_trace_dev_t** out){
  using hipstr::api_fail;
  if (out) *out = NULL;
  if (!tr || !out || n_req < 0) return api_fail("null argument");
  const size_t n = (size_t)n_req;
  const TraceOutView V(tr);
  int64_t tot[HS_TRACE_DEV_POOLS]; bool pool_ok[HS_TRACE_DEV_POOLS];
  for (int p = 0; p < HS_TRACE_DEV_POOLS; p++){
    tot[p] = V.off[p] ? std::max<int64_t>(0, V.off[p][hs_asm_pool_n(p, n_req)]) : 0;
    pool_ok[p] = V.off[p] != NULL;
    for (int a = 0; a < HS_TRACE_DEV_ARRAYS; a++) if (TD_ARR_POOL[a] == p && tot[p] > 0 && !V.arr[a]) pool_ok[p] = false;
    if (!pool_ok[p]) tot[p] = 0;
  }
  hipstr::ApiTables T;
  if (hipstr::api_device_tables(&T)) return 1;
  TraceDevGuard g{trace_dev_new(T.ctx, T.stream, n_req, tot), T.stream};
  hipstr_trace_dev* td = g.t;
  if (!td) return 1;
  const TraceDevLayout L(n, tot);
  PinBlock pin(T.ctx, T.stream, L.bytes);
  if (!pin.p) return api_fail("out of pinned host memory");
  auto put = [&](size_t at, const void* src, size_t nb){ if (src && nb) memcpy(pin.p + at, src, nb); };
  put(L.ll, V.ll, n*8); put(L.mxi, V.max_index, n*4);
  if (!V.ll) td->ll = NULL;
  if (!V.max_index) td->max_index = NULL;
  bool scalars = V.ll && V.max_index;
  for (int i = 0; i < 5; i++){ put(L.scal[i], V.scal[i], n*4); if (!V.scal[i]){ td->scal[i] = NULL; scalars = false; } }
  uint32_t held = 0, lacking = 0;                 // group bits with a pool present / with a pool absent (a group of two pools needs both)
  for (int p = 0; p < HS_TRACE_DEV_POOLS; p++){
    (pool_ok[p] ? held : lacking) |= TD_POOL_BIT[p];
    if (!pool_ok[p]){ td->off[p] = NULL; for (int a = 0; a < HS_TRACE_DEV_ARRAYS; a++) if (TD_ARR_POOL[a] == p) td->arr[a] = NULL; continue; }
    put(L.off[p], V.off[p], ((size_t)hs_asm_pool_n(p, n_req) + 1)*4);
    for (int a = 0; a < HS_TRACE_DEV_ARRAYS; a++) if (TD_ARR_POOL[a] == p) put(L.arr[a], V.arr[a], (size_t)tot[p]*TD_ARR_ESZ[a]);
  }
  HS_HIP(hipMemcpyAsync(td->block, pin.p, L.bytes, hipMemcpyHostToDevice, T.stream));
  HS_HIP(hipstr::wait_stream(T.stream));
  td->groups = (scalars ? HIPSTR_TRACE_F_SCALARS : 0) | (held & ~lacking);
  td->checked = false;
  *out = g.release();
  return 0;
}

namespace {
// what both plans check before they resolve the request list, as the call does; NULL or the refusal
const char* plan_resolve(const hipstr_batch_t* b, int32_t n_req, const int32_t* req_read, const int32_t* req_allele, const int32_t* req_seed,
                         TraceRequests& R, std::string& err){
  if (!b || n_req < 0 || (n_req > 0 && (!req_read || !req_allele))) return "null argument";
  if (b->n_loci < 1) return "hipstr_hmm_trace needs at least one locus";
  if (hipstr::validate_tables(b, err)) return err.c_str();
  return trace_resolve(b, n_req, req_read, req_allele, req_seed, R);
}
int plan_bad(const char* why){ hipstr::api_fail(why); return -1; }
int plan_out(const std::string& o, char* json, int cap){
  if (json && cap > 0){ const size_t m = std::min(o.size(), (size_t)cap - 1); memcpy(json, o.data(), m); json[m] = 0; }
  return (int)o.size();
}
}  // namespace

// Diagnostics (host only): the chunks, fill kernels and walk forms hipstr_hmm_trace_seeded would launch for a request list, from what the
// call itself runs on (trace_resolve, trace_compact_reads, trace_chunk_end, trace_launches, hs_walk_in_lds), as one JSON object.
extern "C" int hipstr_debug_trace_plan(const hipstr_batch_t* b, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                                       const int32_t* req_seed, double ws_mib, char* json, int cap){
  TraceRequests R; std::string err;
  if (const char* why = plan_resolve(b, n_req, req_read, req_allele, req_seed, R, err)) return plan_bad(why);
  // (a call that would ask the device for its free memory: the plan takes the budget it was given, else the default)
  const int64_t budget = ws_mib > 0 ? (int64_t)(ws_mib*1048576.0) : trace_env_budget((int64_t)HS_TRACE_BUDGET_MIB << 20);
  for (int q = 0; q < n_req; q++) if (R.need[q] > budget) return plan_bad("one traceback needs more workspace than the device offers");
  const int64_t total_bases = b->base_off[b->read_off[b->n_loci]];
  const bool compact = n_req > 0 && trace_compact_reads(R.wanted, total_bases);
  std::string o; char buf[256];
  auto put = [&](const char* fmt, auto... a){ snprintf(buf, sizeof buf, fmt, a...); o += buf; };
  put("{\"thresholds\": {\"HS_MAX_COLS\": %d, \"HS_TRACE_STATIC_CLASSES\": %d, \"HS_TRACE_MIXED_MAX_REQ\": %d, \"HS_WALK_LDS\": %d, \"HS_TRACE_BUDGET_MIB\": %d, \"max_side\": %d, \"fill_cols\": [",
      HS_MAX_COLS, HS_TRACE_STATIC_CLASSES, HS_TRACE_MIXED_MAX_REQ, HS_WALK_LDS, HS_TRACE_BUDGET_MIB, 64*HS_MAX_COLS);
  for (int cl = 1; cl <= HS_MAX_COLS; cl++) put("%s%d", cl > 1 ? ", " : "", trace_fill_cols(cl));
  o += "]}, \"routes\": [";
  for (int cl = 1; cl <= HS_TRACE_STATIC_CLASSES; cl++) put("\"hs_trace_fill<%d>\", \"mixed<%d>\", ", cl, cl);
  for (int cl = HS_TRACE_STATIC_CLASSES + 1, last = 0; cl <= HS_MAX_COLS; cl++) if (trace_fill_cols(cl) != last){ last = trace_fill_cols(cl); put("\"hs_trace_fill_long<%d>\", ", last); }
  put("\"hs_trace_fill_mixed\", \"walk_lds\", \"walk_workspace\", \"reads_compact\", \"reads_whole\", \"trace_one_chunk\", \"trace_chunks\"], "
      "\"compact_reads\": %s, \"wanted_bases\": %lld, \"total_bases\": %lld, \"budget\": %lld, \"asks_device\": %s, \"chunks\": [",
      compact ? "true" : "false", (long long)R.wanted, (long long)total_bases, (long long)budget, trace_asks_device(R.rough) ? "true" : "false");
  TraceLaunches L;
  for (int q0 = 0; q0 < n_req; ){
    const int q1 = trace_chunk_end(R.need, q0, budget), nq = q1 - q0;
    int64_t mat = 0; int n_lds = 0, n_ws = 0;
    for (int q = q0; q < q1; q++) mat += R.need[q];
    trace_launches(R, q0, q1, L);
    put("%s{\"q0\": %d, \"q1\": %d, \"bytes\": %lld, \"classes\": [", q0 ? ", " : "", q0, q1, (long long)mat);
    for (int cl = 1; cl <= HS_MAX_COLS; cl++) put("%s%d", cl > 1 ? ", " : "", L.cnt[cl]);
    put("], \"mixed\": %s, \"launch\": [", L.mixed ? "true" : "false");
    for (const TraceLaunch& f : L.fills){
      if (f.cl == 0) put("[\"hs_trace_fill_mixed\", %d], ", f.count);
      else put(f.cl <= HS_TRACE_STATIC_CLASSES ? "[\"hs_trace_fill<%d>\", %d], " : "[\"hs_trace_fill_long<%d>\", %d], ", trace_fill_cols(f.cl), f.count);
    }
    // per request: [left columns, right columns, flank rows + 1, left walk, right walk] (walk: 1 = decisions copied to LDS, 0 = read in the workspace)
    put("[\"hs_trace_walk\", %d]], \"requests\": [", nq);
    for (int q = q0; q < q1; q++){
      const int nL = R.cols(q, 0), nR = R.cols(q, 1), F0 = R.rows(q, 0, 0), F2 = R.rows(q, 0, 2);
      const bool wl = hs_walk_in_lds(hs_trace_side_bytes(F0, F2, nL)), wr = hs_walk_in_lds(hs_trace_side_bytes(F2, F0, nR));
      n_lds += wl + wr; n_ws += !wl + !wr;
      put("%s[%d, %d, %d, %d, %d]", q > q0 ? ", " : "", nL, nR, F0 + 1 + F2, wl ? 1 : 0, wr ? 1 : 0);
    }
    o += "], \"routes\": [";
    put("\"%s\", \"%s\"", (q0 == 0 && q1 == n_req) ? "trace_one_chunk" : "trace_chunks", compact ? "reads_compact" : "reads_whole");
    if (L.mixed){
      o += ", \"hs_trace_fill_mixed\"";
      for (int cl = 1; cl <= HS_TRACE_STATIC_CLASSES; cl++) if (L.cnt[cl]) put(", \"mixed<%d>\"", cl);
    }
    for (size_t i = 0; i < L.fills.size(); i++){
      const TraceLaunch& f = L.fills[i];
      if (f.cl >= 1 && f.cl <= HS_TRACE_STATIC_CLASSES) put(", \"hs_trace_fill<%d>\"", f.cl);
      // (a long kernel is named once for a run of adjacent classes it serves)
      else if (f.cl > HS_TRACE_STATIC_CLASSES && !(i > 0 && L.fills[i-1].cl == f.cl - 1 && trace_fill_cols(f.cl - 1) == trace_fill_cols(f.cl)))
        put(", \"hs_trace_fill_long<%d>\"", trace_fill_cols(f.cl));
    }
    if (n_lds) o += ", \"walk_lds\"";
    if (n_ws) o += ", \"walk_workspace\"";
    o += "]}";
    q0 = q1;
  }
  o += "]}";
  return plan_out(o, json, cap);
}
// Diagnostics (host only): the slots and the staging route of every request of a device-assembled call, from trace_resolve, trace_req_asm_caps
// and hs_asm_in_lds — the functions hipstr_hmm_trace_ex and hs_trace_assemble call.
extern "C" int hipstr_debug_trace_assemble_plan(const hipstr_batch_t* b, int32_t n_req, const int32_t* req_read, const int32_t* req_allele,
                                                const int32_t* req_seed, const char* const* hap_to_ref, char* json, int cap){
  TraceRequests R; std::string err;
  if (const char* why = plan_resolve(b, n_req, req_read, req_allele, req_seed, R, err)) return plan_bad(why);
  std::string o; char buf[256];
  auto put = [&](const char* fmt, auto... a){ snprintf(buf, sizeof buf, fmt, a...); o += buf; };
  put("{\"thresholds\": {\"HS_ASM_LDS\": %d}, \"routes\": [\"assemble_lds\", \"assemble_hbm\"], "
      "\"fields\": [\"hap_aln\", \"seq\", \"indel\", \"snp\", \"stitched\", \"lds_bytes\", \"in_lds\"], \"requests\": [", HS_ASM_LDS);
  int n_lds = 0, n_hbm = 0;
  for (int q = 0; q < n_req; q++){
    const TracePair& p = R.pairs[R.pair[q]];
    const int hlen = hap_to_ref ? (int)strlen(hap_to_ref[b->hap_off[p.locus] + p.allele]) : -1;
    const TraceAsmCaps c = trace_req_asm_caps(b, R, q, hlen);
    const bool lds = hs_asm_in_lds(c.lds_bytes);
    n_lds += lds; n_hbm += !lds;
    put("%s[%d, %d, %d, %d, %d, %d, %d]", q ? ", " : "", c.hap_aln, c.seq, c.indel, c.snp, c.stitched, c.lds_bytes, lds ? 1 : 0);
  }
  o += "], \"routes_hit\": [";
  if (n_lds) o += "\"assemble_lds\"";
  if (n_hbm) o += n_lds ? ", \"assemble_hbm\"" : "\"assemble_hbm\"";
  o += "]}";
  return plan_out(o, json, cap);
}
#endif  // HIPSTR_NO_DEBUG_ABI
