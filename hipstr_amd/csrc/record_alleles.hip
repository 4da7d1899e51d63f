// record_alleles.hip — the alleles of a VCF record on the device: hipstr_record_alleles (include/hipstr_hmm.h) with its host form.
// hs_ra_kernel runs one wavefront per locus: the lanes run over the options of block 1 for every position's stop test of the two trims
// and the wavefront takes the AND (record_alleles_layout.h: the tests); the flanks and the pad come out of the locus' reference window;
// every lane writes its options' allele strings into the locus' piece of a pool (a fixed stride per option, so no offsets are needed
// before the lengths are known) and ranks them by counting the options that sort before each.  The host cuts the pool into the caller's
// offsets; a locus beyond HS_RA_MAX_OPTIONS takes the host twin inside the same call; the flank option strings are cut by the host twin
// from the returned trims in both forms (a few short strings per locus).
#include <hip/hip_runtime.h>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "api_internal.h"
#include "record_alleles_host.h"
#include "record_alleles_layout.h"

using hipstr::api_fail;
namespace ra = hipstr_rec_alleles;

static_assert(HS_RA_MAX_OPTIONS == HIPSTR_ALLELES_DEVICE_OPTIONS && HS_RA_DUPLICATE == HIPSTR_ALLELES_DUPLICATE && HS_RA_OUTSIDE == HIPSTR_ALLELES_OUTSIDE_WINDOW,
              "the header states the cap and the statuses");

__global__ __launch_bounds__(HS_RA_WAVE) void hs_ra_kernel(const hs_ra_dev_t* __restrict__ args){
  const hs_ra_dev_t d = *args;
  const hs_ra_locus_t L = d.loci[blockIdx.x];
  if (L.on_host) return;
  const int lane = threadIdx.x, V = L.n_opts;
  const int32_t* off = d.opt_off + L.opt0;
  const char* seq = d.seq;
  const int o0 = off[0], n0 = off[1] - off[0];
  // ---- the trims (:700-736): at most n0 steps each
  const int64_t gap_l = (int64_t)L.region_start - L.start, gap_r = (int64_t)L.end - L.region_stop;
  const int max_lt = (int)(gap_l < 0 ? 0 : gap_l > n0 ? n0 : gap_l), max_rt = (int)(gap_r < 0 ? 0 : gap_r > n0 ? n0 : gap_r);
  int lt = 0, rt = 0;
  bool go = true;
  for (int t = 0; t < max_lt && go; t++){
    bool stop = false;
    for (int i = lane; i < V && !stop; i += HS_RA_WAVE) stop = hs_ra_left_stop(seq, off[i], off[i + 1] - off[i], o0, n0, t);
    go = !__any(stop);
    if (go) lt = t + 1;
  }
  go = true;
  for (int t = 0; t < max_rt && go; t++){
    bool stop = false;
    for (int i = lane; i < V && !stop; i += HS_RA_WAVE) stop = hs_ra_right_stop(seq, off[i], off[i + 1] - off[i], o0, n0, lt, t);
    go = !__any(stop);
    if (go) rt = t + 1;
  }
  // ---- the flanks, pos and the pad (:738-758), the same on every lane
  const int64_t start = (int64_t)L.start + lt, end = (int64_t)L.end - rt, rs = L.region_start, re = L.region_stop, w0 = rs - HS_RA_WIN_PAD, w1 = w0 + L.win_len;
  const int64_t lf = start >= rs ? start - rs : 0, rf = end <= re ? re - end : 0;
  int status = 0;
  if (lf > 0 && (rs < 0 || rs + lf > w1)) status = HS_RA_OUTSIDE;
  if (rf > 0 && (end < 0 || end < w0 || end + rf > w1)) status = HS_RA_OUTSIDE;
  int64_t pos = rs < start ? rs : start;
  int pad = 0;
  if (lf == 0){
    const char first = n0 - lt - rt > 0 ? seq[o0 + lt] : (char)0;
    bool want = false;
    for (int i = lane; i < V && !want; i += HS_RA_WAVE) want = i >= 1 && (off[i + 1] - off[i] - lt - rt <= 0 || seq[off[i] + lt] != first);
    if (__any(want)){
      pad = 1; pos -= 1;
      if (pos < 0 || pos < w0 || pos >= w1) status = HS_RA_OUTSIDE;
    }
  }
  pos += 1;
  if (pos < INT32_MIN || pos > INT32_MAX) status = HS_RA_OUTSIDE;
  int32_t* const scal = d.scal + 4*(int64_t)blockIdx.x;
  if (status){
    if (lane == 0){ scal[0] = status; scal[1] = 0; scal[2] = 0; scal[3] = 0; }
    return;
  }
  // ---- the strings: [pad byte] left flank, option, right flank
  const char* const win = d.window + L.win_base;
  char* const pool = d.pool + L.pool_base;
  const int total_flank = (int)(pad + lf + rf);
  for (int i = lane; i < V; i += HS_RA_WAVE){
    const int mid = off[i + 1] - off[i] - lt - rt;
    char* s = pool + (int64_t)i*L.stride;
    if (mid + total_flank > L.stride){ d.out_len[L.var_off + i] = 0; continue; }      // (never: the stride is the bound)
    int at = 0;
    if (pad) s[at++] = hs_ra_upper(win[pos - 1 - w0]);
    for (int64_t k = 0; k < lf; k++) s[at++] = hs_ra_upper(win[rs - w0 + k]);
    for (int k = 0; k < mid; k++) s[at++] = seq[off[i] + lt + k];
    for (int64_t k = 0; k < rf; k++) s[at++] = hs_ra_upper(win[end - w0 + k]);
    d.out_len[L.var_off + i] = at;
  }
  __syncthreads();
  // ---- the order (:673-689): allele 0 first, the rest by (length, bytes); two equal strings are refused
  const int len0 = d.out_len[L.var_off];
  bool dup = false;
  for (int i = lane; i < V; i += HS_RA_WAVE){
    const int ni = d.out_len[L.var_off + i];
    const char* si = pool + (int64_t)i*L.stride;
    int r = i == 0 ? 0 : 1;
    for (int j = 0; j < V; j++){
      if (j == i) continue;
      const int c = hs_ra_order(pool + (int64_t)j*L.stride, d.out_len[L.var_off + j], si, ni);
      if (c == 0) dup = true;
      if (c < 0 && i >= 1 && j >= 1) r++;
    }
    d.old_to_new[L.var_off + i] = r;
    d.bp_diff[L.var_off + i] = ni - len0;
  }
  if (__any(dup)){
    if (lane == 0){ scal[0] = HS_RA_DUPLICATE; scal[1] = 0; scal[2] = 0; scal[3] = 0; }
    return;
  }
  for (int i = lane; i < V; i += HS_RA_WAVE) d.new_to_old[L.var_off + d.old_to_new[L.var_off + i]] = i;
  if (lane == 0){ scal[0] = 0; scal[1] = (int32_t)pos; scal[2] = (int32_t)(lt - lf - pad); scal[3] = (int32_t)(rt - rf); }
}

// ---------------------------------------------------------------------------------------------------------------- host side
namespace {
bool null_call(const hipstr_batch_t* b, const hipstr_record_alleles_request_t* rq, const hipstr_record_alleles_out_t* out){
  if (!b || !rq || !out || b->n_loci < 0 || !b->opt_off || !rq->win_off || !out->allele_off) return true;
  if (b->n_loci && (!b->blk_start || !b->blk_end || !b->blk_nopts || !b->seq || !rq->region_start || !rq->region_stop || !rq->window ||
                    !out->status || !out->pos || !out->left_trim || !out->right_trim || !out->alleles || !out->allele_bp_diff || !out->old_to_new || !out->new_to_old))
    return true;
  return (out->lflank_off && !out->lflanks) || (out->rflank_off && !out->rflanks);
}
void host_locus(const hipstr_batch_t* b, const hipstr_record_alleles_request_t* rq, int l, int64_t opt_base, ra::Locus* L){
  ra::alleles_of(ra::block_options(b, opt_base, l, 1), b->blk_start[3*l + 1], b->blk_end[3*l + 1], rq->region_start[l], rq->region_stop[l],
                 rq->window + rq->win_off[l], rq->win_off[l + 1] - rq->win_off[l], L);
}
thread_local int64_t g_last[4];       // of the calling thread's last device call: loci, done by the host twin, bytes up, bytes home
}  // namespace

extern "C" int hipstr_record_alleles_host(const hipstr_batch_t* b, const hipstr_record_alleles_request_t* rq, hipstr_record_alleles_out_t* out){
  if (null_call(b, rq, out)) return api_fail("null argument");
  int64_t nv;
  std::string why = ra::check(b, rq, out, &nv);
  if (!why.empty()) return api_fail("hipstr_record_alleles: " + why);
  std::vector<ra::Locus> loci((size_t)b->n_loci);
  int64_t ob = 0;
  for (int l = 0; l < b->n_loci; l++){ host_locus(b, rq, l, ob, &loci[(size_t)l]); ob += b->blk_nopts[3*l] + b->blk_nopts[3*l + 1] + b->blk_nopts[3*l + 2]; }
  why = ra::emit(b, loci, out);
  return why.empty() ? 0 : api_fail("hipstr_record_alleles: " + why);
}

extern "C" int hipstr_record_alleles(const hipstr_batch_t* b, const hipstr_record_alleles_request_t* rq, hipstr_record_alleles_out_t* out){
  if (null_call(b, rq, out)) return api_fail("null argument");
  int64_t nv64;
  std::string why = ra::check(b, rq, out, &nv64);
  if (!why.empty()) return api_fail("hipstr_record_alleles: " + why);
  for (int i = 0; i < 4; i++) g_last[i] = 0;
  const int nl = b->n_loci;
  std::vector<ra::Locus> res((size_t)nl);
  if (nl == 0){ why = ra::emit(b, res, out); return why.empty() ? 0 : api_fail("hipstr_record_alleles: " + why); }
  const size_t nv = (size_t)nv64;
  // the loci's table; the pool's pieces
  std::vector<hs_ra_locus_t> loci((size_t)nl);
  std::vector<int64_t> opt_base((size_t)nl);
  int64_t ob = 0, vo = 0, pool = 0, n_host = 0;
  for (int l = 0; l < nl; l++){
    hs_ra_locus_t& L = loci[(size_t)l]; memset(&L, 0, sizeof L);
    opt_base[(size_t)l] = ob;
    L.opt0 = (int32_t)(ob + b->blk_nopts[3*l]); L.n_opts = b->blk_nopts[3*l + 1];
    L.start = b->blk_start[3*l + 1]; L.end = b->blk_end[3*l + 1]; L.region_start = rq->region_start[l]; L.region_stop = rq->region_stop[l];
    L.win_base = rq->win_off[l]; L.win_len = rq->win_off[l + 1] - rq->win_off[l]; L.var_off = (int32_t)vo;
    int longest = 0;
    for (int i = 0; i < L.n_opts; i++) longest = std::max(longest, b->opt_off[L.opt0 + i + 1] - b->opt_off[L.opt0 + i]);
    const int64_t stride = (int64_t)longest + 2*(int64_t)L.win_len + 1;
    L.on_host = (L.n_opts > HS_RA_MAX_OPTIONS || stride > INT32_MAX/2) ? 1 : 0;
    if (L.on_host) n_host++;
    else { L.pool_base = pool; L.stride = (int32_t)stride; pool += stride*L.n_opts; }
    ob += b->blk_nopts[3*l] + b->blk_nopts[3*l + 1] + b->blk_nopts[3*l + 2]; vo += L.n_opts;
  }
  const size_t n_opts = (size_t)ob, n_seq = (size_t)b->opt_off[n_opts], n_win = (size_t)rq->win_off[nl];
  if (n_host < nl){
    hipstr::ApiTables A;
    if (hipstr::api_device_tables(&A)) return 1;
    hipStream_t st = A.stream;
    hipstr::HostArena ar;
    hs_ra_dev_t h; memset(&h, 0, sizeof h);
    const size_t o_loci = ar.add(loci.data(), loci.size()*sizeof(hs_ra_locus_t)), o_off = ar.add(b->opt_off, (n_opts + 1)*4), o_seq = ar.add(b->seq, n_seq),
                 o_win = ar.add(rq->window, n_win), o_args = ar.add(&h, sizeof h);
    if (ar.reserve(A.ctx)) return 1;
    hipstr::ResultBlocks B;
    const size_t r_scal = B.take((size_t)nl*16), r_len = B.take(nv*4), r_bp = B.take(nv*4), r_o2n = B.take(nv*4), r_n2o = B.take(nv*4), r_pool = B.take((size_t)pool);
    B.end_results();
    if (B.reserve(A.ctx, st)) return 1;
    h.loci = ar.at<hs_ra_locus_t>(o_loci); h.opt_off = ar.at<int32_t>(o_off); h.seq = ar.at<char>(o_seq); h.window = ar.at<char>(o_win);
    h.scal = B.dev<int32_t>(r_scal); h.out_len = B.dev<int32_t>(r_len); h.bp_diff = B.dev<int32_t>(r_bp); h.old_to_new = B.dev<int32_t>(r_o2n);
    h.new_to_old = B.dev<int32_t>(r_n2o); h.pool = B.dev<char>(r_pool); h.n_loci = nl;
    if (ar.send(st)) return 1;
    hipLaunchKernelGGL(hs_ra_kernel, dim3((unsigned)nl), dim3(HS_RA_WAVE), 0, st, ar.at<hs_ra_dev_t>(o_args));
    HS_HIP(hipGetLastError());
    if (B.fetch()) return 1;
    const int32_t* scal = B.host<int32_t>(r_scal); const int32_t* len = B.host<int32_t>(r_len);
    for (int l = 0; l < nl; l++){
      const hs_ra_locus_t& L = loci[(size_t)l];
      if (L.on_host) continue;
      ra::Locus& R = res[(size_t)l];
      R.status = scal[4*l]; R.pos = scal[4*l + 1]; R.left_trim = scal[4*l + 2]; R.right_trim = scal[4*l + 3];
      if (R.status != 0) continue;
      const size_t V = (size_t)L.n_opts;
      R.alleles.resize(V);
      for (size_t i = 0; i < V; i++){
        const int32_t n = len[L.var_off + (int32_t)i];
        if (n < 0 || n > L.stride) return api_fail("hipstr_record_alleles: the device's allele length is outside its piece");
        R.alleles[i].assign(B.host<char>(r_pool) + L.pool_base + (int64_t)i*L.stride, (size_t)n);
      }
      R.bp_diff.assign(B.host<int32_t>(r_bp) + L.var_off, B.host<int32_t>(r_bp) + L.var_off + V);
      R.old_to_new.assign(B.host<int32_t>(r_o2n) + L.var_off, B.host<int32_t>(r_o2n) + L.var_off + V);
      R.new_to_old.assign(B.host<int32_t>(r_n2o) + L.var_off, B.host<int32_t>(r_n2o) + L.var_off + V);
    }
    g_last[2] = (int64_t)ar.total; g_last[3] = (int64_t)B.res;
  }
  for (int l = 0; l < nl; l++) if (loci[(size_t)l].on_host) host_locus(b, rq, l, opt_base[(size_t)l], &res[(size_t)l]);
  g_last[0] = nl; g_last[1] = n_host;
  why = ra::emit(b, res, out);
  return why.empty() ? 0 : api_fail("hipstr_record_alleles: " + why);
}

#ifndef HIPSTR_NO_DEBUG_ABI
// the calling thread's last hipstr_record_alleles: out[0] loci, out[1] done by the host twin, out[2] bytes up, out[3] bytes home
extern "C" int hipstr_debug_record_alleles_last(int64_t out[4]){
  if (!out) return api_fail("null argument");
  for (int i = 0; i < 4; i++) out[i] = g_last[i];
  return 0;
}
#endif
