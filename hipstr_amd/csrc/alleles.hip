// alleles.hip — the allele-set update between two genotype() rounds on gfx950: add_and_remove_alleles (seq_stutter_genotyper.cpp:330-369)
// for a batch of loci (include/hipstr_hmm.h: hipstr_alleles_apply, hipstr_alleles_step).  The host computes counts and offsets
// (alleles_host.cpp: plan); one workgroup per locus does the strings:
//
//   hs_alleles_kernel   1  a wavefront per option, old and new: every lane folds its run of the bytes into (hash, B^length), the lanes' pairs
//                          are folded in order across the wavefront; a new option's bytes are written to the new seq on the way
//                       2  a thread per old haplotype: its key (hash, total length) from its three options in O(1), into the LDS table:
//                          the first haplotype of a key claims the slot (atomicCAS), the highest index is the slot's value (atomicMax)
//                       3  a thread per new haplotype: its options (hap_to_allele), its key, the lookup; realign_hap, and the mapping of
//                          the slot's value by atomicMax (the last new haplotype of a key wins)
//                       4  the mapping and the two counts go out
// The hash only filters: "is this slot my key?" is answered, in 2 and 3 alike, by the bytes of the two haplotypes walked through their
// options (hs_alleles_equal).  Integer work throughout: device and host form agree bit for bit.  No kernel waits on memory, no workgroup talks
// to another, every loop has a bound taken from the uploaded tables or from alleles_layout.h.  A locus beyond a limit of alleles_layout.h is
// done by the host code in the same call.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <string>
#include <vector>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "alleles_host.h"
#include "alleles_layout.h"
#include "api_internal.h"

namespace {

#define AL_NT HS_ALLELES_THREADS
#define AL_NEW HS_ALLELES_MAX_OPTS     // where the new options start in the per-option LDS arrays

// ------------------------------------------------------------------------------------------------------------------------ kernel
struct AlSide { int n0, n1, n2, base; };       // a side's option counts and where its options start in the LDS arrays

__device__ __forceinline__ void al_hap(const AlSide& s, int k, int* e0, int* e1, int* e2){
  int o0, o1, o2;
  hs_alleles_digits(s.n0, s.n1, s.n2, k, &o0, &o1, &o2);
  *e0 = s.base + o0; *e1 = s.base + s.n0 + o1; *e2 = s.base + s.n0 + s.n1 + o2;
}

extern "C" __global__ void __launch_bounds__(AL_NT) hs_alleles_kernel(const hs_alleles_dev_t d){
  __shared__ uint64_t s_h[2*HS_ALLELES_MAX_OPTS], s_pw[2*HS_ALLELES_MAX_OPTS];
  __shared__ int32_t s_len[2*HS_ALLELES_MAX_OPTS];
  __shared__ int32_t s_lead[HS_ALLELES_SLOTS], s_val[HS_ALLELES_SLOTS];
  __shared__ int32_t s_map[HS_ALLELES_MAX_HAPS];
  __shared__ unsigned int s_cnt[2];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lc = blockIdx.x;
  const int32_t* no = d.nopts + 6*lc;
  const AlSide O = { no[0], no[1], no[2], 0 }, N = { no[3], no[4], no[5], AL_NEW };
  const int NO = O.n0 + O.n1 + O.n2, NN = N.n0 + N.n1 + N.n2;
  const int ob = d.l_oopt[lc], nb = d.l_nopt[lc];
  const int oh0 = d.l_ohap[lc], A_old = d.l_ohap[lc+1] - oh0, nh0 = d.l_nhap[lc], A_new = d.l_nhap[lc+1] - nh0;
  if (NO > HS_ALLELES_MAX_OPTS || NN > HS_ALLELES_MAX_OPTS || A_old > HS_ALLELES_MAX_HAPS || A_new > HS_ALLELES_MAX_HAPS) return;      // (the host sends no such locus)

  // ---- 1: an empty table; the options' hashes, the new options' bytes
  for (int i = t; i < HS_ALLELES_SLOTS; i += AL_NT){ s_lead[i] = -1; s_val[i] = -1; }
  for (int i = t; i < A_old; i += AL_NT) s_map[i] = -1;
  if (t < 2) s_cnt[t] = 0;
  for (int e = wave; e < NO + NN; e += AL_NT/64){
    const char* p; char* dst = NULL; int len, at;
    if (e < NO){ const int a = d.o_off[ob + e]; p = d.old_seq + a; len = d.o_off[ob + e + 1] - a; at = e; }
    else {
      const int j = e - NO, src = d.n_src[nb + j], a = d.n_off[nb + j];
      p = src >= 0 ? d.old_seq + src : d.add_seq + (-1 - src); len = d.n_off[nb + j + 1] - a; dst = d.new_seq + a; at = AL_NEW + j;
    }
    const int run = (len + 63) >> 6, i0 = min(lane*run, len), i1 = min(i0 + run, len);
    uint64_t h = 0, pw = 1;
    for (int i = i0; i < i1; i++){ const char c = p[i]; if (dst) dst[i] = c; h = hs_alleles_hash_step(h, c); pw *= HS_ALLELES_BASE; }
    for (int dlt = 1; dlt < 64; dlt <<= 1){                           // lane 0 ends with the lanes' pieces folded in order
      const uint64_t h_next = __shfl_down((unsigned long long)h, dlt), pw_next = __shfl_down((unsigned long long)pw, dlt);
      if (lane + dlt < 64){ h = h*pw_next + h_next; pw *= pw_next; }
    }
    if (lane == 0){ s_h[at] = h; s_pw[at] = pw; s_len[at] = len; }
  }
  __syncthreads();

  unsigned int probes = 0, compares = 0;
  // ---- 2: the old haplotypes into the table
  for (int i = t; i < A_old; i += AL_NT){
    int e0, e1, e2; al_hap(O, i, &e0, &e1, &e2);
    const uint64_t h = hs_alleles_hap_hash(s_h[e0], s_h[e1], s_pw[e1], s_h[e2], s_pw[e2], d.hash_bits);
    const int tl = s_len[e0] + s_len[e1] + s_len[e2];
    uint32_t s = hs_alleles_slot(h, tl, HS_ALLELES_SLOTS);
    for (int probe = 0; probe < HS_ALLELES_SLOTS; probe++, s = (s + 1) & (HS_ALLELES_SLOTS - 1)){
      probes++;
      const int prev = atomicCAS(&s_lead[s], -1, i);
      if (prev == -1){ atomicMax(&s_val[s], i); break; }
      int q0, q1, q2; al_hap(O, prev, &q0, &q1, &q2);
      if (hs_alleles_hap_hash(s_h[q0], s_h[q1], s_pw[q1], s_h[q2], s_pw[q2], d.hash_bits) != h || s_len[q0] + s_len[q1] + s_len[q2] != tl) continue;
      compares++;
      if (hs_alleles_equal(d.old_seq + d.o_off[ob + e0], s_len[e0], d.old_seq + d.o_off[ob + e1], s_len[e1], d.old_seq + d.o_off[ob + e2], s_len[e2],
                           d.old_seq + d.o_off[ob + q0], s_len[q0], d.old_seq + d.o_off[ob + q1], s_len[q1], d.old_seq + d.o_off[ob + q2], s_len[q2])){
        atomicMax(&s_val[s], i); break;
      }
    }
  }
  __syncthreads();
  // ---- 3: the new haplotypes, looked up
  for (int j = t; j < A_new; j += AL_NT){
    int e0, e1, e2; al_hap(N, j, &e0, &e1, &e2);
    int32_t* rows = d.h2a + 3*(size_t)nh0;
    rows[j] = e0 - AL_NEW; rows[A_new + j] = e1 - AL_NEW - N.n0; rows[2*A_new + j] = e2 - AL_NEW - N.n0 - N.n1;
    const uint64_t h = hs_alleles_hap_hash(s_h[e0], s_h[e1], s_pw[e1], s_h[e2], s_pw[e2], d.hash_bits);
    const int tl = s_len[e0] + s_len[e1] + s_len[e2];
    const int c0 = d.n_src[nb + e0 - AL_NEW], c1 = d.n_src[nb + e1 - AL_NEW], c2 = d.n_src[nb + e2 - AL_NEW];       // (the sources: nothing this kernel wrote is read)
    const char* p0 = c0 >= 0 ? d.old_seq + c0 : d.add_seq + (-1 - c0);
    const char* p1 = c1 >= 0 ? d.old_seq + c1 : d.add_seq + (-1 - c1);
    const char* p2 = c2 >= 0 ? d.old_seq + c2 : d.add_seq + (-1 - c2);
    uint8_t realign = 1;
    uint32_t s = hs_alleles_slot(h, tl, HS_ALLELES_SLOTS);
    for (int probe = 0; probe < HS_ALLELES_SLOTS; probe++, s = (s + 1) & (HS_ALLELES_SLOTS - 1)){
      probes++;
      const int L = s_lead[s];
      if (L < 0) break;
      int q0, q1, q2; al_hap(O, L, &q0, &q1, &q2);
      if (hs_alleles_hap_hash(s_h[q0], s_h[q1], s_pw[q1], s_h[q2], s_pw[q2], d.hash_bits) != h || s_len[q0] + s_len[q1] + s_len[q2] != tl) continue;
      compares++;
      if (hs_alleles_equal(p0, s_len[e0], p1, s_len[e1], p2, s_len[e2],
                           d.old_seq + d.o_off[ob + q0], s_len[q0], d.old_seq + d.o_off[ob + q1], s_len[q1], d.old_seq + d.o_off[ob + q2], s_len[q2])){
        realign = 0; atomicMax(&s_map[s_val[s]], j); break;
      }
    }
    d.realign[nh0 + j] = realign;
  }
  atomicAdd(&s_cnt[0], probes); atomicAdd(&s_cnt[1], compares);
  __syncthreads();
  // ---- 4
  for (int i = t; i < A_old; i += AL_NT) d.mapping[oh0 + i] = s_map[i];
  if (t < 2) d.counts[2*lc + t] = (int32_t)s_cnt[t];
}
static_assert(HS_ALLELES_SLOTS >= 2*HS_ALLELES_MAX_HAPS && (HS_ALLELES_SLOTS & (HS_ALLELES_SLOTS - 1)) == 0, "the table stays at most half full");
static_assert(HS_ALLELES_LDS_BYTES <= 65536, "the workgroup's LDS is static");

// ------------------------------------------------------------------------------------------------------------------------ host side
using hipstr::api_fail;

thread_local hipstr::ChunkLast t_last;
std::atomic<int> g_hash_bits{64};

int64_t alleles_ws_bytes(){ return hipstr::chunk_budget(0.0, "HIPSTR_ALLELES_WS_MIB", (double)HS_ALLELES_WS_MIB, (double)HS_ALLELES_MAX_CHUNK_BYTES); }

// the loci of [l0, l1) that go to the device, as one chunk
int alleles_chunk(hipstr::Ctx* ctx, hipStream_t st, const hipstr_al::Plan& P, hipstr_alleles& a, const std::vector<uint8_t>& dev, int l0, int l1,
                  int hash_bits, bool timing, hipstr::ChunkLast& last){
  const hipstr_batch_t* b = P.b;
  std::vector<int> loci;
  for (int l = l0; l < l1; l++) if (dev[l]) loci.push_back(l);
  const size_t NL = loci.size();
  if (!NL) return 0;
  int64_t n_oo = 0, n_no = 0, n_oh = 0, n_nh = 0, B_old = 0, B_add = 0, B_new = 0;
  for (int l : loci){
    n_oo += P.o_opt0[l+1] - P.o_opt0[l]; n_no += P.n_opt0[l+1] - P.n_opt0[l];
    n_oh += b->hap_off[l+1] - b->hap_off[l]; n_nh += a.new_n[l];
    B_old += b->opt_off[P.o_opt0[l+1]] - b->opt_off[P.o_opt0[l]];
    B_new += a.opt_off[P.n_opt0[l+1]] - a.opt_off[P.n_opt0[l]];
    for (int o = P.n_opt0[l]; o < P.n_opt0[l+1]; o++) if (P.n_src[o] < 0) B_add += a.opt_off[o+1] - a.opt_off[o];
  }
  if (B_old > INT32_MAX || B_add > INT32_MAX || B_new > INT32_MAX || 3*n_nh > INT32_MAX) return api_fail("hipstr_alleles_apply: a chunk of more than 2^31 bytes (lower HIPSTR_ALLELES_WS_MIB)");
  hipstr::ChunkBlocks K(ctx, st);
  // uploaded | results
  const size_t u_nopts = K.take(NL*24), u_loo = K.take((NL + 1)*4), u_lno = K.take((NL + 1)*4), u_loh = K.take((NL + 1)*4), u_lnh = K.take((NL + 1)*4),
               u_ooff = K.take((size_t)(n_oo + 1)*4), u_noff = K.take((size_t)(n_no + 1)*4), u_nsrc = K.take((size_t)n_no*4), u_old = K.take((size_t)B_old),
               u_add = K.take((size_t)B_add);
  K.end_upload();
  K.begin_results();
  const size_t o_map = K.take((size_t)n_oh*4), o_h2a = K.take((size_t)n_nh*12), o_cnt = K.take(NL*8), o_re = K.take((size_t)n_nh), o_seq = K.take((size_t)B_new);
  if (K.reserve()) return 1;
  {
    int32_t* h_nopts = K.up<int32_t>(u_nopts), *h_loo = K.up<int32_t>(u_loo), *h_lno = K.up<int32_t>(u_lno), *h_loh = K.up<int32_t>(u_loh), *h_lnh = K.up<int32_t>(u_lnh),
           * h_ooff = K.up<int32_t>(u_ooff), *h_noff = K.up<int32_t>(u_noff), *h_nsrc = K.up<int32_t>(u_nsrc);
    char* h_old = K.up<char>(u_old), *h_add = K.up<char>(u_add);
    int32_t oo = 0, no = 0, oh = 0, nh = 0, bo = 0, ba = 0, bn = 0;
    for (size_t lc = 0; lc < NL; lc++){
      const int l = loci[lc];
      for (int k = 0; k < 3; k++){ h_nopts[6*lc + k] = b->blk_nopts[3*l + k]; h_nopts[6*lc + 3 + k] = a.blk_nopts[(size_t)3*l + k]; }
      h_loo[lc] = oo; h_lno[lc] = no; h_loh[lc] = oh; h_lnh[lc] = nh;
      const int32_t s0 = b->opt_off[P.o_opt0[l]], s1 = b->opt_off[P.o_opt0[l+1]];
      for (int o = P.o_opt0[l]; o < P.o_opt0[l+1]; o++) h_ooff[oo++] = bo + (b->opt_off[o] - s0);
      if (s1 > s0) memcpy(h_old + bo, b->seq + s0, (size_t)(s1 - s0));
      const int32_t q0 = a.opt_off[P.n_opt0[l]];
      for (int o = P.n_opt0[l]; o < P.n_opt0[l+1]; o++){
        const int32_t src = P.n_src[o], len = a.opt_off[(size_t)o+1] - a.opt_off[o];
        h_noff[no] = bn + (a.opt_off[o] - q0);
        if (src >= 0) h_nsrc[no] = bo + (src - s0);
        else { h_nsrc[no] = -1 - ba; if (len) memcpy(h_add + ba, P.rq->add_seq + (-1 - src), (size_t)len); ba += len; }
        no++;
      }
      bo += s1 - s0; bn += a.opt_off[P.n_opt0[l+1]] - q0;
      oh += b->hap_off[l+1] - b->hap_off[l]; nh += a.new_n[l];
    }
    h_loo[NL] = oo; h_lno[NL] = no; h_loh[NL] = oh; h_lnh[NL] = nh; h_ooff[oo] = bo; h_noff[no] = bn;
  }
  hs_alleles_dev_t d; memset(&d, 0, sizeof d);
  char* D = K.dev;
  d.nopts = (const int32_t*)(D + u_nopts); d.l_oopt = (const int32_t*)(D + u_loo); d.l_nopt = (const int32_t*)(D + u_lno); d.l_ohap = (const int32_t*)(D + u_loh);
  d.l_nhap = (const int32_t*)(D + u_lnh); d.o_off = (const int32_t*)(D + u_ooff); d.n_off = (const int32_t*)(D + u_noff); d.n_src = (const int32_t*)(D + u_nsrc);
  d.old_seq = D + u_old; d.add_seq = D + u_add;
  d.mapping = (int32_t*)(D + o_map); d.h2a = (int32_t*)(D + o_h2a); d.counts = (int32_t*)(D + o_cnt); d.realign = (uint8_t*)(D + o_re); d.new_seq = D + o_seq;
  d.nl = (int32_t)NL; d.hash_bits = hash_bits;
  if (K.upload(timing)) return 1;
  hipLaunchKernelGGL(hs_alleles_kernel, dim3((unsigned)NL), dim3(AL_NT), 0, st, d);
  HS_HIP(hipGetLastError());
  if (K.fetch(timing, &last.t[0])) return 1;
  last.t[1] += (double)K.up_bytes; last.t[2] += (double)K.res_bytes(); last.v[5]++;
  // ---- home: every piece to its place in the result
  const int32_t* r_map = K.host<int32_t>(o_map), *r_h2a = K.host<int32_t>(o_h2a), *r_cnt = K.host<int32_t>(o_cnt);
  const uint8_t* r_re = K.host<uint8_t>(o_re); const char* r_seq = K.host<char>(o_seq);
  int64_t oh = 0, nh = 0, bn = 0;
  for (size_t lc = 0; lc < NL; lc++){
    const int l = loci[lc];
    const int A_old = b->hap_off[l+1] - b->hap_off[l], A_new = a.new_n[l];
    const int32_t q0 = a.opt_off[P.n_opt0[l]], q1 = a.opt_off[P.n_opt0[l+1]];
    if (A_old) memcpy(a.mapping.data() + b->hap_off[l], r_map + oh, (size_t)A_old*4);
    for (int k = 0; k < 3; k++) memcpy(a.h2a[k].data() + a.hap_off[l], r_h2a + 3*nh + (int64_t)k*A_new, (size_t)A_new*4);
    memcpy(a.realign.data() + a.hap_off[l], r_re + nh, (size_t)A_new);
    if (q1 > q0) memcpy(a.seq.data() + q0, r_seq + bn, (size_t)(q1 - q0));
    last.v[2] += (uint32_t)r_cnt[2*lc]; last.v[3] += (uint32_t)r_cnt[2*lc + 1];
    oh += A_old; nh += A_new; bn += q1 - q0;
  }
  return 0;
}

hipstr_alleles_t* alleles_device(const hipstr_alleles_request_t* rq, const char* who){
  hipstr_al::Plan P; std::string err;
  hipstr_alleles* a = new hipstr_alleles;
  if (hipstr_al::plan(rq, P, *a, err)){ delete a; api_fail(std::string(who) + ": " + err); return NULL; }
  hipstr::Ctx* ctx = hipstr::api_current_ctx();
  if (!ctx || hipstr::api_bind(ctx)){ delete a; return NULL; }
  hipStream_t st = hipstr::ctx_stream(ctx);
  hipstr::ChunkLast last;
  t_last = last;                                  // a call that fails on the way reports zeros, not the call before it
  const int hash_bits = g_hash_bits.load();
  const bool timing = getenv("HIPSTR_ALLELES_TIMING") != NULL;
  const int64_t budget = alleles_ws_bytes();
  const hipstr_batch_t* b = P.b;
  const int nl = P.nl;
  std::vector<uint8_t> dev((size_t)nl, 0); std::vector<int64_t> cost((size_t)nl, 0);
  for (int l = 0; l < nl; l++){
    if (!P.on[l]) continue;
    const int64_t oo = P.o_opt0[l+1] - P.o_opt0[l], no = P.n_opt0[l+1] - P.n_opt0[l], oh = b->hap_off[l+1] - b->hap_off[l], nh = a->new_n[l];
    const int64_t so = b->opt_off[P.o_opt0[l+1]] - b->opt_off[P.o_opt0[l]], sn = a->opt_off[P.n_opt0[l+1]] - a->opt_off[P.n_opt0[l]];
    const int64_t bytes = hs_alleles_locus_bytes(oh, nh, oo, no, so, sn, sn);      // (the adds are part of the new strings)
    dev[l] = hs_alleles_on_device(oh, nh, oo, no, bytes) ? 1 : 0;
    cost[l] = dev[l] ? bytes : 0;
  }
  for (int l0 = 0; l0 < nl; ){
    const int l1 = hs_pool_chunk_end(cost.data(), l0, nl, budget);
    if (alleles_chunk(ctx, st, P, *a, dev, l0, l1, hash_bits, timing, last)){ delete a; return NULL; }
    for (int l = l0; l < l1; l++){
      if (dev[l]){ last.v[0]++; continue; }
      hipstr_al::gather_locus(P, l, *a);
      if (!P.on[l]){ hipstr_al::identity_locus(P, l, *a); last.v[4]++; continue; }
      int64_t c[2] = {0, 0};
      hipstr_al::map_locus(P, l, *a, hash_bits, c);
      last.v[1]++; last.v[2] += c[0]; last.v[3] += c[1];
    }
    l0 = l1;
  }
  hipstr_al::finish(P, *a);
  t_last = last;
  return a;
}

hipstr_alleles_t* alleles_host(const hipstr_alleles_request_t* rq, const char* who){
  std::string err; int64_t c[4] = {0, 0, 0, 0};
  hipstr_alleles* a = hipstr_al::apply_host(rq, g_hash_bits.load(), c, err);
  if (!a){ api_fail(std::string(who) + ": " + err); return NULL; }
  hipstr::ChunkLast last;
  for (int i = 0; i < 4; i++) last.v[i] = c[i];
  t_last = last;
  return a;
}

}  // namespace

extern "C" hipstr_alleles_t* hipstr_alleles_apply(const hipstr_alleles_request_t* rq){ return alleles_device(rq, "hipstr_alleles_apply"); }
extern "C" hipstr_alleles_t* hipstr_alleles_apply_host(const hipstr_alleles_request_t* rq){ return alleles_host(rq, "hipstr_alleles_apply_host"); }
extern "C" const hipstr_batch_t* hipstr_alleles_batch(const hipstr_alleles_t* a){ return a ? &a->batch : NULL; }
extern "C" const hipstr_batch_t* hipstr_alleles_batch_all(const hipstr_alleles_t* a){ return a ? &a->batch_all : NULL; }
extern "C" const int32_t* hipstr_alleles_mapping(const hipstr_alleles_t* a){ return a ? a->mapping.data() : NULL; }
extern "C" const int32_t* hipstr_alleles_new_n_alleles(const hipstr_alleles_t* a){ return a ? a->new_n.data() : NULL; }
extern "C" const int32_t* hipstr_alleles_hap_to_allele(const hipstr_alleles_t* a, int block){ return (a && block >= 0 && block < 3) ? a->h2a[block].data() : NULL; }
extern "C" const uint8_t* hipstr_alleles_added(const hipstr_alleles_t* a){ return a ? a->added.data() : NULL; }
extern "C" void hipstr_alleles_free(hipstr_alleles_t* a){ delete a; }

extern "C" hipstr_alleles_t* hipstr_alleles_step(const hipstr_batch_t* pooled, const hipstr_census_out_t* census, int32_t* phase, int32_t max_total_haplotypes,
                                                 uint32_t flags, hipstr_alleles_step_out_t* out){
  if (!out || !phase){ api_fail("hipstr_alleles_step: null argument"); return NULL; }
  if (flags & ~(uint32_t)HIPSTR_ALLELES_ON_HOST){ api_fail("hipstr_alleles_step: unknown flag"); return NULL; }
  if (pooled && pooled->n_loci > 0 && (!out->status || !out->n_added || !out->n_removed || !out->n_affected_blocks)){ api_fail("hipstr_alleles_step: null output array"); return NULL; }
  hipstr_al::Step S; std::string err;
  if (hipstr_al::step_plan(pooled, census, phase, max_total_haplotypes, S, err)){ api_fail("hipstr_alleles_step: " + err); return NULL; }
  hipstr_alleles_t* a = (flags & HIPSTR_ALLELES_ON_HOST) ? alleles_host(&S.rq, "hipstr_alleles_step") : alleles_device(&S.rq, "hipstr_alleles_step");
  if (!a) return NULL;
  const size_t nl = (size_t)pooled->n_loci;
  if (nl){
    memcpy(phase, S.phase.data(), nl*4); memcpy(out->status, S.status.data(), nl*4); memcpy(out->n_added, S.n_added.data(), nl*4);
    memcpy(out->n_removed, S.n_removed.data(), nl*4); memcpy(out->n_affected_blocks, S.n_affected.data(), nl*4);
  }
  out->any_added = S.any_added;
  return a;
}

#ifndef HIPSTR_NO_DEBUG_ABI
extern "C" int hipstr_debug_alleles_hash_bits(int bits){
  if (bits < 0 || bits > 64) return api_fail("hipstr_debug_alleles_hash_bits: bits outside 0..64");
  g_hash_bits.store(bits == 0 ? 64 : bits);
  return 0;
}
extern "C" int hipstr_debug_alleles_last(int64_t out[8]){
  if (!out) return api_fail("hipstr_debug_alleles_last: null argument");
  memcpy(out, t_last.v, sizeof t_last.v);
  return 0;
}
extern "C" int hipstr_debug_alleles_last_timing(double out[4]){
  if (!out) return api_fail("hipstr_debug_alleles_last_timing: null argument");
  memcpy(out, t_last.t, sizeof t_last.t);
  return 0;
}
extern "C" int hipstr_debug_alleles_limits(int64_t out[4]){
  if (!out) return api_fail("hipstr_debug_alleles_limits: null argument");
  out[0] = HS_ALLELES_THREADS; out[1] = HS_ALLELES_MAX_HAPS; out[2] = HS_ALLELES_MAX_OPTS; out[3] = HS_ALLELES_SLOTS;
  return 0;
}
#endif  // HIPSTR_NO_DEBUG_ABI
