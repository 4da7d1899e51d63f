// record.hip — the numeric fields of a VCF record on the device: hipstr_bias_pvalues and hipstr_record_fields (include/hipstr_hmm.h) with
// their host forms.  One lane per (locus, sample) runs the two serial recurrences behind AB and FS — cephes' continued fraction for the
// incomplete beta integral and the tail sums of htslib's Fisher test (record_layout.h: the lane's body) — and decides the sample's filter;
// the INFO counts of a locus are integer sums over its lanes.
//
// Shape of the launch: a workgroup is ONE wavefront of up to 64 consecutive samples of one locus, taken as they come (no sorting).  The
// lanes of a wavefront diverge by the length of their loops — the Fisher tails grow with the sample's read count, the continued fraction
// stops after 10-300 terms — so a wavefront costs what its deepest sample costs; samples of one locus share the locus' coverage, which is
// the similarity that can be had without reordering.  Single-wavefront workgroups keep that cost from spreading over four wavefronts and
// let the scheduler fill a CU with whatever is ready.  The lane's state is a dozen doubles: occupancy is not the limit, the serial
// double-precision chains are.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "api_internal.h"
#include "record_host.h"
#include "record_layout.h"

using hipstr::api_fail;
namespace hr = hipstr_record;

// ---------------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(HS_REC_THREADS) void hs_rec_pvalues_kernel(const hs_rec_pv_dev_t* __restrict__ args){
  const hs_rec_pv_dev_t d = *args;
  const int64_t i = (int64_t)blockIdx.x*HS_REC_THREADS + threadIdx.x;
  if (i >= d.n) return;
  const int u1 = d.u1[i], u2 = d.u2[i], r1 = d.rv1[i], r2 = d.rv2[i];
  if ((int64_t)u1 + u2 > HS_REC_TABLE_READS) return;          // beyond the table: the host fills it in
  d.ab[i] = hs_rec_allele_bias(d.table, u1, u2);
  d.fs[i] = hs_rec_strand_bias(d.table, u1, r1, u2, r2);
}

__global__ __launch_bounds__(HS_REC_THREADS) void hs_rec_fields_kernel(const hs_rec_dev_t* __restrict__ args){
  const hs_rec_dev_t d = *args;
  __shared__ int32_t acc[7];
  const int lane = threadIdx.x;
  if (lane < 7) acc[lane] = 0;
  __syncthreads();
  const int l = d.group_locus[blockIdx.x];
  const hs_rec_locus_t L = d.loci[l];
  const int i = ((int)blockIdx.x - L.first_group)*HS_REC_THREADS + lane;
  if (i < L.n_samples){
    const int64_t s = (int64_t)L.samp_off + i;
    const int32_t na = d.counts[0][s], nsnp = d.counts[1][s], nst = d.counts[2][s], nfi = d.counts[3][s];
    const int32_t u1 = d.counts[4][s], u2 = d.counts[5][s], r1 = d.counts[6][s], r2 = d.counts[7][s];
    int ha = d.map_gt[2*s], hb = d.map_gt[2*s + 1];
    // The three refusals below mirror hipstr_record::fields.  A posterior run never leaves such pairs (its MAP pair is in range, present for
    // a sample with reads, and homozygous at a haploid locus), so no GPU test reaches them: the host form's tests are their only cover.
    int err = 0;
    if (ha < -1 || ha >= L.n_alleles || hb < -1 || hb >= L.n_alleles || (ha < 0) != (hb < 0)){ err |= HS_REC_ERR_MAP_RANGE; ha = hb = -1; }
    const int g0 = ha < 0 ? -1 : d.hap_to_allele[L.hap_off + ha], g1 = hb < 0 ? -1 : d.hap_to_allele[L.hap_off + hb];
    const bool reported = !d.reported || d.reported[s], masked = d.masked && d.masked[s];
    const float rhs = d.frac*(float)na;
    const bool over = na > 0 && (float)nfi > rhs;
    const int status = !reported ? HIPSTR_RECORD_NOT_REPORTED : na == 0 ? HIPSTR_RECORD_NO_READS : masked ? HIPSTR_RECORD_MASKED :
                       over ? HIPSTR_RECORD_FLANK_INDEL_FRAC : HIPSTR_RECORD_PASS;
    // :1163-1187
    if (reported && na != 0){
      if (over) atomicAdd(&acc[1], 1);
      else if (masked) atomicAdd(&acc[0], 1);
      else if (ha < 0) err |= HS_REC_ERR_NO_PAIR;
      else if (L.haploid){
        if (g0 != g1) err |= HS_REC_ERR_HAPLOID_HET;
        else { atomicAdd(&d.allele_count[L.var_off + g0], 1); atomicAdd(&acc[2], 1); }
      } else { atomicAdd(&d.allele_count[L.var_off + g0], 1); atomicAdd(&d.allele_count[L.var_off + g1], 1); atomicAdd(&acc[2], 2); }
    }
    // :1238-1254
    if (reported && !masked && !over){ atomicAdd(&acc[3], na); atomicAdd(&acc[4], nsnp); atomicAdd(&acc[5], nst); atomicAdd(&acc[6], nfi); }
    if (err) atomicOr(d.error, err);
    d.status[s] = status; d.gt[2*s] = g0; d.gt[2*s + 1] = g1;
    // :1362-1375: the haplotypes differ, not the genotypes
    if (status == HIPSTR_RECORD_PASS && !L.haploid && ha != hb){
      d.dab[s] = u1 + u2;
      if ((int64_t)u1 + u2 <= HS_REC_TABLE_READS){          // (else the host fills both in)
        d.ab[s] = hs_rec_allele_bias(d.table, u1, u2);
        d.fs[s] = hs_rec_strand_bias(d.table, u1, r1, u2, r2);
      } else { d.ab[s] = 0.0; d.fs[s] = 0.0; }
    } else { d.ab[s] = HS_REC_NOT_APPLICABLE; d.fs[s] = HS_REC_NOT_APPLICABLE; d.dab[s] = 0; }
  }
  __syncthreads();
  if (lane < 7 && acc[lane] != 0) atomicAdd(&d.locus_out[(int64_t)lane*d.n_loci + l], acc[lane]);
}

// ---------------------------------------------------------------------------------------------------------------- host side
namespace {
// The table of a context (120 KB): filled by the host twin's own functions on the context's first call of this file, then the context's
// like its other constant tables (hipstr_hmm_shutdown frees it with them).  The only allocation of this file outside the caches.
int device_table(hipstr::Ctx* ctx, const double** out){
  return hipstr::ctx_record_table(ctx, 3*(size_t)HS_REC_TABLE_N, [](double* t){ hr::fill_table(t, HS_REC_TABLE_N); }, out);
}

thread_local int64_t g_last[4];       // of the calling thread's last device call: lanes, computed by the host twin, bytes up, bytes home

int check_pvalues(int64_t n, const int32_t* u1, const int32_t* u2, const int32_t* r1, const int32_t* r2, double* ab, double* fs){
  if (n < 0) return api_fail("hipstr_bias_pvalues: n must not be negative");
  if (n > 0 && (!u1 || !u2 || !r1 || !r2 || !ab || !fs)) return api_fail("null argument");
  for (int64_t i = 0; i < n; i++){
    const std::string why = hr::check_counts(u1[i], u2[i], r1[i], r2[i]);
    if (!why.empty()) return api_fail("hipstr_bias_pvalues: " + why);
  }
  return 0;
}
}  // namespace

extern "C" int hipstr_bias_pvalues_host(int64_t n, const int32_t* u1, const int32_t* u2, const int32_t* r1, const int32_t* r2, double* ab, double* fs){
  if (check_pvalues(n, u1, u2, r1, r2, ab, fs)) return 1;
  for (int64_t i = 0; i < n; i++){ ab[i] = hr::allele_bias(u1[i], u2[i]); fs[i] = hr::strand_bias(u1[i], r1[i], u2[i], r2[i]); }
  return 0;
}

extern "C" int hipstr_bias_pvalues(int64_t n, const int32_t* u1, const int32_t* u2, const int32_t* r1, const int32_t* r2, double* ab, double* fs){
  if (check_pvalues(n, u1, u2, r1, r2, ab, fs)) return 1;
  for (int i = 0; i < 4; i++) g_last[i] = 0;
  if (n == 0) return 0;
  if (n > (int64_t)INT32_MAX*HS_REC_THREADS/2) return api_fail("hipstr_bias_pvalues: too many quadruples for one call");
  hipstr::ApiTables A;
  if (hipstr::api_device_tables(&A)) return 1;
  const double* table;
  if (device_table(A.ctx, &table)) return 1;
  hipStream_t st = A.stream;
  const size_t nn = (size_t)n;
  hipstr::HostArena ar;
  hs_rec_pv_dev_t h; memset(&h, 0, sizeof h);
  const size_t o1 = ar.add(u1, nn*4), o2 = ar.add(u2, nn*4), o3 = ar.add(r1, nn*4), o4 = ar.add(r2, nn*4), o_args = ar.add(&h, sizeof h);
  if (ar.reserve(A.ctx)) return 1;
  hipstr::ResultBlocks B;
  const size_t r_ab = B.take(nn*8), r_fs = B.take(nn*8);
  B.end_results();
  if (B.reserve(A.ctx, st)) return 1;
  h.table = table; h.u1 = ar.at<int32_t>(o1); h.u2 = ar.at<int32_t>(o2); h.rv1 = ar.at<int32_t>(o3); h.rv2 = ar.at<int32_t>(o4);
  h.ab = B.dev<double>(r_ab); h.fs = B.dev<double>(r_fs); h.n = n;
  if (ar.send(st)) return 1;
  hipLaunchKernelGGL(hs_rec_pvalues_kernel, dim3((unsigned)((n + HS_REC_THREADS - 1)/HS_REC_THREADS)), dim3(HS_REC_THREADS), 0, st, ar.at<hs_rec_pv_dev_t>(o_args));
  HS_HIP(hipGetLastError());
  if (B.fetch()) return 1;
  memcpy(ab, B.host<char>(r_ab), nn*8); memcpy(fs, B.host<char>(r_fs), nn*8);
  int64_t n_host = 0;
  for (int64_t i = 0; i < n; i++)
    if ((int64_t)u1[i] + u2[i] > HS_REC_TABLE_READS){ ab[i] = hr::allele_bias(u1[i], u2[i]); fs[i] = hr::strand_bias(u1[i], r1[i], u2[i], r2[i]); n_host++; }
  g_last[0] = n; g_last[1] = n_host; g_last[2] = (int64_t)ar.total; g_last[3] = (int64_t)B.res;
  return 0;
}

namespace {
int null_batch(const hipstr_post_batch_t* pb){
  return !pb || pb->n_loci < 0 || (pb->n_loci && (!pb->n_alleles || !pb->n_samples));
}
int64_t samples_of(int n_loci, const int32_t* n_samples){ int64_t n = 0; for (int l = 0; l < n_loci; l++) n += n_samples[l]; return n; }
}  // namespace

extern "C" int hipstr_record_fields_host(const hipstr_post_batch_t* pb, const int32_t* map_gt, const hipstr_record_request_t* rq, hipstr_record_out_t* out){
  if (null_batch(pb) || hr::null_request(rq) || hr::null_out(out)) return api_fail("null argument");
  for (int l = 0; l < pb->n_loci; l++) if (pb->n_samples[l] < 0) return api_fail("hipstr_record_fields: a negative sample count");
  if (!map_gt && samples_of(pb->n_loci, pb->n_samples) > 0) return api_fail("null argument");
  const std::string why = hr::fields(pb->n_loci, pb->n_alleles, pb->n_samples, pb->haploid, map_gt, rq, out);
  return why.empty() ? 0 : api_fail("hipstr_record_fields: " + why);
}

extern "C" int hipstr_record_fields(hipstr_post_dev_t* pd, const hipstr_record_request_t* rq, hipstr_record_out_t* out){
  if (!pd || hr::null_request(rq) || hr::null_out(out)) return api_fail("null argument");
  hipstr::PostView V;
  hipstr::post_view(pd, &V);
  if (!V.launched) return api_fail("hipstr_record_fields needs the MAP pairs: call hipstr_post_launch first");
  const int nl = (int)V.n_loci;
  {
    const std::string why = hr::check_request(nl, V.n_alleles, V.n_samples, rq);
    if (!why.empty()) return api_fail("hipstr_record_fields: " + why);
  }
  for (int i = 0; i < 4; i++) g_last[i] = 0;
  const int64_t ns64 = V.n_samp;
  if (ns64 == 0){
    int64_t vo = 0;
    for (int l = 0; l < nl; l++){
      out->n_skip[l] = out->n_filt[l] = out->an[l] = out->dp[l] = out->dsnp[l] = out->dstutter[l] = out->dflankindel[l] = 0;
      for (int v = 0; v < rq->n_variants[l]; v++) out->allele_count[vo + v] = 0;
      vo += rq->n_variants[l];
    }
    return 0;
  }
  if (ns64 > INT32_MAX/2) return api_fail("hipstr_record_fields: too many samples for one call");
  const size_t ns = (size_t)ns64;
  // the workgroups: a wavefront per 64 samples of a locus
  int64_t ho = 0, vo = 0; size_t ng = 0;
  for (int l = 0; l < nl; l++){
    ng += ((size_t)V.n_samples[l] + HS_REC_THREADS - 1)/HS_REC_THREADS; ho += V.n_alleles[l]; vo += rq->n_variants[l];
    if (ho > INT32_MAX || vo > INT32_MAX) return api_fail("hipstr_record_fields: too many haplotypes for one call");
  }
  const size_t nv = (size_t)vo;

  hipstr::ApiTables A;
  if (hipstr::api_tables_of(V.ctx, &A)) return 1;
  const double* table;
  if (device_table(V.ctx, &table)) return 1;
  hipStream_t st = A.stream;
  // Every array of the call lies in a block of the context's caches, device or pinned: the caller's arrays are packed from where they lie,
  // the loci and the workgroups' list are written into the pinned block itself.  (Host heap: the arena's list of a dozen pieces only.)
  hipstr::HostArena ar;
  hs_rec_dev_t h; memset(&h, 0, sizeof h);
  const int32_t* const cnt[8] = { rq->n_aligned, rq->n_snp, rq->n_stutter, rq->n_flank_indel, rq->uniq_one, rq->uniq_two, rq->rv_uniq_one, rq->rv_uniq_two };
  const size_t o_loci = ar.add(NULL, (size_t)nl*sizeof(hs_rec_locus_t)), o_gl = ar.add(NULL, ng*4),
               o_h2a = ar.add(rq->hap_to_allele, (size_t)ho*4), o_rep = rq->sample_reported ? ar.add(rq->sample_reported, ns) : 0,
               o_msk = rq->sample_masked ? ar.add(rq->sample_masked, ns) : 0;
  size_t o_cnt[8];
  for (int k = 0; k < 8; k++) o_cnt[k] = ar.add(cnt[k], ns*4);
  const size_t o_args = ar.add(&h, sizeof h);
  if (ar.reserve(V.ctx)) return 1;
  {
    hs_rec_locus_t* const loci = (hs_rec_locus_t*)(ar.pin + o_loci);
    int32_t* const group_locus = (int32_t*)(ar.pin + o_gl);
    int64_t so = 0, hh = 0, vv = 0; size_t g = 0;
    for (int l = 0; l < nl; l++){
      hs_rec_locus_t& L = loci[l];
      L.samp_off = (int32_t)so; L.n_samples = V.n_samples[l]; L.hap_off = (int32_t)hh; L.n_alleles = V.n_alleles[l];
      L.var_off = (int32_t)vv; L.n_variants = rq->n_variants[l]; L.haploid = V.haploid[l] ? 1 : 0; L.first_group = (int32_t)g;
      for (int s = 0; s < L.n_samples; s += HS_REC_THREADS) group_locus[g++] = l;
      so += L.n_samples; hh += L.n_alleles; vv += L.n_variants;
    }
  }
  hipstr::ResultBlocks B;
  const size_t r_status = B.take(ns*4), r_gt = B.take(ns*8), r_dab = B.take(ns*4), r_ab = B.take(ns*8), r_fs = B.take(ns*8);
  const size_t r_zero = B.take((size_t)7*nl*4), r_ac = B.take(nv*4), r_err = B.take(4);       // zeroed before the launch, one memset: back to back
  B.end_results();
  if (B.reserve(V.ctx, st)) return 1;
  h.table = table; h.loci = ar.at<hs_rec_locus_t>(o_loci); h.group_locus = ar.at<int32_t>(o_gl); h.map_gt = V.map_gt;
  h.hap_to_allele = ar.at<int32_t>(o_h2a); h.reported = rq->sample_reported ? ar.at<uint8_t>(o_rep) : NULL;
  h.masked = rq->sample_masked ? ar.at<uint8_t>(o_msk) : NULL;
  for (int k = 0; k < 8; k++) h.counts[k] = ar.at<int32_t>(o_cnt[k]);
  h.status = B.dev<int32_t>(r_status); h.gt = B.dev<int32_t>(r_gt); h.dab = B.dev<int32_t>(r_dab); h.ab = B.dev<double>(r_ab); h.fs = B.dev<double>(r_fs);
  h.locus_out = B.dev<int32_t>(r_zero); h.allele_count = B.dev<int32_t>(r_ac); h.error = B.dev<int32_t>(r_err);
  h.n_loci = nl; h.n_groups = (int32_t)ng; h.n_samp = ns64; h.frac = hr::flank_frac_of(rq);
  // the MAP pairs are the posterior kernel's: behind it, whichever stream it ran on
  if (V.foreign_stream) HS_HIP(hipDeviceSynchronize());
  else if (st != V.stream) HS_HIP(hipstr::wait_stream(V.stream));
  if (ar.send(st)) return 1;
  HS_HIP(hipMemsetAsync(B.dev<char>(r_zero), 0, B.res - r_zero, st));
  hipLaunchKernelGGL(hs_rec_fields_kernel, dim3((unsigned)ng), dim3(HS_REC_THREADS), 0, st, ar.at<hs_rec_dev_t>(o_args));
  HS_HIP(hipGetLastError());
  if (B.fetch()) return 1;
  const int err = *B.host<int32_t>(r_err);
  if (err & HS_REC_ERR_MAP_RANGE) return api_fail("hipstr_record_fields: map_gt outside [-1, n_alleles)");
  if (err & HS_REC_ERR_NO_PAIR) return api_fail("hipstr_record_fields: a sample with reads and without a MAP pair");
  if (err & HS_REC_ERR_HAPLOID_HET) return api_fail("hipstr_record_fields: a heterozygous genotype at a haploid locus");
  memcpy(out->status, B.host<char>(r_status), ns*4); memcpy(out->gt, B.host<char>(r_gt), ns*8); memcpy(out->dab, B.host<char>(r_dab), ns*4);
  memcpy(out->ab, B.host<char>(r_ab), ns*8); memcpy(out->fs, B.host<char>(r_fs), ns*8);
  int32_t* const loc[7] = { out->n_skip, out->n_filt, out->an, out->dp, out->dsnp, out->dstutter, out->dflankindel };
  for (int k = 0; k < 7; k++) memcpy(loc[k], B.host<char>(r_zero) + (size_t)k*nl*4, (size_t)nl*4);
  memcpy(out->allele_count, B.host<char>(r_ac), nv*4);
  // samples beyond the table: the host twin, inside the same call (dab != 0 marks a sample whose p-values are computed; an empty total is
  // never beyond the table)
  int64_t n_host = 0;
  for (size_t s = 0; s < ns; s++)
    if (out->dab[s] != 0 && (int64_t)rq->uniq_one[s] + rq->uniq_two[s] > HS_REC_TABLE_READS){
      out->ab[s] = hr::allele_bias(rq->uniq_one[s], rq->uniq_two[s]);
      out->fs[s] = hr::strand_bias(rq->uniq_one[s], rq->rv_uniq_one[s], rq->uniq_two[s], rq->rv_uniq_two[s]);
      n_host++;
    }
  g_last[0] = ns64; g_last[1] = n_host; g_last[2] = (int64_t)ar.total; g_last[3] = (int64_t)B.res;
  return 0;
}

#ifndef HIPSTR_NO_DEBUG_ABI
// the calling thread's last device call of this file: out[0] lanes, out[1] computed by the host twin, out[2] bytes up, out[3] bytes home
extern "C" int hipstr_debug_record_last(int64_t out[4]){
  if (!out) return api_fail("null argument");
  for (int i = 0; i < 4; i++) out[i] = g_last[i];
  return 0;
}
#endif
