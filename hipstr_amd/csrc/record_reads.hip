// record_reads.hip — the per-read sizes of a VCF record and their per-sample histograms on the device: hipstr_cigar_bp_diffs and
// hipstr_sample_histograms (include/hipstr_hmm.h) with their host forms, and the host-only hipstr_em_batch_from_bp_diffs.
//
//   hs_rr_cigar_kernel   one lane per read walks the read's runs (record_reads_layout.h: the lane's body).  Integer work on a few dozen bytes
//                        per read; the lanes of a wavefront diverge by their run counts only.
//   hs_rr_hist_kernel    one wavefront per sample: the values other than the skip value are packed into LDS (a ballot per 64 reads), every
//                        value is put at its rank — the values that sort before it, counted by its lane over LDS broadcasts — the run heads
//                        are packed the same way, and the sample's pairs go to a scratch piece at the sample's first read.
//   hs_rr_scan_kernel    one workgroup: the samples' pair counts into pair_off, in chunks with a carried base.
//   hs_rr_write_kernel   one wavefront per sample copies its pairs to pair_off[s].
// A sample beyond HS_RR_HIST_READS is condensed by the host twin BEFORE the launch: its count and pairs are uploaded, and the scan and the
// write treat it like every other sample, so the offsets behind it need no second pass.  A read beyond HS_RR_CIGAR_RUNS is walked by the
// host twin after the fetch.
#include <hip/hip_runtime.h>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "api_internal.h"
#include "record_reads_host.h"
#include "record_reads_layout.h"

using hipstr::api_fail;
namespace rr = hipstr_record_reads;

static_assert(HS_RR_CIGAR_RUNS == HIPSTR_CIGAR_DEVICE_RUNS && HS_RR_HIST_READS == HIPSTR_HISTOGRAM_DEVICE_READS, "the header states the caps");

// ---------------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(HS_RR_CIGAR_THREADS) void hs_rr_cigar_kernel(const hs_rr_cigar_dev_t* __restrict__ args){
  const hs_rr_cigar_dev_t d = *args;
  const int64_t r = (int64_t)blockIdx.x*HS_RR_CIGAR_THREADS + threadIdx.x;
  if (r >= d.n_reads) return;
  const int32_t c0 = d.cigar_off[r], n = d.cigar_off[r + 1] - c0;
  if (n > HS_RR_CIGAR_RUNS) return;                           // the host fills it in
  const int l = d.read_locus[r];
  int32_t bp;
  const int got = hs_rr_cigar_lane(d.cigar_op + c0, d.cigar_len + c0, n, d.read_start[r], d.pad_start[l], d.pad_end[l], &bp);
  d.got[r] = (uint8_t)got; d.bp_diff[r] = bp;
}

__global__ __launch_bounds__(HS_RR_WAVE) void hs_rr_hist_kernel(const hs_rr_hist_dev_t* __restrict__ args){
  const hs_rr_hist_dev_t d = *args;
  __shared__ int32_t raw[HS_RR_HIST_READS], sorted[HS_RR_HIST_READS], head_at[HS_RR_HIST_READS];
  const int lane = threadIdx.x;
  const hs_rr_unit_t u = d.units[blockIdx.x];
  if (u.big_off >= 0 || u.n_reads > HS_RR_HIST_READS) return;   // (the whole wavefront) the host's pairs and count are there already
  const unsigned long long below = (1ull << lane) - 1;
  int m = 0;
  for (int base = 0; base < u.n_reads; base += HS_RR_WAVE){
    const int i = base + lane;
    const int32_t v = i < u.n_reads ? d.value[u.read_begin + i] : 0;
    const bool keep = i < u.n_reads && v != d.skip;
    const unsigned long long mask = __ballot(keep);
    if (keep) raw[m + __popcll(mask & below)] = v;
    m += __popcll(mask);
  }
  __syncthreads();
  for (int i = lane; i < m; i += HS_RR_WAVE) sorted[hs_rr_rank(raw, m, i)] = raw[i];
  __syncthreads();
  int np = 0;
  for (int base = 0; base < m; base += HS_RR_WAVE){
    const int k = base + lane;
    const bool head = k < m && hs_rr_is_head(sorted, k);
    const unsigned long long mask = __ballot(head);
    if (head) head_at[np + __popcll(mask & below)] = k;
    np += __popcll(mask);
  }
  __syncthreads();
  for (int p = lane; p < np; p += HS_RR_WAVE){
    const int k = head_at[p];
    d.tmp_value[u.read_begin + p] = sorted[k];
    d.tmp_count[u.read_begin + p] = (p + 1 < np ? head_at[p + 1] : m) - k;
  }
  if (lane == 0) d.n_pairs[blockIdx.x] = np;
}

// One workgroup: a thread per sample of a chunk, an inclusive scan (Hillis-Steele) per chunk, the base carried from chunk to chunk.
__global__ __launch_bounds__(HS_RR_SCAN_CHUNK) void hs_rr_scan_kernel(const hs_rr_hist_dev_t* __restrict__ args){
  const hs_rr_hist_dev_t d = *args;
  const int tid = threadIdx.x;
  __shared__ int sc[HS_RR_SCAN_CHUNK];
  __shared__ int base;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int s0 = 0; s0 < d.n_samp; s0 += HS_RR_SCAN_CHUNK){
    const int s = s0 + tid;
    const int v = s < d.n_samp ? d.n_pairs[s] : 0;
    sc[tid] = v;
    __syncthreads();
    for (int off = 1; off < HS_RR_SCAN_CHUNK; off <<= 1){
      const int a = tid >= off ? sc[tid - off] : 0;
      __syncthreads();
      sc[tid] += a;
      __syncthreads();
    }
    if (s < d.n_samp) d.pair_off[s] = base + sc[tid] - v;
    __syncthreads();
    if (tid == HS_RR_SCAN_CHUNK - 1) base += sc[HS_RR_SCAN_CHUNK - 1];
    __syncthreads();
  }
  if (tid == 0) d.pair_off[d.n_samp] = base;
}

__global__ __launch_bounds__(HS_RR_WAVE) void hs_rr_write_kernel(const hs_rr_hist_dev_t* __restrict__ args){
  const hs_rr_hist_dev_t d = *args;
  const hs_rr_unit_t u = d.units[blockIdx.x];
  const int np = d.n_pairs[blockIdx.x], to = d.pair_off[blockIdx.x];
  if (np > u.n_reads || to < 0 || (int64_t)to + np > d.n_reads) return;       // (never: a sample has at most a pair per read)
  const int32_t* const sv = u.big_off >= 0 ? d.big_value + u.big_off : d.tmp_value + u.read_begin;
  const int32_t* const sn = u.big_off >= 0 ? d.big_count + u.big_off : d.tmp_count + u.read_begin;
  for (int p = threadIdx.x; p < np; p += HS_RR_WAVE){ d.hist_value[to + p] = sv[p]; d.hist_count[to + p] = sn[p]; }
}

// ---------------------------------------------------------------------------------------------------------------- host side
namespace {
thread_local int64_t g_last[4];       // of the calling thread's last device call: items (reads / samples), done by the host twin, bytes up, bytes home

bool null_cigars(const hipstr_cigar_request_t* rq){
  return !rq || rq->n_loci < 0 || !rq->read_off || !rq->cigar_off || (rq->n_loci && (!rq->region_start || !rq->region_stop || !rq->pad));
}
// the checks of both forms; n_reads and the padded regions on success
int check_cigar_call(const hipstr_cigar_request_t* rq, uint8_t* got, int32_t* bp_diff, int64_t* nr, int64_t* nc, std::vector<int32_t>* ps, std::vector<int32_t>* pe){
  if (null_cigars(rq)) return api_fail("null argument");
  for (int l = 0; l < rq->n_loci; l++) if (rq->read_off[l + 1] < 0) return api_fail("hipstr_cigar_bp_diffs: read_off must ascend");
  if (rq->n_loci && rq->read_off[rq->n_loci] > 0 && (!rq->read_start || !rq->cigar_op || !rq->cigar_len || !got || !bp_diff)) return api_fail("null argument");
  const std::string why = rr::check_cigars(rq, nr, nc, ps, pe);
  return why.empty() ? 0 : api_fail("hipstr_cigar_bp_diffs: " + why);
}

bool null_hist(const hipstr_post_batch_t* pb, const int32_t* pair_off){
  return !pb || pb->n_loci < 0 || !pair_off || !pb->read_off || (pb->n_loci && !pb->n_samples);
}
int check_hist_call(const char* who, const hipstr_post_batch_t* pb, const int32_t* value, const int32_t* pair_off, const int32_t* hv, const int32_t* hc,
                    std::vector<int32_t>* begin, std::vector<int32_t>* count){
  if (null_hist(pb, pair_off)) return api_fail("null argument");
  for (int l = 0; l < pb->n_loci; l++) if (pb->read_off[l + 1] < 0) return api_fail(std::string(who) + ": read_off must ascend");
  if (pb->read_off[pb->n_loci] > 0 && (!pb->sample_label || !value || !hv || !hc)) return api_fail("null argument");
  const std::string why = rr::sample_runs(pb, begin, count);
  return why.empty() ? 0 : api_fail(std::string(who) + ": " + why);
}
}  // namespace

extern "C" int hipstr_cigar_bp_diffs_host(const hipstr_cigar_request_t* rq, uint8_t* got, int32_t* bp_diff){
  int64_t nr, nc; std::vector<int32_t> ps, pe;
  if (check_cigar_call(rq, got, bp_diff, &nr, &nc, &ps, &pe)) return 1;
  rr::cigars(rq, ps.data(), pe.data(), got, bp_diff);
  return 0;
}

extern "C" int hipstr_cigar_bp_diffs(const hipstr_cigar_request_t* rq, uint8_t* got, int32_t* bp_diff){
  int64_t nr64, nc64; std::vector<int32_t> ps, pe;
  if (check_cigar_call(rq, got, bp_diff, &nr64, &nc64, &ps, &pe)) return 1;
  for (int i = 0; i < 4; i++) g_last[i] = 0;
  if (nr64 == 0) return 0;
  const size_t nr = (size_t)nr64, nc = (size_t)nc64, nl = (size_t)rq->n_loci;
  hipstr::ApiTables A;
  if (hipstr::api_device_tables(&A)) return 1;
  hipStream_t st = A.stream;
  hipstr::HostArena ar;
  hs_rr_cigar_dev_t h; memset(&h, 0, sizeof h);
  const size_t o_loc = ar.add(NULL, nr*4), o_start = ar.add(rq->read_start, nr*4), o_coff = ar.add(rq->cigar_off, (nr + 1)*4),
               o_op = ar.add(rq->cigar_op, nc), o_len = ar.add(rq->cigar_len, nc*4), o_ps = ar.add(ps.data(), nl*4), o_pe = ar.add(pe.data(), nl*4),
               o_args = ar.add(&h, sizeof h);
  if (ar.reserve(A.ctx)) return 1;
  {
    int32_t* const loc = (int32_t*)(ar.pin + o_loc);
    for (int l = 0; l < rq->n_loci; l++) for (int32_t r = rq->read_off[l]; r < rq->read_off[l + 1]; r++) loc[r] = l;
  }
  hipstr::ResultBlocks B;
  const size_t r_got = B.take(nr), r_bp = B.take(nr*4);
  B.end_results();
  if (B.reserve(A.ctx, st)) return 1;
  h.read_locus = ar.at<int32_t>(o_loc); h.read_start = ar.at<int32_t>(o_start); h.cigar_off = ar.at<int32_t>(o_coff);
  h.cigar_op = ar.at<uint8_t>(o_op); h.cigar_len = ar.at<int32_t>(o_len); h.pad_start = ar.at<int32_t>(o_ps); h.pad_end = ar.at<int32_t>(o_pe);
  h.got = B.dev<uint8_t>(r_got); h.bp_diff = B.dev<int32_t>(r_bp); h.n_reads = (int32_t)nr; h.n_loci = rq->n_loci;
  if (ar.send(st)) return 1;
  hipLaunchKernelGGL(hs_rr_cigar_kernel, dim3((unsigned)((nr + HS_RR_CIGAR_THREADS - 1)/HS_RR_CIGAR_THREADS)), dim3(HS_RR_CIGAR_THREADS), 0, st, ar.at<hs_rr_cigar_dev_t>(o_args));
  HS_HIP(hipGetLastError());
  if (B.fetch()) return 1;
  memcpy(got, B.host<char>(r_got), nr); memcpy(bp_diff, B.host<char>(r_bp), nr*4);
  int64_t n_host = 0;
  for (int l = 0; l < rq->n_loci; l++)
    for (int32_t r = rq->read_off[l]; r < rq->read_off[l + 1]; r++){
      const int32_t c0 = rq->cigar_off[r], n = rq->cigar_off[r + 1] - c0;
      if (n <= HS_RR_CIGAR_RUNS) continue;
      got[r] = rr::extract_cigar(rq->cigar_op + c0, rq->cigar_len + c0, n, rq->read_start[r], ps[l], pe[l], &bp_diff[r]) ? 1 : 0;
      n_host++;
    }
  g_last[0] = nr64; g_last[1] = n_host; g_last[2] = (int64_t)ar.total; g_last[3] = (int64_t)B.res;
  return 0;
}

extern "C" int hipstr_sample_histograms_host(const hipstr_post_batch_t* pb, const int32_t* value, int32_t skip, int32_t* pair_off, int32_t* hist_value, int32_t* hist_count){
  std::vector<int32_t> begin, count;
  if (check_hist_call("hipstr_sample_histograms", pb, value, pair_off, hist_value, hist_count, &begin, &count)) return 1;
  int32_t to = 0;
  for (size_t s = 0; s < begin.size(); s++){
    pair_off[s] = to;
    if (count[s]) to += rr::condense(value + begin[s], count[s], skip, hist_value + to, hist_count + to);
  }
  pair_off[begin.size()] = to;
  return 0;
}

extern "C" int hipstr_sample_histograms(const hipstr_post_batch_t* pb, const int32_t* value, int32_t skip, int32_t* pair_off, int32_t* hist_value, int32_t* hist_count){
  std::vector<int32_t> begin, count;
  if (check_hist_call("hipstr_sample_histograms", pb, value, pair_off, hist_value, hist_count, &begin, &count)) return 1;
  for (int i = 0; i < 4; i++) g_last[i] = 0;
  const size_t ns = begin.size(), nr = (size_t)pb->read_off[pb->n_loci];
  if (ns == 0 || nr == 0){ for (size_t s = 0; s <= ns; s++) pair_off[s] = 0; return 0; }
  // the samples beyond the cap: the host twin, now
  std::vector<int32_t> big_v, big_c;
  int64_t n_host = 0;
  for (size_t s = 0; s < ns; s++) if (count[s] > HS_RR_HIST_READS) n_host++;
  hipstr::ApiTables A;
  if (hipstr::api_device_tables(&A)) return 1;
  hipStream_t st = A.stream;
  std::vector<int32_t> big_off, big_n;
  if (n_host){
    big_off.assign(ns, -1); big_n.assign(ns, 0);
    for (size_t s = 0; s < ns; s++) if (count[s] > HS_RR_HIST_READS){
      const size_t at = big_v.size();
      big_v.resize(at + (size_t)count[s]); big_c.resize(at + (size_t)count[s]);
      const int np = rr::condense(value + begin[s], count[s], skip, big_v.data() + at, big_c.data() + at);
      big_v.resize(at + (size_t)np); big_c.resize(at + (size_t)np);
      big_off[s] = (int32_t)at; big_n[s] = np;
    }
  }
  hipstr::HostArena ar;
  hs_rr_hist_dev_t h; memset(&h, 0, sizeof h);
  const size_t o_units = ar.add(NULL, ns*sizeof(hs_rr_unit_t)), o_np = ar.add(NULL, ns*4), o_val = ar.add(value, nr*4),
               o_bv = ar.add(big_v.data(), big_v.size()*4), o_bc = ar.add(big_c.data(), big_c.size()*4), o_args = ar.add(&h, sizeof h);
  if (ar.reserve(A.ctx)) return 1;
  {
    hs_rr_unit_t* const units = (hs_rr_unit_t*)(ar.pin + o_units);
    int32_t* const n_pairs = (int32_t*)(ar.pin + o_np);
    for (size_t s = 0; s < ns; s++){
      units[s].read_begin = begin[s]; units[s].n_reads = count[s]; units[s].big_off = n_host ? big_off[s] : -1; units[s].pad_ = 0;
      n_pairs[s] = n_host ? big_n[s] : 0;
    }
  }
  hipstr::ResultBlocks B;
  const size_t r_off = B.take((ns + 1)*4), r_val = B.take(nr*4), r_cnt = B.take(nr*4);
  B.end_results();
  const size_t w_val = B.take(nr*4), w_cnt = B.take(nr*4);
  if (B.reserve(A.ctx, st)) return 1;
  h.units = ar.at<hs_rr_unit_t>(o_units); h.value = ar.at<int32_t>(o_val); h.big_value = ar.at<int32_t>(o_bv); h.big_count = ar.at<int32_t>(o_bc);
  h.n_pairs = ar.at<int32_t>(o_np); h.tmp_value = B.dev<int32_t>(w_val); h.tmp_count = B.dev<int32_t>(w_cnt);
  h.pair_off = B.dev<int32_t>(r_off); h.hist_value = B.dev<int32_t>(r_val); h.hist_count = B.dev<int32_t>(r_cnt);
  h.n_samp = (int32_t)ns; h.n_reads = (int32_t)nr; h.skip = skip;
  if (ar.send(st)) return 1;
  const hs_rr_hist_dev_t* const d_args = ar.at<hs_rr_hist_dev_t>(o_args);
  hipLaunchKernelGGL(hs_rr_hist_kernel, dim3((unsigned)ns), dim3(HS_RR_WAVE), 0, st, d_args);
  HS_HIP(hipGetLastError());
  hipLaunchKernelGGL(hs_rr_scan_kernel, dim3(1), dim3(HS_RR_SCAN_CHUNK), 0, st, d_args);
  HS_HIP(hipGetLastError());
  hipLaunchKernelGGL(hs_rr_write_kernel, dim3((unsigned)ns), dim3(HS_RR_WAVE), 0, st, d_args);
  HS_HIP(hipGetLastError());
  if (B.fetch()) return 1;
  const int32_t np = B.host<int32_t>(r_off)[ns];             // what lies behind the pairs in the two pieces was never written
  if (np < 0 || (size_t)np > nr) return api_fail("hipstr_sample_histograms: the device's pair count is outside [0, n_reads]");
  memcpy(pair_off, B.host<char>(r_off), (ns + 1)*4);
  memcpy(hist_value, B.host<char>(r_val), (size_t)np*4); memcpy(hist_count, B.host<char>(r_cnt), (size_t)np*4);
  g_last[0] = (int64_t)ns; g_last[1] = n_host; g_last[2] = (int64_t)ar.total; g_last[3] = (int64_t)B.res;
  return 0;
}

extern "C" int hipstr_em_batch_from_bp_diffs(const hipstr_post_batch_t* pb, const uint8_t* got, const int32_t* bp_diff, const int32_t* region_start,
                                             const int32_t* region_stop, int32_t min_total_reads, int32_t* em_read_off, int32_t* sample_label,
                                             int32_t* num_bps, double* log_p1, double* log_p2, uint8_t* too_few){
  if (!pb || pb->n_loci < 0 || !em_read_off || !pb->read_off || (pb->n_loci && (!pb->n_samples || !region_start || !region_stop || !too_few)))
    return api_fail("null argument");
  for (int l = 0; l < pb->n_loci; l++) if (pb->read_off[l + 1] < 0) return api_fail("hipstr_em_batch_from_bp_diffs: read_off must ascend");
  if (pb->read_off[pb->n_loci] > 0 && (!pb->sample_label || !got || !bp_diff || !sample_label || !num_bps || !log_p1 || !log_p2)) return api_fail("null argument");
  if (pb->log_p1 && !pb->log_p2) return api_fail("hipstr_em_batch_from_bp_diffs: log_p1 without log_p2");
  if (min_total_reads < 0) return api_fail("hipstr_em_batch_from_bp_diffs: min_total_reads must not be negative");
  for (int l = 0; l < pb->n_loci; l++) if (region_stop[l] < region_start[l]) return api_fail("hipstr_em_batch_from_bp_diffs: region_stop < region_start");
  std::vector<int32_t> begin, count;
  const std::string why = rr::sample_runs(pb, &begin, &count);
  if (!why.empty()) return api_fail("hipstr_em_batch_from_bp_diffs: " + why);
  const int MAX_INF_READS = 10000;                            // genotyper_bam_processor.cpp:111
  int32_t to = 0; size_t so = 0;
  for (int l = 0; l < pb->n_loci; l++){
    em_read_off[l] = to;
    const int64_t floor_bp = -((int64_t)region_stop[l] - region_start[l] + 1);
    int inf = 0;
    for (int s = 0; s < pb->n_samples[l] && inf <= MAX_INF_READS; s++)
      for (int32_t r = begin[so + s]; r < begin[so + s] + count[so + s]; r++){
        if (!got[r] || bp_diff[r] < floor_bp) continue;
        sample_label[to] = s; num_bps[to] = bp_diff[r];
        log_p1[to] = pb->log_p1 ? pb->log_p1[r] : 0.0; log_p2[to] = pb->log_p1 ? pb->log_p2[r] : 0.0;
        to++; inf++;
      }
    too_few[l] = inf < min_total_reads ? 1 : 0;
    so += (size_t)pb->n_samples[l];
  }
  em_read_off[pb->n_loci] = to;
  return 0;
}

#ifndef HIPSTR_NO_DEBUG_ABI
// the calling thread's last device call of this file: out[0] reads / samples, out[1] done by the host twin, out[2] bytes up, out[3] bytes home
extern "C" int hipstr_debug_record_reads_last(int64_t out[4]){
  if (!out) return api_fail("null argument");
  for (int i = 0; i < 4; i++) out[i] = g_last[i];
  return 0;
}
#endif
