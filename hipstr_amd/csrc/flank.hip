// flank.hip — the flank reassembly that closes SeqStutterGenotyper::genotype() on gfx950: assemble_flanks (seq_stutter_genotyper.cpp:40-217)
// for a batch of loci on a resident traceback result.  One wavefront assembles one (locus, flank, sample) task where the flank strings lie
// (flank_task.h: the De Bruijn graph in two LDS hash tables, pruning, peeling, the path enumeration on one lane); a task writes its few
// paths, a lane each, into one piece of a dense pool of the call (one bump allocation per task), so only the per-task records and the pool's used bytes come home.  The
// aggregation (:99-201) is flank_host.cpp's ONE function on those records, shared with the host entry point; tasks that left the device for
// a limit of flank_layout.h are assembled by the host twin inside the same call, on flank strings fetched once.
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
#include "flank_layout.h"
#include "flank_task.h"
#include "flank_host.h"
#include "api_internal.h"

extern "C" __global__ void __launch_bounds__(HS_FLK_WAVE) hs_flank_task_kernel(const hs_flk_dev_t* __restrict__ dp){
  __shared__ hs_flk_lds_t L;
  const int64_t t = blockIdx.x;
  if (t >= dp->n_tasks) return;                               // (the whole workgroup)
  hs_flk_task(*dp, (int)t, L);
}

// ---- host side -------------------------------------------------------------------------------------------------
namespace {
using hipstr::api_fail;
namespace hf = hipstr_flank;

// the caps of this call: HIPSTR_DEBUG_FLANK_CAPS = "edges,nodes,recs,reads,len,path_len" (missing or 0 = the compiled limit), read per call
hs_flk_caps_t flank_caps(){
  hs_flk_caps_t c = hs_flk_default_caps();
  const char* e = getenv("HIPSTR_DEBUG_FLANK_CAPS");
  if (!e || !*e) return c;
  int32_t* f[6] = { &c.max_edges, &c.max_nodes, &c.max_recs, &c.max_reads, &c.max_len, &c.max_path_len };
  for (int i = 0; i < 6 && *e; i++){
    char* end = NULL;
    const long v = strtol(e, &end, 10);
    if (end == e) break;
    if (v > 0) *f[i] = hs_flk_clamp_cap(v, *f[i]);
    e = *end == ',' ? end + 1 : end;
  }
  return c;
}

bool null_out(const hipstr_flank_out_t* o){
  return !o || !o->status || !o->new_n_haps || !o->opt_off || !o->opt_seq_off || !o->opt_seq || !o->opt_n_samples || !o->sample_status ||
         !o->realign_sample || !o->realign_pool || !o->copy_read;
}

// the tables of a posterior batch (the host entry point): the runs as post_units cuts them
int tables_of_batch(const hipstr_post_batch_t* pb, hf::Tables& T){
  const int nl = pb->n_loci;
  T.n_loci = nl; T.n_samples = pb->n_samples;
  T.read_off.assign((size_t)nl + 1, 0); T.samp_off.assign((size_t)nl + 1, 0);
  for (int l = 0; l < nl; l++){
    const int S = pb->n_samples[l], r0 = pb->read_off[l], r1 = pb->read_off[l+1];
    if (S < 0 || r1 < r0 || r0 < 0) return api_fail("hipstr_flank_assemble: negative counts");
    int r = r0;
    for (int s = 0; s < S; s++){
      T.run_begin.push_back(r);
      while (r < r1 && pb->sample_label[r] == s) r++;
      T.run_len.push_back(r - T.run_begin.back());
    }
    if (r != r1) return api_fail("reads of a locus must be grouped by ascending sample label (genotyper.h:112-119)");
    T.read_off[l] = r0; T.read_off[l+1] = r1; T.samp_off[l+1] = T.samp_off[l] + S;
  }
  return 0;
}

// the per-thread record of the last device call (hipstr_debug_flank_last)
thread_local int64_t g_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
thread_local std::vector<int32_t> g_last_flags, g_last_sizes;

int assemble_all_host(const hipstr_flank_request_t* rq, const hf::Tables& T, const int32_t* flank_off, const char* flank_seq, std::vector<hf::Task>& tasks){
  const hf::Params P = hf::params_of(rq);
  tasks.assign((size_t)T.n_tasks(), hf::Task());
  std::vector<hf::Str> strs;
  for (int l = 0; l < T.n_loci; l++)
    for (int f = 0; f < 2; f++)
      for (int s = 0; s < T.n_samples[l]; s++){
        if (hf::task_skipped(rq, T, l, f, s)) continue;
        hf::task_strings(rq, T, l, f, s, flank_off, flank_seq, strs);
        hf::assemble_task(T.ref[2*l + f], strs, T.kmer[2*l + f], T.max_k[2*l + f], P, tasks[(size_t)T.task_of(l, f, s)]);
      }
  return 0;
}
}  // namespace

extern "C" int hipstr_flank_kmer_lengths(const hipstr_batch_t* b, int32_t min_kmer, int32_t max_kmer, int32_t* kmer){
  if (!b || !kmer || b->n_loci < 0 || (b->n_loci && (!b->blk_nopts || !b->opt_off || !b->seq))) return api_fail("null argument");
  if (!min_kmer) min_kmer = 10;
  if (!max_kmer) max_kmer = 15;
  int64_t oi = 0;
  for (int l = 0; l < b->n_loci; l++)
    for (int blk = 0; blk < 3; blk++){
      const int no = b->blk_nopts[3*l + blk];
      if (no < 1) return api_fail("hipstr_flank_assemble: a block without options");
      if (blk != 1 && b->opt_off[oi+1] < b->opt_off[oi]) return api_fail("hipstr_flank_assemble: opt_off decreases");
      oi += no;
    }
  oi = 0;
  for (int l = 0; l < b->n_loci; l++)
    for (int blk = 0; blk < 3; blk++){
      if (blk != 1){
        const hf::Str ref = { b->seq + b->opt_off[oi], b->opt_off[oi+1] - b->opt_off[oi] };
        kmer[2*l + (blk ? 1 : 0)] = hf::kmer_length(ref, min_kmer, hf::max_k_of(ref.len, max_kmer));
      }
      oi += b->blk_nopts[3*l + blk];
    }
  return 0;
}

extern "C" int hipstr_flank_assemble(const hipstr_post_batch_t* pb, const hipstr_flank_request_t* rq, const hipstr_trace_out_t* tr, hipstr_flank_out_t* out){
  if (!pb || !tr || null_out(out) || hf::null_request(rq)) return api_fail("null argument");
  if (pb->n_loci < 0 || (pb->n_loci && (!pb->n_samples || !pb->read_off || !pb->sample_label))) return api_fail("null argument");
  if (rq->n_req > 0 && (!tr->flank_seq_off || !tr->flank_seq)) return api_fail("hipstr_flank_assemble: trace output without flank_seq_off / flank_seq");
  hf::Tables T;
  if (tables_of_batch(pb, T)) return 1;
  const std::string why = hf::check_tables(rq, T);
  if (!why.empty()) return api_fail(why);
  std::vector<hf::Task> tasks;
  assemble_all_host(rq, T, tr->flank_seq_off, tr->flank_seq, tasks);
  return hf::finish(rq, T, tasks, out);
}

extern "C" int hipstr_flank_assemble_dev(hipstr_post_dev_t* pd, const hipstr_flank_request_t* rq, const hipstr_trace_dev_t* td, hipstr_flank_out_t* out){
  if (!pd || !td || null_out(out) || hf::null_request(rq)) return api_fail("null argument");
  hipstr::PostView V;
  hipstr::post_view(pd, &V);
  if (td->ctx != V.ctx) return api_fail("hipstr_flank_assemble_dev: the trace handle lives on another device than the posteriors");
  if (rq->n_req != td->n_req) return api_fail("hipstr_flank_assemble_dev: rq->n_req differs from the trace handle's");
  if (rq->n_req > 0 && (!(td->groups & HIPSTR_TRACE_F_FLANKS) || !td->off[2] || (td->totals[2] > 0 && !td->arr[2])))
    return api_fail("hipstr_flank_assemble: trace output without flank_seq_off / flank_seq");
  // the tables, from the run's units (locus-major, a unit per sample: unit index == sample slot)
  hf::Tables T;
  const int nl = (int)V.n_loci;
  T.n_loci = nl; T.n_samples = V.n_samples;
  V.locus_tables(T.read_off, T.samp_off);
  for (size_t ui = 0; ui < (size_t)T.n_samp(); ui++){ T.run_begin.push_back(V.units[ui].read_begin); T.run_len.push_back(V.units[ui].n_reads); }
  const std::string why = hf::check_tables(rq, T);
  if (!why.empty()) return api_fail(why);
  const int64_t n_tasks = T.n_tasks();
  for (int i = 0; i < 8; i++) g_last[i] = 0;
  g_last_flags.clear(); g_last_sizes.clear();
  std::vector<hf::Task> tasks((size_t)n_tasks);
  if (n_tasks == 0) return hf::finish(rq, T, tasks, out);
  if (n_tasks > INT32_MAX/HS_FLK_MAX_PATHS) return api_fail("hipstr_flank_assemble_dev: too many samples for one call");

  const hf::Params P = hf::params_of(rq);
  const size_t n = (size_t)V.n_reads, nt = (size_t)n_tasks;
  std::vector<int32_t> task_unit(nt), task_lf(nt), ref_off(2*(size_t)nl + 1, 0);
  std::vector<uint8_t> task_skip(nt);
  std::string ref_seq;
  int64_t sum_ref = 0;
  for (int l = 0; l < nl; l++)
    for (int f = 0; f < 2; f++){
      ref_off[2*l + f] = (int32_t)ref_seq.size();
      ref_seq.append(T.ref[2*l + f].p, (size_t)T.ref[2*l + f].len);
      for (int s = 0; s < V.n_samples[l]; s++){
        const size_t t = (size_t)T.task_of(l, f, s);
        task_unit[t] = T.samp_off[l] + s; task_lf[t] = 2*l + f; task_skip[t] = hf::task_skipped(rq, T, l, f, s) ? 1 : 0;
        sum_ref += T.ref[2*l + f].len;
      }
    }
  ref_off[2*(size_t)nl] = (int32_t)ref_seq.size();
  const int64_t pool_cap = std::min<int64_t>(hs_flk_pool_bytes(n_tasks, sum_ref), INT32_MAX);

  hipstr::ApiTables A;
  if (hipstr::api_tables_of(V.ctx, &A)) return 1;
  hipStream_t st = A.stream;
  hipstr::HostArena ar;
  hs_flk_dev_t h; memset(&h, 0, sizeof h);
  const size_t o_unit = ar.add(task_unit.data(), nt*4), o_lf = ar.add(task_lf.data(), nt*4), o_skip = ar.add(task_skip.data(), nt),
               o_roff = ar.add(ref_off.data(), ref_off.size()*4), o_rseq = ar.add(ref_seq.data(), ref_seq.size()),
               o_kmer = ar.add(T.kmer.data(), T.kmer.size()*4), o_maxk = ar.add(T.max_k.data(), T.max_k.size()*4),
               o_seed = ar.add(rq->seed, n*4), o_rreq = ar.add(rq->read_req, n*4), o_args = ar.add(&h, sizeof h);
  if (ar.reserve(V.ctx)) return 1;
  // what comes home (one copy), then the pool
  hipstr::ResultBlocks B;
  const size_t r_used = B.take(8), r_k = B.take(nt*4), r_flag = B.take(nt*4), r_np = B.take(nt*4), r_size = B.take(nt*4*HS_FLK_SIZES), r_at = B.take(nt*4);
  B.end_results();
  const size_t d_pool = B.take((size_t)pool_cap);
  if (B.reserve(V.ctx, st)) return 1;
  h.units = V.d_units; h.task_unit = ar.at<int32_t>(o_unit); h.task_lf = ar.at<int32_t>(o_lf); h.task_skip = ar.at<uint8_t>(o_skip);
  h.ref_off = ar.at<int32_t>(o_roff); h.ref_seq = ar.at<char>(o_rseq); h.kmer0 = ar.at<int32_t>(o_kmer); h.max_k = ar.at<int32_t>(o_maxk);
  h.seed = ar.at<int32_t>(o_seed); h.read_req = ar.at<int32_t>(o_rreq);
  h.flank_off = td->off[2]; h.flank_seq = td->arr[2]; h.flank_total = td->totals[2];
  h.task_k = B.dev<int32_t>(r_k); h.task_flag = B.dev<int32_t>(r_flag); h.task_np = B.dev<int32_t>(r_np); h.task_size = B.dev<int32_t>(r_size);
  h.task_at = B.dev<int32_t>(r_at);
  h.pool = B.dev<char>(d_pool); h.pool_used = B.dev<unsigned long long>(r_used); h.pool_cap = pool_cap;
  h.n_tasks = (int32_t)n_tasks; h.min_path_weight = P.min_path_weight; h.max_paths = P.max_paths;
  h.caps = flank_caps();
  // the run's inputs may still be on their way (a small run sends them asynchronously on its own stream)
  if (V.ev_up && st != V.stream) HS_HIP(hipStreamWaitEvent(st, V.ev_up, 0));
  if (ar.send(st)) return 1;
  HS_HIP(hipMemsetAsync(B.dev<char>(r_used), 0, 8, st));
  hipLaunchKernelGGL(hs_flank_task_kernel, dim3((unsigned)n_tasks), dim3(HS_FLK_WAVE), 0, st, ar.at<hs_flk_dev_t>(o_args));
  HS_HIP(hipGetLastError());
  if (B.fetch()) return 1;
  const int64_t used = std::min<int64_t>((int64_t)*B.host<unsigned long long>(r_used), pool_cap);
  std::vector<char> pool_h((size_t)std::max<int64_t>(used, 0));       // the part of the pool in use, in a copy of its own
  if (used > 0 && hipstr::fetch_to_host(V.ctx, st, pool_h.data(), B.dev<char>(d_pool), (size_t)used)) return 1;
  const char* pool = pool_h.data();
  const int32_t *tk = B.host<int32_t>(r_k), *tf = B.host<int32_t>(r_flag), *tn = B.host<int32_t>(r_np), *pa = B.host<int32_t>(r_at);
  g_last_flags.assign(tf, tf + nt);
  g_last_sizes.assign(B.host<int32_t>(r_size), B.host<int32_t>(r_size) + nt*HS_FLK_SIZES);
  g_last[0] = n_tasks; g_last[4] = (int64_t)ar.total; g_last[5] = (int64_t)B.res + used;
  size_t n_fall = 0;
  for (size_t t = 0; t < nt; t++){
    if (tf[t]){ n_fall++; continue; }
    hf::Task& K = tasks[t];
    K.k = tk[t];
    if (K.k == HIPSTR_FLANK_TASK_SKIPPED) g_last[1]++;
    int64_t at = pa[t];
    for (int i = 0; i < tn[t]; i++){
      if (at < 0 || at + 8 > used) return api_fail("hipstr_flank_assemble_dev: a path record outside the pool");
      int32_t head[2]; memcpy(head, pool + at, 8);
      if (head[1] < 0 || at + hs_flk_path_bytes(head[1]) > used) return api_fail("hipstr_flank_assemble_dev: a path record outside the pool");
      K.paths.emplace_back(pool + at + 8, (size_t)head[1]); K.weights.push_back(head[0]);
      at += hs_flk_path_bytes(head[1]);
    }
  }
  g_last[2] = (int64_t)n_fall;
  if (n_fall){
    // the flank strings, fetched once, for the host twin
    const size_t n_off = 2*(size_t)td->n_req + 1, n_chr = (size_t)td->totals[2];
    std::vector<int32_t> foff(n_off); std::vector<char> fseq(n_chr ? n_chr : 1);
    char* p = (char*)hipstr::pin_alloc(V.ctx, n_off*4 + n_chr);
    if (!p) return 1;
    bool ok = hipMemcpyAsync(p, td->off[2], n_off*4, hipMemcpyDeviceToHost, st) == hipSuccess &&
              (!n_chr || hipMemcpyAsync(p + n_off*4, td->arr[2], n_chr, hipMemcpyDeviceToHost, st) == hipSuccess);
    ok = hipstr::wait_stream(st) == hipSuccess && ok;
    if (ok){ memcpy(foff.data(), p, n_off*4); if (n_chr) memcpy(fseq.data(), p + n_off*4, n_chr); } else hipStreamSynchronize(st);
    hipstr::pin_free(V.ctx, p);
    if (!ok) return api_fail("device-to-host copy failed");
    for (size_t i = 0; i + 1 < n_off; i++)
      if (foff[i] < 0 || foff[i+1] < foff[i] || (size_t)foff[i+1] > n_chr) return api_fail("hipstr_flank_assemble_dev: flank_seq_off decreases or leaves the pool");
    g_last[5] += (int64_t)(n_off*4 + n_chr); g_last[3] = 1;
    std::vector<hf::Str> strs;
    for (int l = 0; l < nl; l++)
      for (int f = 0; f < 2; f++)
        for (int s = 0; s < V.n_samples[l]; s++){
          const size_t t = (size_t)T.task_of(l, f, s);
          if (!tf[t]) continue;
          hf::task_strings(rq, T, l, f, s, foff.data(), fseq.data(), strs);
          hf::assemble_task(T.ref[2*l + f], strs, T.kmer[2*l + f], T.max_k[2*l + f], P, tasks[t]);
        }
  }
  return hf::finish(rq, T, tasks, out);
}

#ifndef HIPSTR_NO_DEBUG_ABI
extern "C" int hipstr_debug_flank_last(int64_t out[8], int32_t* flags, int32_t* sizes, int64_t cap_tasks){
  if (!out) return api_fail("null argument");
  for (int i = 0; i < 8; i++) out[i] = g_last[i];
  const size_t nt = std::min<size_t>(g_last_flags.size(), cap_tasks < 0 ? 0 : (size_t)cap_tasks);
  if (flags && nt) memcpy(flags, g_last_flags.data(), nt*4);
  if (sizes && nt) memcpy(sizes, g_last_sizes.data(), nt*4*HS_FLK_SIZES);
  return 0;
}

extern "C" int hipstr_debug_flank_plan(const hipstr_post_batch_t* pb, const hipstr_flank_request_t* rq, const hipstr_trace_out_t* tr, char* json, int cap){
  if (!pb || !tr || hf::null_request(rq) || (cap > 0 && !json)){ api_fail("null argument"); return -1; }
  if (pb->n_loci < 0 || (pb->n_loci && (!pb->n_samples || !pb->read_off || !pb->sample_label))){ api_fail("null argument"); return -1; }
  if (rq->n_req > 0 && (!tr->flank_seq_off || !tr->flank_seq)){ api_fail("hipstr_flank_assemble: trace output without flank_seq_off / flank_seq"); return -1; }
  hf::Tables T;
  if (tables_of_batch(pb, T)) return -1;
  const std::string why = hf::check_tables(rq, T);
  if (!why.empty()){ api_fail(why); return -1; }
  const hs_flk_caps_t caps = flank_caps();
  const hf::Params P = hf::params_of(rq);
  std::string s = "{\"thresholds\": {";
  auto kv = [&](const char* k, int64_t v, bool last = false){ s += "\"" + std::string(k) + "\": " + std::to_string(v) + (last ? "" : ", "); };
  kv("HS_FLK_WAVE", HS_FLK_WAVE); kv("HS_FLK_MAX_K", HS_FLK_MAX_K); kv("HS_FLK_K_STEPS", HS_FLK_K_STEPS); kv("HS_FLK_EDGE_SLOTS", HS_FLK_EDGE_SLOTS);
  kv("HS_FLK_NODE_SLOTS", HS_FLK_NODE_SLOTS); kv("HS_FLK_MAX_EDGES", HS_FLK_MAX_EDGES); kv("HS_FLK_MAX_NODES", HS_FLK_MAX_NODES); kv("HS_FLK_MAX_RECS", HS_FLK_MAX_RECS);
  kv("HS_FLK_MAX_READS", HS_FLK_MAX_READS); kv("HS_FLK_MAX_LEN", HS_FLK_MAX_LEN); kv("HS_FLK_MAX_PATHS", HS_FLK_MAX_PATHS); kv("HS_FLK_MAX_PATH_LEN", HS_FLK_MAX_PATH_LEN);
  kv("lds_bytes", (int64_t)sizeof(hs_flk_lds_t), true);
  s += "}, \"caps\": {";
  kv("edges", caps.max_edges); kv("nodes", caps.max_nodes); kv("recs", caps.max_recs); kv("reads", caps.max_reads); kv("len", caps.max_len); kv("path_len", caps.max_path_len, true);
  s += "}, \"peel_rounds\": " + std::to_string(hs_flk_peel_rounds(caps));
  s += ", \"routes\": [\"device\", \"host\", \"skipped\"], \"fields\": [\"k\", \"edges\", \"nodes\", \"recs\", \"reads\", \"len\", \"path_len\", \"strings\", \"flags\", \"route\"], \"tasks\": [";
  int64_t hit[3] = {0, 0, 0}, sum_ref = 0;
  std::vector<hf::Str> strs;
  bool first = true;
  for (int l = 0; l < T.n_loci; l++)
    for (int f = 0; f < 2; f++)
      for (int sm = 0; sm < T.n_samples[l]; sm++){
        hf::Task K; hf::Sizes Z; int flags = 0, route = 2;
        sum_ref += T.ref[2*l + f].len;
        if (!hf::task_skipped(rq, T, l, f, sm)){
          hf::task_strings(rq, T, l, f, sm, tr->flank_seq_off, tr->flank_seq, strs);
          hf::assemble_task(T.ref[2*l + f], strs, T.kmer[2*l + f], T.max_k[2*l + f], P, K, &Z);
          Z.reads = T.run_len[(size_t)(T.samp_off[l] + sm)];
          flags = hs_flk_task_flags(T.kmer[2*l + f], T.max_k[2*l + f], P.max_paths, Z.edges, Z.nodes, Z.recs, Z.reads, Z.len, Z.path_len, Z.bad_byte, caps);
          route = flags ? 1 : 0;
        }
        hit[route]++;
        s += std::string(first ? "" : ", ") + "[" + std::to_string(K.k) + ", " + std::to_string(Z.edges) + ", " + std::to_string(Z.nodes) + ", " + std::to_string(Z.recs) + ", " +
             std::to_string(Z.reads) + ", " + std::to_string(Z.len) + ", " + std::to_string(Z.path_len) + ", " + std::to_string(Z.strings) + ", " + std::to_string(flags) + ", " + std::to_string(route) + "]";
        first = false;
      }
  s += "], \"routes_hit\": [" + std::to_string(hit[0]) + ", " + std::to_string(hit[1]) + ", " + std::to_string(hit[2]) + "]";
  s += ", \"pool_bytes\": " + std::to_string(hs_flk_pool_bytes(T.n_tasks(), sum_ref)) + ", \"workgroups\": " + std::to_string(T.n_tasks()) + "}";
  if (cap > 0){ const size_t m = std::min(s.size(), (size_t)cap - 1); memcpy(json, s.data(), m); json[m] = 0; }
  return (int)s.size();
}
#endif  // HIPSTR_NO_DEBUG_ABI
