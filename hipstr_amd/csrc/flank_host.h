// flank_host.h — the host twin of the flank reassembly (flank_host.cpp; plain C++, no HIP): DebruijnGraph restated (graph, pruning, Kahn's
// test, source / sink checks, the path enumeration on std::push_heap / std::pop_heap), calc_kmer_length, and the ONE aggregation
// (seq_stutter_genotyper.cpp:99-201) both entry points run on the per-task records, whichever side assembled them.
#pragma once
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hipstr_hmm.h"

namespace hipstr_flank {

struct Params { int min_kmer, max_kmer, min_path_weight, max_paths; };
Params params_of(const hipstr_flank_request_t* rq);            // 0 = 10 / 15 / 2 / 10

struct Str { const char* p; int len; };

// One task's record: k (HIPSTR_FLANK_TASK_CYCLIC / _SKIPPED) and the sink paths in pop order.
struct Task { int k = HIPSTR_FLANK_TASK_SKIPPED; std::vector<std::string> paths; std::vector<int> weights; };
// What a task needed, over the k it tried (hipstr_debug_flank_plan: the device's limits are decided on these, flank_layout.h): most distinct
// edges and nodes of a graph, path records of the enumeration, reads of the run, the longest string that entered a graph (the reference
// flank included), the longest path, a byte other than ACGTN in a string that entered.
struct Sizes { int edges = 0, nodes = 0, recs = 0, reads = 0, len = 0, path_len = 0, bad_byte = 0, strings = 0; };

// min(max_kmer, len - 1), -1 for an empty ref_seq (:54)
int max_k_of(int ref_len, int max_kmer);
// DebruijnGraph::calc_kmer_length(ref, min_kmer, max_k): the first k whose reference-only graph is acyclic, or -1
int kmer_length(Str ref, int min_kmer, int max_k);
// the loop of :77-96 for one sample: strings in read order (empty ones left out by the caller or not: they never enter)
void assemble_task(Str ref, const std::vector<Str>& strings, int k0, int max_k, const Params& P, Task& out, Sizes* sizes = NULL);

// The tables both entry points check and the aggregation reads.  Runs: per global sample slot the run of its reads.
struct Tables {
  int n_loci = 0;
  const int32_t* n_samples = NULL;                 // [n_loci]
  std::vector<int32_t> read_off;                   // [n_loci+1] un-pooled reads
  std::vector<int32_t> samp_off;                   // [n_loci+1]
  std::vector<int32_t> run_begin, run_len;         // [n_samp]
  std::vector<int32_t> req_locus;                  // [n_req]
  std::vector<Str> ref;                            // [2*n_loci]
  std::vector<int32_t> kmer, max_k;                // [2*n_loci]
  int64_t n_samp() const { return samp_off.empty() ? 0 : samp_off.back(); }
  int64_t n_tasks() const { return 2*n_samp(); }
  int64_t task_of(int l, int flank, int s) const { return 2*(int64_t)samp_off[l] + (int64_t)flank*n_samples[l] + s; }
};
// null arguments of the request (the entry points add their own)
bool null_request(const hipstr_flank_request_t* rq);
// Fills T from the runs already in it (n_loci, n_samples, run_begin, run_len, read_off) and checks the request against it; "" or the refusal.
std::string check_tables(const hipstr_flank_request_t* rq, Tables& T);
// nothing to assemble for this task: a masked sample or a flank without k
bool task_skipped(const hipstr_flank_request_t* rq, const Tables& T, int l, int flank, int s);
// The strings of a task from host flank arrays, in read order.
void task_strings(const hipstr_flank_request_t* rq, const Tables& T, int l, int flank, int s, const int32_t* flank_off, const char* flank_seq, std::vector<Str>& out);

// The aggregation and the outputs: tasks [n_tasks] as assembled (the records of tasks the aggregation ignores are reset to skipped).
// Returns 0, or 3 when a capacity is too small (opt_off and the cap_* fields are then filled).
int finish(const hipstr_flank_request_t* rq, const Tables& T, std::vector<Task>& tasks, hipstr_flank_out_t* out);

}  // namespace hipstr_flank
