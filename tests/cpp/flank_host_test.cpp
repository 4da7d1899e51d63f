// flank_host_test.cpp — a stand-alone program over the host twin of the flank reassembly (hipstr_amd/csrc/flank_host.cpp) and over the
// device's task body run as plain C++ (hipstr_amd/csrc/flank_task.h with HS_FLK_SIMULATE: the lanes of a phase run one after the other).
//   flank_host_test cases IN OUT   assembles the cases of a text file (tests/flank_cases.py writes it; the format the reference-driven
//                                  golden generator reads) with the host twin, writes the records in the golden's format, and requires the
//                                  simulated device task to give the same records for every task it does not flag
//   flank_host_test self           the restated libstdc++ sift loops against std::push_heap / std::pop_heap on sequences with ties; random
//                                  tasks, host twin against simulated device task, with the compiled caps and with shrunk ones (the flags
//                                  must be the ones hs_flk_task_flags predicts from the host twin's sizes)
// Built and run by tests/test_flank_host.py with -fsanitize=address,undefined.
#define HS_FLK_SIMULATE
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hipstr_amd/csrc/flank_host.h"
#include "../../hipstr_amd/csrc/flank_task.h"

namespace hf = hipstr_flank;

static int g_failed, g_compared = 0, g_multi = 0, g_cyclic = 0, g_escalated = 0;
#define CHECK(cond, ...) do { if (!(cond)){ g_failed++; fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed*0x9E3779B97F4A7C15ull + 0x1234567ull) {}
  uint64_t next(){ s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
  int below(int n){ return (int)(next() % (uint64_t)n); }
};

// the device's task on host arrays: one sample whose reads are the strings, every one with a seed and a request of its own
struct SimResult { int k, flag; std::vector<std::string> paths; std::vector<int> weights; int sizes[HS_FLK_SIZES]; };
static SimResult simulate(const std::string& ref, const std::vector<std::string>& strings, int k0, int max_k, const hf::Params& P, const hs_flk_caps_t& caps, int flank){
  const int n = (int)strings.size();
  hs_post_unit_t unit; memset(&unit, 0, sizeof unit); unit.read_begin = 0; unit.n_reads = n;
  std::vector<int32_t> seed((size_t)n + 1, 5), rreq((size_t)n + 1), foff(2*(size_t)n + 1, 0);
  std::string fseq;
  for (int i = 0; i < n; i++){
    rreq[i] = i;
    foff[2*i] = (int32_t)fseq.size();
    if (flank == 0) fseq += strings[i];
    foff[2*i + 1] = (int32_t)fseq.size();
    if (flank == 1) fseq += strings[i];
  }
  foff[2*n] = (int32_t)fseq.size();
  fseq.push_back('?');
  const int32_t task_unit[1] = {0}, task_lf[1] = {flank}, kmer0[2] = {k0, k0}, maxk[2] = {max_k, max_k};
  const int32_t ref_off[3] = {0, flank == 0 ? (int32_t)ref.size() : 0, (int32_t)ref.size()};
  const uint8_t skip[1] = {0};
  int32_t tk[1] = {-99}, tf[1] = {-99}, tn[1] = {-99}, ta[1] = {-99}, tsz[HS_FLK_SIZES];
  std::vector<int32_t> pool_words(1 << 14);
  char* pool = (char*)pool_words.data();
  unsigned long long used = 40;                               // (other tasks took their pieces before)
  hs_flk_dev_t d; memset(&d, 0, sizeof d);
  d.units = &unit; d.task_unit = task_unit; d.task_lf = task_lf; d.task_skip = skip; d.ref_off = ref_off; d.ref_seq = ref.data(); d.kmer0 = kmer0; d.max_k = maxk;
  d.seed = seed.data(); d.read_req = rreq.data(); d.flank_off = foff.data(); d.flank_seq = fseq.data(); d.flank_total = (int64_t)fseq.size() - 1;
  d.task_k = tk; d.task_flag = tf; d.task_np = tn; d.task_size = tsz; d.task_at = ta;
  d.pool = pool; d.pool_used = &used; d.pool_cap = (int64_t)pool_words.size()*4; d.n_tasks = 1; d.min_path_weight = P.min_path_weight; d.max_paths = P.max_paths; d.caps = caps;
  static hs_flk_lds_t L;
  memset(&L, 0xA5, sizeof L);                                  // LDS starts with whatever it held
  hs_flk_task(d, 0, L);
  SimResult R; R.k = tk[0]; R.flag = tf[0];
  for (int i = 0; i < HS_FLK_SIZES; i++) R.sizes[i] = tsz[i];
  int at = ta[0];
  for (int i = 0; i < tn[0]; i++){
    int32_t head[2]; memcpy(head, pool + at, 8);
    R.paths.emplace_back(pool + at + 8, (size_t)head[1]); R.weights.push_back(head[0]);
    at += hs_flk_path_bytes(head[1]);
  }
  if (!tf[0] && (unsigned long long)at != (tn[0] ? used : (unsigned long long)at)){ g_failed++; fprintf(stderr, "FAILED: the task's piece of the pool does not end where the pool does\n"); }
  return R;
}

static void compare(const char* what, const std::string& ref, const std::vector<std::string>& strings, const hf::Params& P, const hs_flk_caps_t& caps, int flank,
                    hf::Task* host_out = NULL, int* n_flagged = NULL){
  const hf::Str r = { ref.data(), (int)ref.size() };
  const int max_k = hf::max_k_of(r.len, P.max_kmer), k0 = hf::kmer_length(r, P.min_kmer, max_k);
  std::vector<hf::Str> strs;
  for (const std::string& s : strings) if (!s.empty()) strs.push_back(hf::Str{ s.data(), (int)s.size() });
  hf::Task T; hf::Sizes Z;
  if (k0 >= 0) hf::assemble_task(r, strs, k0, max_k, P, T, &Z);
  if (host_out) *host_out = T;
  if (k0 < 0) return;                                          // no task is launched for a flank without k
  Z.reads = (int)strings.size();
  const int want_flags = hs_flk_task_flags(k0, max_k, P.max_paths, Z.edges, Z.nodes, Z.recs, Z.reads, Z.len, Z.path_len, Z.bad_byte, caps);
  const SimResult S = simulate(ref, strings, k0, max_k, P, caps, flank);
  CHECK((S.flag != 0) == (want_flags != 0), "%s: flags %d, predicted %d (edges %d nodes %d recs %d len %d)", what, S.flag, want_flags, Z.edges, Z.nodes, Z.recs, Z.len);
  if (S.flag){ if (n_flagged) ++*n_flagged; return; }
  g_compared++; g_multi += T.paths.size() > 1; g_cyclic += T.k < 0; g_escalated += T.k > k0;
  CHECK(S.k == T.k, "%s: k %d != %d", what, S.k, T.k);
  CHECK(S.paths == T.paths, "%s: paths differ (%zu vs %zu)", what, S.paths.size(), T.paths.size());
  CHECK(S.weights == T.weights, "%s: weights differ", what);
  CHECK(S.sizes[0] == Z.edges && S.sizes[1] == Z.nodes && (T.k < 0 || S.sizes[2] == Z.recs) && S.sizes[3] == Z.strings, "%s: sizes %d %d %d %d vs %d %d %d %d", what,
        S.sizes[0], S.sizes[1], S.sizes[2], S.sizes[3], Z.edges, Z.nodes, Z.recs, Z.strings);
}

static void heap_selftest(){
  Rng rng(11);
  for (int round = 0; round < 300; round++){
    std::vector<int32_t> rw; std::vector<uint16_t> mine; std::vector<int> theirs;
    auto cmp = [&](int a, int b){ return rw[a] < rw[b]; };
    const int span = 1 + rng.below(4);                         // few distinct weights: ties everywhere
    for (int step = 0; step < 200; step++){
      if (mine.empty() || rng.below(3) != 0){
        rw.push_back(rng.below(span));
        const uint16_t v = (uint16_t)(rw.size() - 1);
        mine.push_back(v); flk_push_heap(mine.data(), rw.data(), (int)mine.size() - 1, 0, v);
        theirs.push_back(v); std::push_heap(theirs.begin(), theirs.end(), cmp);
      } else {
        flk_pop_heap(mine.data(), rw.data(), (int)mine.size()); const int a = mine.back(); mine.pop_back();
        std::pop_heap(theirs.begin(), theirs.end(), cmp); const int b = theirs.back(); theirs.pop_back();
        CHECK(a == b, "heap pop %d != %d", a, b);
      }
      bool same = mine.size() == theirs.size();
      for (size_t i = 0; same && i < mine.size(); i++) same = mine[i] == theirs[i];
      CHECK(same, "heap arrays differ at round %d step %d", round, step);
      if (!same) return;
    }
  }
}

static std::string random_seq(Rng& rng, int n){ std::string s; for (int i = 0; i < n; i++) s.push_back("ACGT"[rng.below(4)]); return s; }

static void random_selftest(){
  Rng rng(2024);
  const hf::Params P = { 10, 15, 2, 10 };
  const hs_flk_caps_t full = hs_flk_default_caps();
  int flagged_full = 0, flagged_small = 0, n = 0;
  for (int it = 0; it < 400; it++){
    const int len = 20 + rng.below(21);
    std::string ref = random_seq(rng, len);
    if (it % 7 == 0){ const std::string unit = random_seq(rng, 1 + rng.below(4)); ref.clear(); while ((int)ref.size() < len) ref += unit; ref.resize((size_t)len); }      // repetitive
    if (it % 5 == 1){ const int n = 10 + rng.below(4), b = rng.below(len - n + 1); ref += ref.substr((size_t)b, (size_t)n); }      // a repeat of 10-13 bases: the first k is above 10
    std::vector<std::string> alleles(1, ref);
    for (int a = rng.below(4); a > 0; a--){
      std::string m = ref;
      for (int e = 1 + rng.below(3); e > 0; e--){
        const int p = rng.below((int)m.size()), kind = rng.below(10);
        if (kind < 6) m[p] = "ACGTN"[rng.below(5)]; else if (kind < 8) m.erase((size_t)p, 1); else if (kind < 9) m.insert((size_t)p, 1, "ACGT"[rng.below(4)]);
        else { const int n = 11 + rng.below(8), b = rng.below(std::max(1, (int)m.size() - n)); m.insert((size_t)b, m.substr((size_t)b, (size_t)n)); }      // a tandem copy: a cycle below its length
      }
      alleles.push_back(m);
    }
    std::vector<std::string> strings;
    for (int s = rng.below(17); s > 0; s--){
      const std::string& a = alleles[(size_t)rng.below((int)alleles.size())];
      const int b = rng.below(3) ? 0 : rng.below((int)a.size()), e = rng.below(3) ? (int)a.size() : b + rng.below((int)a.size() - b + 1);
      strings.push_back(a.substr((size_t)b, (size_t)(e - b)));
    }
    char what[64]; snprintf(what, sizeof what, "random %d", it);
    compare(what, ref, strings, P, full, it & 1, NULL, &flagged_full);
    hs_flk_caps_t small = full;
    small.max_edges = 24 + rng.below(30); small.max_nodes = 24 + rng.below(30); small.max_recs = 20 + rng.below(60); small.max_reads = 4 + rng.below(14);
    small.max_len = 30 + rng.below(12); small.max_path_len = 30 + rng.below(12);
    compare(what, ref, strings, P, small, it & 1, NULL, &flagged_small);
    n++;
  }
  printf("random tasks: %d compared on both sides, %d with more than one path, %d cyclic, %d accepted above the first k\n", g_compared, g_multi, g_cyclic, g_escalated);
  CHECK(g_multi > 40 && g_cyclic > 5 && g_escalated > 5, "the random tasks do not reach every branch");
  CHECK(flagged_full == 0, "%d of %d random tasks left the device under the compiled caps", flagged_full, n);
  CHECK(flagged_small > n/10 && flagged_small < n, "%d of %d random tasks left the device under shrunk caps", flagged_small, n);
  // a byte the device does not pack, and k beyond what it packs
  int fl = 0;
  compare("lower case", "ACGTTGCATGCCATGACTGACTTGA", { "ACGTTGCATGCCaTGACTGACTTGA" }, P, full, 0, NULL, &fl);
  CHECK(fl == 1, "a lower-case base must leave the device");
  const hf::Params wide = { 10, 20, 2, 10 };
  fl = 0;
  compare("max_kmer 20", "ACGTTGCATGCCATGACTGACTTGA", { "ACGTTGCATGCCATGACTGACTTGA" }, wide, full, 0, NULL, &fl);
  CHECK(fl == 1, "k up to 20 must leave the device");
}

static int run_cases(const char* in_path, const char* out_path){
  std::ifstream in(in_path);
  FILE* out = fopen(out_path, "w");
  if (!in || !out){ fprintf(stderr, "cannot open %s / %s\n", in_path, out_path); return 2; }
  std::string line;
  const hs_flk_caps_t full = hs_flk_default_caps();
  auto seq = [](const std::string& s){ return s == "-" ? std::string() : s; };
  while (std::getline(in, line)){
    if (line.empty()) continue;
    std::istringstream hd(line);
    std::string word, name; hf::Params P; int n_samples = 0;
    hd >> word >> name >> P.min_kmer >> P.max_kmer >> P.min_path_weight >> P.max_paths >> n_samples;
    if (word != "case" || !hd){ fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
    std::string ref;
    std::getline(in, line); { std::istringstream ls(line); ls >> word >> ref; ref = seq(ref); }
    const hf::Str r = { ref.data(), (int)ref.size() };
    const int max_k = hf::max_k_of(r.len, P.max_kmer), k0 = hf::kmer_length(r, P.min_kmer, max_k);
    fprintf(out, "case %s kmer %d\n", name.c_str(), k0);
    for (int s = 0; s < n_samples; s++){
      int n = 0;
      std::getline(in, line); { std::istringstream ls(line); ls >> word >> n; }
      std::vector<std::string> strings((size_t)n);
      for (int i = 0; i < n; i++){ std::getline(in, line); strings[i] = seq(line); }
      if (k0 < 0) continue;                                    // assemble_flanks returns before any task
      hf::Task T;
      compare((name + " sample " + std::to_string(s)).c_str(), ref, strings, P, full, s & 1, &T);
      fprintf(out, "task %d k %d n %zu\n", s, T.k, T.paths.size());
      for (size_t i = 0; i < T.paths.size(); i++) fprintf(out, "path %d %s\n", T.weights[i], T.paths[i].c_str());
    }
  }
  fclose(out);
  return 0;
}

int main(int argc, char** argv){
  int rc = 0;
  if (argc == 4 && !strcmp(argv[1], "cases")) rc = run_cases(argv[2], argv[3]);
  else if (argc == 2 && !strcmp(argv[1], "self")){ heap_selftest(); random_selftest(); }
  else { fprintf(stderr, "usage: %s cases IN OUT | self\n", argv[0]); return 2; }
  if (rc) return rc;
  if (g_failed){ fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
  printf("ok\n");
  return 0;
}
