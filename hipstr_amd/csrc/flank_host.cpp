// flank_host.cpp — the host twin of the flank reassembly (plain C++, no HIP): SeqStutterGenotyper::assemble_flanks
// (seq_stutter_genotyper.cpp:40-217) over a restatement of DebruijnGraph / DirectedGraph (debruijn_graph.cpp, directed_graph.cpp).
// What the result depends on is kept literally: node and edge ids in order of first occurrence (reference flank first, then the strings in
// read order), a node's departing edges in edge-id order, the pruning threshold max(2, ceil(0.02 * strings)) on non-reference edges, the
// 1-mismatch sources and sinks over A/C/G/T, and a max-heap on min_weight driven by std::push_heap / std::pop_heap with the reference's
// comparator shape, so that ties fall as libstdc++ lets them fall there.
#include "flank_host.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <unordered_map>

namespace hipstr_flank {
namespace {

struct Graph {
  int k;
  std::unordered_map<std::string, int> ids;
  std::vector<std::string> labels;
  struct Edge { int src, dst, w; bool ref, keep; };
  std::vector<Edge> edges;
  std::vector<std::vector<int> > dep, arr;       // per node: edge ids in insertion order
  std::vector<char> live;
  int n_strings = 0;

  explicit Graph(int k_) : k(k_) {}
  int node(const std::string& s){
    auto it = ids.find(s);
    if (it != ids.end()) return it->second;
    const int id = (int)labels.size();
    ids.emplace(s, id); labels.push_back(s); dep.emplace_back(); arr.emplace_back();
    return id;
  }
  int find(const std::string& s) const { auto it = ids.find(s); return it == ids.end() ? -1 : it->second; }
  // DebruijnGraph::add_string + DirectedGraph::increment_edge
  void add(Str s, int w, bool is_ref){
    if (s.len <= k) return;
    n_strings++;
    std::string prev(s.p, (size_t)k);
    for (int i = 1; i < s.len + 1 - k; i++){
      std::string next(s.p + i, (size_t)k);
      const int a = node(prev), b = node(next);
      bool found = false;
      for (int e : arr[b]) if (edges[e].src == a){ edges[e].w += w; found = true; break; }
      if (!found){
        const int e = (int)edges.size();
        edges.push_back(Edge{a, b, w, is_ref, true});
        dep[a].push_back(e); arr[b].push_back(e);
      }
      prev.swap(next);
    }
  }
  // prune_edges(0.02, 2): edges leave their nodes' lists in place (Node::remove_edge keeps the order); nodes without an edge die, the
  // source and the sink stay
  void prune(int src, int snk){
    int thr = (int)ceil(0.02*n_strings);
    if (thr < 2) thr = 2;
    for (Edge& e : edges) e.keep = e.ref || e.w >= thr;
    for (auto* lists : { &dep, &arr })
      for (std::vector<int>& v : *lists) v.erase(std::remove_if(v.begin(), v.end(), [&](int e){ return !edges[e].keep; }), v.end());
    live.assign(labels.size(), 0);
    if (src >= 0) live[src] = 1;
    if (snk >= 0) live[snk] = 1;
    for (const Edge& e : edges) if (e.keep){ live[e.src] = 1; live[e.dst] = 1; }
  }
  void all_live(){ live.assign(labels.size(), 1); }
  // !can_sort_topologically(): Kahn over the live nodes (the verdict does not depend on the order)
  bool has_cycles() const {
    std::vector<int> indeg(labels.size(), 0), todo;
    size_t n_live = 0, seen = 0;
    for (size_t n = 0; n < labels.size(); n++) if (live[n]){ n_live++; indeg[n] = (int)arr[n].size(); if (!indeg[n]) todo.push_back((int)n); }
    while (!todo.empty()){
      const int n = todo.back(); todo.pop_back(); seen++;
      for (int e : dep[n]) if (--indeg[edges[e].dst] == 0) todo.push_back(edges[e].dst);
    }
    return seen != n_live;
  }
  // get_alt_kmer_nodes
  void alts(std::string kmer, bool source, std::vector<int>& out) const {
    static const char bases[4] = {'A', 'C', 'G', 'T'};
    for (size_t i = 0; i < kmer.size(); i++){
      const char orig = kmer[i];
      for (int j = 0; j < 4; j++){
        if (bases[j] == orig) continue;
        kmer[i] = bases[j];
        const int n = find(kmer);
        if (n < 0 || !live[n]) continue;
        if (source ? !arr[n].empty() : !dep[n].empty()) continue;
        out.push_back(n);
      }
      kmer[i] = orig;
    }
  }
};

struct Path { int node, parent, min_w; };

// DebruijnGraph::enumerate_paths; the sequence is the first node's label and the last base of every later node, which equals
// DebruijnPath::get_sequence's string for any path of a De Bruijn graph
void enumerate(const Graph& G, int src, int snk, const std::string& src_kmer, const std::string& snk_kmer, const Params& P, Task& out, int* n_recs){
  std::vector<Path> all;
  std::vector<int> heap;
  auto cmp = [&](int a, int b){ return all[a].min_w < all[b].min_w; };      // path_comparator
  all.push_back(Path{src, -1, 1000000}); heap.push_back(0);
  std::make_heap(heap.begin(), heap.end(), cmp);
  std::vector<int> alt_src, alt_snk;
  G.alts(src_kmer, true, alt_src);
  for (int n : alt_src){ all.push_back(Path{n, -1, 1000000}); heap.push_back((int)all.size() - 1); std::push_heap(heap.begin(), heap.end(), cmp); }
  G.alts(snk_kmer, false, alt_snk);
  std::vector<char> is_sink(G.labels.size(), 0);
  is_sink[snk] = 1;
  for (int n : alt_snk) is_sink[n] = 1;
  while (!heap.empty()){
    if ((int)out.paths.size() == P.max_paths) break;
    std::pop_heap(heap.begin(), heap.end(), cmp);
    const int best = heap.back(); heap.pop_back();
    const int node = all[best].node;
    if (is_sink[node]){
      std::string rev;
      for (auto it = G.labels[node].rbegin(); it != G.labels[node].rend(); ++it) rev.push_back(*it);
      for (int p = all[best].parent; p >= 0; p = all[p].parent) rev.push_back(G.labels[all[p].node][0]);
      std::reverse(rev.begin(), rev.end());
      out.paths.push_back(rev); out.weights.push_back(all[best].min_w);
    }
    for (int e : G.dep[node]){
      if (G.edges[e].w < P.min_path_weight) continue;
      all.push_back(Path{G.edges[e].dst, best, std::min(all[best].min_w, G.edges[e].w)});
      heap.push_back((int)all.size() - 1);
      std::push_heap(heap.begin(), heap.end(), cmp);
    }
  }
  *n_recs = (int)all.size();
}

bool bad_bytes(Str s){
  for (int i = 0; i < s.len; i++){ const char c = s.p[i]; if (c != 'A' && c != 'C' && c != 'G' && c != 'T' && c != 'N') return true; }
  return false;
}

}  // namespace

Params params_of(const hipstr_flank_request_t* rq){
  Params P;
  P.min_kmer = rq->min_kmer ? rq->min_kmer : 10; P.max_kmer = rq->max_kmer ? rq->max_kmer : 15;
  P.min_path_weight = rq->min_path_weight ? rq->min_path_weight : 2; P.max_paths = rq->max_paths ? rq->max_paths : 10;
  return P;
}

int max_k_of(int ref_len, int max_kmer){ const int m = ref_len == 0 ? -1 : ref_len - 1; return std::min(max_kmer, m); }

int kmer_length(Str ref, int min_kmer, int max_k){
  if (min_kmer < 1) return -1;
  for (int k = min_kmer; k <= max_k; k++){
    Graph G(k);
    G.add(ref, 2, true);
    G.all_live();
    if (!G.has_cycles()) return k;
  }
  return -1;
}

void assemble_task(Str ref, const std::vector<Str>& strings, int k0, int max_k, const Params& P, Task& out, Sizes* sz){
  out = Task();
  out.k = HIPSTR_FLANK_TASK_CYCLIC;
  if (k0 < 1) return;
  for (int k = k0; k <= max_k; k++){
    Graph G(k);
    G.add(ref, 2, true);
    for (const Str& s : strings) if (s.len > 0) G.add(s, 1, false);
    if (sz){
      sz->edges = std::max(sz->edges, (int)G.edges.size()); sz->nodes = std::max(sz->nodes, (int)G.labels.size());
      sz->len = std::max(sz->len, ref.len); sz->strings = G.n_strings - 1;
      if (bad_bytes(ref)) sz->bad_byte = 1;
      for (const Str& s : strings) if (s.len > k){ sz->len = std::max(sz->len, s.len); if (bad_bytes(s)) sz->bad_byte = 1; }
    }
    const std::string src_kmer(ref.p, (size_t)k), snk_kmer(ref.p + ref.len - k, (size_t)k);
    const int src = G.find(src_kmer), snk = G.find(snk_kmer);
    G.prune(src, snk);
    if (G.has_cycles()) continue;
    if (!(G.dep[src].size() > 0 && G.arr[src].empty())) continue;          // is_source_ok
    if (!(G.arr[snk].size() > 0 && G.dep[snk].empty())) continue;          // is_sink_ok
    out.k = k;
    int n_recs = 0;
    enumerate(G, src, snk, src_kmer, snk_kmer, P, out, &n_recs);
    if (sz){ sz->recs = n_recs; for (const std::string& p : out.paths) sz->path_len = std::max(sz->path_len, (int)p.size()); }
    return;
  }
}

bool null_request(const hipstr_flank_request_t* rq){
  if (!rq || !rq->pooled || !rq->seed || !rq->read_req || !rq->pool_index) return true;
  const hipstr_batch_t* b = rq->pooled;
  return b->n_loci < 0 || (b->n_loci && (!b->blk_nopts || !b->opt_off || !b->seq || !b->hap_off || !b->read_off)) || (rq->n_req > 0 && !rq->req_read);
}

std::string check_tables(const hipstr_flank_request_t* rq, Tables& T){
  const hipstr_batch_t* b = rq->pooled;
  const int nl = T.n_loci;
  if (b->n_loci != nl) return "hipstr_flank_assemble: pooled->n_loci differs from the posterior batch's";
  if (rq->n_req < 0) return "hipstr_flank_assemble: negative n_req";
  const int32_t nq = rq->n_req;
  T.req_locus.resize((size_t)nq);
  {
    int l = 0;
    const int32_t n_pooled = nl ? b->read_off[nl] : 0;
    for (int32_t q = 0; q < nq; q++){
      const int32_t pr = rq->req_read[q];
      if (pr < 0 || pr >= n_pooled) return "hipstr_flank_assemble: req_read outside the pooled reads";
      while (l < nl && pr >= b->read_off[l+1]) l++;
      if (pr < b->read_off[l]) return "hipstr_flank_assemble: requests must be grouped by locus, in locus order";
      T.req_locus[q] = l;
    }
  }
  for (int l = 0; l < nl; l++){
    const int32_t P = b->read_off[l+1] - b->read_off[l];
    for (int r = T.read_off[l]; r < T.read_off[l+1]; r++){
      const int32_t q = rq->read_req[r];
      if (q < -1 || q >= nq) return "hipstr_flank_assemble: read_req outside [-1, n_req)";
      if (q >= 0 && T.req_locus[q] != l) return "hipstr_flank_assemble: a read's request belongs to another locus";
      if (rq->pool_index[r] < 0 || rq->pool_index[r] >= P) return "hipstr_flank_assemble: pool_index outside the locus' pooled reads";
    }
  }
  const Params P = params_of(rq);
  T.ref.resize(2*(size_t)nl); T.kmer.resize(2*(size_t)nl); T.max_k.resize(2*(size_t)nl);
  int64_t oi = 0;
  for (int l = 0; l < nl; l++){
    for (int blk = 0; blk < 3; blk++){
      const int no = b->blk_nopts[3*l + blk];
      if (no < 1) return "hipstr_flank_assemble: a block without options";
      if (blk != 1){
        const int f = blk == 0 ? 0 : 1;
        const int len = b->opt_off[oi+1] - b->opt_off[oi];
        if (len < 0) return "hipstr_flank_assemble: opt_off decreases";
        T.ref[2*l + f] = Str{ b->seq + b->opt_off[oi], len };
        T.max_k[2*l + f] = max_k_of(len, P.max_kmer);
        T.kmer[2*l + f] = kmer_length(T.ref[2*l + f], P.min_kmer, T.max_k[2*l + f]);
      }
      oi += no;
    }
  }
  return "";
}

bool task_skipped(const hipstr_flank_request_t* rq, const Tables& T, int l, int flank, int s){
  return T.kmer[2*l + flank] < 0 || (rq->sample_masked && rq->sample_masked[T.samp_off[l] + s]);
}

void task_strings(const hipstr_flank_request_t* rq, const Tables& T, int l, int flank, int s, const int32_t* flank_off, const char* flank_seq, std::vector<Str>& out){
  out.clear();
  const int64_t slot = T.samp_off[l] + s;
  for (int r = T.run_begin[slot]; r < T.run_begin[slot] + T.run_len[slot]; r++){
    if (rq->seed[r] < 0) continue;                              // traced_alns[r] == NULL
    const int q = rq->read_req[r];
    if (q < 0) continue;
    const int o = flank_off[2*q + flank], len = flank_off[2*q + flank + 1] - o;
    if (len > 0) out.push_back(Str{ flank_seq + o, len });
  }
}

namespace {
struct LocusOut { int status = 0; int64_t new_n_haps = 0; std::vector<std::string> opts[2]; std::vector<int> counts[2]; };

// :46-180 for one locus; st / realign: [S]
void aggregate_locus(const hipstr_flank_request_t* rq, const Tables& T, int l, std::vector<Task>& tasks, uint8_t* st, uint8_t* realign, LocusOut& O){
  const hipstr_batch_t* b = rq->pooled;
  const int S = T.n_samples[l];
  int64_t new_total = b->hap_off[l+1] - b->hap_off[l];
  for (int flank = 0; flank < 2; flank++){
    const Str ref = T.ref[2*l + flank];
    new_total /= b->blk_nopts[3*l + (flank == 0 ? 0 : 2)];
    O.new_n_haps = new_total;
    if (T.kmer[2*l + flank] < 0){ O.status = 1; return; }
    std::map<std::string, int> index;
    std::vector<std::vector<int> > hap_samples;
    for (int s = 0; s < S; s++){
      Task& tk = tasks[(size_t)T.task_of(l, flank, s)];
      const bool masked = rq->sample_masked && rq->sample_masked[T.samp_off[l] + s];
      if (masked || st[s] != HIPSTR_FLANK_OK){ tk = Task(); continue; }      // !call_sample_[s].empty()
      if (tk.k < 0){ st[s] = HIPSTR_FLANK_ASSEMBLY_CYCLIC; tk.k = HIPSTR_FLANK_TASK_CYCLIC; continue; }
      if (tk.paths.size() <= 1) continue;
      int total_depth = 0;
      for (int w : tk.weights) total_depth += w;
      for (size_t i = 0; i < tk.paths.size(); i++){
        const std::string& seq = tk.paths[i];
        if ((int)seq.size() == ref.len && memcmp(seq.data(), ref.p, seq.size()) == 0) continue;
        if (!(tk.weights[i]*1.0/total_depth > 0.25)) continue;
        if ((int)seq.size() != ref.len){ st[s] = HIPSTR_FLANK_ASSEMBLY_INDEL; realign[s] = 0; }
        else {
          auto it = index.find(seq);
          if (it == index.end()){ it = index.emplace(seq, (int)index.size()).first; hap_samples.emplace_back(); }
          realign[s] = 1;
          hap_samples[it->second].push_back(s);
        }
      }
    }
    for (auto it = index.begin(); it != index.end(); ){
      const std::vector<int>& hs = hap_samples[it->second];
      if (hs.size() < rq->min_flank_freq*S){
        for (int s : hs) if (st[s] == HIPSTR_FLANK_OK){ st[s] = HIPSTR_FLANK_LOW_FREQUENCY_ALT; realign[s] = 0; }
        index.erase(it++);
      } else ++it;
    }
    if (!index.empty()){
      if (index.size() > (size_t)rq->max_flank_haplotypes){ O.status = 2; return; }
      for (auto& kv : index){ O.opts[flank].push_back(kv.first); O.counts[flank].push_back((int)hap_samples[kv.second].size()); }
      new_total *= (int64_t)(1 + index.size());
      O.new_n_haps = new_total;
    }
  }
  if (new_total > rq->max_total_haplotypes) O.status = 3;
}
}  // namespace

int finish(const hipstr_flank_request_t* rq, const Tables& T, std::vector<Task>& tasks, hipstr_flank_out_t* out){
  const hipstr_batch_t* b = rq->pooled;
  const int nl = T.n_loci;
  const int64_t n_samp = T.n_samp();
  std::vector<uint8_t> st((size_t)n_samp, 0), realign((size_t)n_samp, 0);
  std::vector<LocusOut> loci((size_t)nl);
  int64_t n_opts = 0, opt_chars = 0, n_paths = 0, path_chars = 0;
  for (int l = 0; l < nl; l++){
    LocusOut& O = loci[l];
    uint8_t* ls = st.data() + T.samp_off[l]; uint8_t* lr = realign.data() + T.samp_off[l];
    aggregate_locus(rq, T, l, tasks, ls, lr, O);
    if (O.status != 0){                                        // a failed locus: nothing but the status
      for (int s = 0; s < T.n_samples[l]; s++){ ls[s] = 0; lr[s] = 0; }
      O.opts[0].clear(); O.opts[1].clear(); O.counts[0].clear(); O.counts[1].clear();
    }
    for (int f = 0; f < 2; f++){ n_opts += (int64_t)O.opts[f].size(); for (const std::string& s : O.opts[f]) opt_chars += (int64_t)s.size(); }
  }
  for (const Task& tk : tasks){ n_paths += (int64_t)tk.paths.size(); for (const std::string& s : tk.paths) path_chars += (int64_t)s.size(); }
  const bool want_paths = out->path_weight || out->path_seq_off || out->path_seq;
  if (n_opts > out->cap_opts || opt_chars > out->cap_opt_chars || (want_paths && n_paths > out->cap_paths) || (out->path_seq && path_chars > out->cap_path_chars)){
    int32_t n = 0;
    for (int l = 0; l < nl; l++) for (int f = 0; f < 2; f++){ out->opt_off[2*l + f] = n; n += (int32_t)loci[l].opts[f].size(); }
    out->opt_off[2*nl] = n;
    out->cap_opts = (int32_t)n_opts; out->cap_opt_chars = (int32_t)opt_chars; out->cap_paths = (int32_t)n_paths; out->cap_path_chars = (int32_t)path_chars;
    return 3;
  }
  int32_t n = 0, c = 0;
  out->opt_seq_off[0] = 0;
  for (int l = 0; l < nl; l++){
    out->status[l] = loci[l].status; out->new_n_haps[l] = loci[l].new_n_haps;
    for (int f = 0; f < 2; f++){
      out->opt_off[2*l + f] = n;
      for (size_t i = 0; i < loci[l].opts[f].size(); i++){
        const std::string& s = loci[l].opts[f][i];
        memcpy(out->opt_seq + c, s.data(), s.size()); c += (int32_t)s.size();
        out->opt_n_samples[n] = loci[l].counts[f][i];
        out->opt_seq_off[++n] = c;
      }
    }
  }
  out->opt_off[2*nl] = n;
  if (n_samp){ memcpy(out->sample_status, st.data(), (size_t)n_samp); memcpy(out->realign_sample, realign.data(), (size_t)n_samp); }
  // realign_pools / copy_reads (:185-191)
  const int32_t n_pooled = nl ? b->read_off[nl] : 0;
  if (n_pooled) memset(out->realign_pool, 0, (size_t)n_pooled);
  for (int l = 0; l < nl; l++)
    for (int s = 0; s < T.n_samples[l]; s++){
      const int64_t slot = T.samp_off[l] + s;
      const uint8_t flag = realign[(size_t)slot];
      for (int r = T.run_begin[slot]; r < T.run_begin[slot] + T.run_len[slot]; r++){
        out->copy_read[r] = flag;
        if (flag) out->realign_pool[b->read_off[l] + rq->pool_index[r]] = 1;
      }
    }
  int32_t np = 0, pc = 0;
  if (out->path_seq_off) out->path_seq_off[0] = 0;
  for (size_t t = 0; t < tasks.size(); t++){
    const Task& tk = tasks[t];
    if (out->task_k) out->task_k[t] = tk.k;
    if (out->task_n_paths) out->task_n_paths[t] = (int32_t)tk.paths.size();
    for (size_t i = 0; i < tk.paths.size(); i++){
      if (out->path_weight) out->path_weight[np] = tk.weights[i];
      if (out->path_seq) memcpy(out->path_seq + pc, tk.paths[i].data(), tk.paths[i].size());
      pc += (int32_t)tk.paths[i].size(); np++;
      if (out->path_seq_off) out->path_seq_off[np] = pc;
    }
  }
  return 0;
}

}  // namespace hipstr_flank
