// hapgen_host_test.cpp — stand-alone check of the haplotype generator's host twin (hipstr_amd/csrc/hapgen_host.cpp), meant to be built
// with -fsanitize=address,undefined (tests/test_hapgen_host.py does):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=all tests/cpp/hapgen_host_test.cpp hipstr_amd/csrc/hapgen_host.cpp -o hapgen_host_test
// Generated loci (0-150 reads with random = X I D runs around a repeat, starts and ends on either side of the span test, reads that are not
// flagged, samples without reads, lower case, regions at the chromosome's ends, read_stop given or NULL) go through check() and
// hapgen_host() into arrays of EXACTLY the documented sizes, and are compared with a restatement on std::string and std::map that follows
// HaplotypeGenerator.cpp statement by statement.  Then the batch is assembled and its tables checked.  Prints "ok <loci> <reads> <built> <options>".
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../hipstr_amd/csrc/hapgen_host.h"

namespace {

#define CHECK(c) do { if (!(c)){ fprintf(stderr, "hapgen_host_test: %s failed at line %d (case %d, locus %d)\n", #c, __LINE__, g_case, g_locus); exit(1); } } while (0)
int g_case = 0, g_locus = 0;

struct Read { int start, stop, sample; bool use; std::vector<std::pair<char,int>> cigar; std::string seq; };
struct Locus { std::string chrom; int a, b, period, n_samples; std::vector<Read> reads; };

std::string upper(const std::string& s){ std::string o = s; for (char& c : o) if (c >= 'a' && c <= 'z') c = (char)(c - 32); return o; }

// extract_sequence (:82-155) on the gapped alignment string
bool extract(const Read& r, int rs, int re, std::string& seq){
  if (r.start >= rs) return false;
  if (r.stop <= re) return false;
  std::string aln; { size_t k = 0; for (auto& c : r.cigar){ if (c.first == 'D') aln += std::string((size_t)c.second, '-'); else { aln += r.seq.substr(k, (size_t)c.second); k += (size_t)c.second; } } }
  int align_index = 0, char_index = 0, pos = r.start; size_t ci = 0;
  std::string reg;
  while (ci < r.cigar.size()){
    const char op = r.cigar[ci].first; const int num = r.cigar[ci].second;
    if (char_index == num){ ci++; char_index = 0; }
    else if (pos > re){ seq = upper(reg); return true; }
    else if (pos == re){
      if (op == 'I'){ reg += aln.substr((size_t)align_index, (size_t)num); align_index += num; char_index = 0; ci++; }
      else { seq = upper(reg); return true; }
    }
    else if (pos >= rs){
      int nb = std::min(re - pos, num - char_index);
      if (op == 'I'){ nb = num; reg += aln.substr((size_t)align_index, (size_t)nb); }
      else if (op == 'D') pos += nb;
      else { reg += aln.substr((size_t)align_index, (size_t)nb); pos += nb; }
      align_index += nb; char_index += nb;
    }
    else {
      int nb;
      if (op == 'I') nb = num - char_index;
      else { nb = std::min(rs - pos, num - char_index); pos += nb; }
      align_index += nb; char_index += nb;
    }
  }
  CHECK(!"the walk ran off the CIGAR");
  return false;
}

struct Want { int status; int bs[3], be[3]; std::vector<std::string> opts[3]; int tot_reads, tot_samples, distinct; };

Want restate(const Locus& lc){
  Want w; memset(w.bs, 0, sizeof w.bs); memset(w.be, 0, sizeof w.be); w.tot_reads = w.tot_samples = w.distinct = 0;
  long long min_all = INT_MAX, max_all = INT_MIN, min_f = INT_MAX, max_f = INT_MIN;
  for (const Read& r : lc.reads){
    min_all = std::min<long long>(min_all, r.start); max_all = std::max<long long>(max_all, r.stop);
    if (r.use){ min_f = std::min<long long>(min_f, r.start); max_f = std::max<long long>(max_f, r.stop); }
  }
  if (lc.a < 40 || lc.b + 40 > (int)lc.chrom.size()){ w.status = 1; return w; }
  int rs = lc.a - 5, re = lc.b + 5;
  if (min_f + 5 >= rs || max_f - 5 <= re){ w.status = 2; return w; }
  w.status = 0;
  const std::string ref_seq = upper(lc.chrom.substr((size_t)rs, (size_t)(re - rs)));
  std::map<std::string, double> sample_counts; std::map<std::string, int> read_counts, must_inc;
  for (int s = 0; s < lc.n_samples; s++){
    int samp_reads = 0; std::map<std::string, int> counts;
    for (const Read& r : lc.reads){
      if (r.sample != s || !r.use) continue;
      std::string sub;
      if (extract(r, rs, re, sub)){ read_counts[sub]++; counts[sub]++; w.tot_reads++; samp_reads++; }
    }
    for (auto& it : counts){
      if (it.second >= 2.0 && it.second >= 0.2*samp_reads) must_inc[it.first]++;
      sample_counts[it.first] += it.second*1.0/samp_reads;
    }
    if (samp_reads > 0) w.tot_samples++;
  }
  w.distinct = (int)read_counts.size();
  std::vector<std::string> seqs; int ref_index = -1;
  for (auto& it : must_inc)
    if (it.second >= 1){ sample_counts.erase(it.first); read_counts.erase(it.first); seqs.push_back(it.first); if (it.first == ref_seq) ref_index = (int)seqs.size() - 1; }
  for (auto& it : sample_counts)
    if (it.second > 0.05*w.tot_samples || read_counts[it.first] > 0.05*w.tot_reads){ seqs.push_back(it.first); if (ref_index == -1 && it.first == ref_seq) ref_index = (int)seqs.size() - 1; }
  if (ref_index == -1) seqs.insert(seqs.begin(), ref_seq); else { seqs[(size_t)ref_index] = seqs[0]; seqs[0] = ref_seq; }
  std::sort(seqs.begin() + 1, seqs.end(), [](const std::string& x, const std::string& y){ return x.size() != y.size() ? x.size() < y.size() : x.compare(y) < 0; });
  // trim :12-80
  int min_len = INT_MAX; for (auto& s : seqs) min_len = std::min(min_len, (int)s.size());
  const int ideal = 3*lc.period;
  if (min_len > ideal){
    int ml = 0, mr = 0;
    while (ml < min_len - ideal){ size_t j = 1; while (j < seqs.size()){ if (seqs[j][(size_t)ml] != seqs[j-1][(size_t)ml]) break; j++; } if (j != seqs.size()) break; ml++; }
    while (mr < min_len - ideal){ const char c = seqs[0][seqs[0].size()-1-(size_t)mr]; size_t j = 1; while (j < seqs.size()){ if (seqs[j][seqs[j].size()-1-(size_t)mr] != c) break; j++; } if (j != seqs.size()) break; mr++; }
    ml = std::min(5, ml); mr = std::min(5, mr);
    ml = std::max(0, std::min(min_len - 5, ml)); mr = std::max(0, std::min(min_len - 5, mr));
    int lt, rt;
    if (min_len - 2*std::min(ml, mr) <= ideal){ lt = rt = std::min(ml, mr); while (min_len - lt - rt < ideal){ if (lt > rt) lt--; else rt--; } }
    else if (ml > mr){ rt = mr; lt = std::min(ml, min_len - ideal - mr); }
    else { lt = ml; rt = std::min(mr, min_len - ideal - ml); }
    for (auto& s : seqs) s = s.substr((size_t)lt, s.size() - (size_t)lt - (size_t)rt);
    rs += lt; re -= rt;
  }
  const int min_start = (int)std::min<long long>(rs - 10, std::max<long long>(rs - 35, min_all)), max_stop = (int)std::max<long long>(re + 10, std::min<long long>(re + 35, max_all));
  w.bs[0] = min_start; w.be[0] = rs; w.bs[1] = rs; w.be[1] = re; w.bs[2] = re; w.be[2] = max_stop;
  w.opts[0].push_back(upper(lc.chrom.substr((size_t)min_start, (size_t)(rs - min_start))));
  w.opts[1] = seqs;
  w.opts[2].push_back(upper(lc.chrom.substr((size_t)re, (size_t)(max_stop - re))));
  return w;
}

void run_case(std::mt19937_64& rng, int n_loci, int max_reads, bool give_stop, bool give_use, bool want_optional, long totals[4]){
  auto rnd = [&](int lo, int hi){ return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
  auto base = [&](){ return "ACGT"[rng() & 3]; };
  std::vector<Locus> loci((size_t)n_loci);
  for (Locus& lc : loci){
    lc.period = rnd(1, 6);
    const int copies = rnd(2, 9), kind = rnd(0, 11);
    const int left = kind == 0 ? 39 : kind == 1 ? 40 : rnd(60, 150), right = kind == 2 ? 39 : kind == 3 ? 40 : rnd(60, 150);
    std::string motif; for (int i = 0; i < lc.period; i++) motif += base();
    for (int i = 0; i < left; i++) lc.chrom += (rnd(0, 19) == 0 ? "acgtn"[rnd(0, 4)] : base());
    lc.a = left; for (int i = 0; i < copies; i++) lc.chrom += motif; lc.b = (int)lc.chrom.size();
    for (int i = 0; i < right; i++) lc.chrom += base();
    lc.n_samples = rnd(1, 5);
    const int n = rnd(0, 7) == 0 ? rnd(0, 2) : rnd(0, max_reads);
    const int rs = lc.a - 5, re = lc.b + 5, L = (int)lc.chrom.size();
    for (int k = 0; k < n; k++){
      Read r; r.sample = rnd(0, lc.n_samples - 1); r.use = !give_use || rnd(0, 14) != 0;
      r.start = std::max(0, rnd(0, 5) == 0 ? rs - rnd(-3, 3) : rs - rnd(1, 50));
      const int end = std::min(L, rnd(0, 5) == 0 ? re + rnd(-3, 3) : re + rnd(1, 50));
      // runs from start to end: mostly '=', now and then X, I or D — more often near the region's edges
      int pos = r.start; const bool lower = rnd(0, 19) == 0;
      auto push = [&](char op, int len){ if (!r.cigar.empty() && r.cigar.back().first == op && rnd(0, 3)) r.cigar.back().second += len; else r.cigar.push_back({op, len}); };
      while (pos < end){
        const bool edge = std::abs(pos - rs) < 3 || std::abs(pos - re) < 3;
        const int u = rnd(0, edge ? 7 : 39);
        if (u == 0){ const int len = rnd(1, 3); push('I', len); for (int i = 0; i < len; i++) r.seq += base(); }
        else if (u == 1){ const int len = std::min(end - pos, rnd(1, rnd(0, 9) == 0 ? 40 : 4)); push('D', len); pos += len; }
        else if (u == 2){ push('X', 1); r.seq += lc.chrom[(size_t)pos] == 'A' ? 'C' : 'A'; pos++; }
        else { const int len = std::min(end - pos, rnd(1, 12)); push('=', len); r.seq += lc.chrom.substr((size_t)pos, (size_t)len); pos += len; }
      }
      if (pos == end && rnd(0, 9) == 0){ push('I', 2); r.seq += "GT"; }
      if (r.cigar.empty()){ push('=', 1); r.seq += 'A'; pos++; }
      if (lower) for (char& c : r.seq) c = (char)tolower(c);
      r.stop = give_stop ? pos - rnd(0, 1) : pos;
      lc.reads.push_back(r);
    }
  }
  // ---- the flat form, arrays of exactly the documented sizes
  std::vector<int32_t> read_off{0}, base_off{0}, read_start, cigar_off{0}, cigar_len, region_start, region_stop, period, win_off{0}, n_samples, sample_label, read_stop;
  std::vector<int64_t> chrom_len; std::vector<uint8_t> use_read; std::vector<double> stutter; std::string bases, quals, cigar_op, window;
  for (const Locus& lc : loci){
    for (const Read& r : lc.reads){
      bases += r.seq; quals += std::string(r.seq.size(), 'F'); base_off.push_back((int32_t)bases.size()); read_start.push_back(r.start);
      for (auto& c : r.cigar){ cigar_op += c.first; cigar_len.push_back(c.second); }
      cigar_off.push_back((int32_t)cigar_op.size()); sample_label.push_back(r.sample); read_stop.push_back(r.stop); use_read.push_back(r.use ? 1 : 0);
    }
    read_off.push_back((int32_t)read_start.size());
    region_start.push_back(lc.a); region_stop.push_back(lc.b); period.push_back(lc.period); chrom_len.push_back((int64_t)lc.chrom.size()); n_samples.push_back(lc.n_samples);
    if (lc.a >= 40 && lc.b + 40 <= (int)lc.chrom.size()) window += lc.chrom.substr((size_t)(lc.a - 40), (size_t)(lc.b - lc.a + 80));
    win_off.push_back((int32_t)window.size());
    for (int k = 0; k < 6; k++) stutter.push_back(0.01*(k + 1));
  }
  const size_t nl = loci.size(), n = read_start.size();
  read_start.push_back(0); cigar_len.push_back(0); sample_label.push_back(0); read_stop.push_back(0); use_read.push_back(0);      // (never empty: data() stays a pointer)
  hipstr_batch_t b; memset(&b, 0, sizeof b);
  b.n_loci = (int32_t)nl; b.read_off = read_off.data(); b.base_off = base_off.data(); b.bases = bases.data(); b.quals = quals.data(); b.read_start = read_start.data();
  b.cigar_off = cigar_off.data(); b.cigar_op = cigar_op.data(); b.cigar_len = cigar_len.data();
  hipstr_hapgen_request_t rq; memset(&rq, 0, sizeof rq);
  rq.region_start = region_start.data(); rq.region_stop = region_stop.data(); rq.period = period.data(); rq.chrom_len = chrom_len.data(); rq.win_off = win_off.data();
  rq.window = window.data(); rq.n_samples = n_samples.data(); rq.sample_label = sample_label.data(); rq.read_stop = give_stop ? read_stop.data() : NULL;
  rq.use_read = give_use ? use_read.data() : NULL; rq.stutter = stutter.data();
  std::vector<int32_t> status(nl), blk_start(3*nl), blk_end(3*nl), blk_nopts(3*nl), opt_off(3*nl + n + 1), n_spanning(nl), n_ss(nl), n_distinct(nl), lt(nl), rt(nl),
                       mn(nl), mx(nl), ext_off(n), ext_len(n), dist_len(n), dist_rep(n), dist_reads(n), dist_strong(n);
  std::vector<double> dist_frac(n); std::vector<char> seq(window.size() + bases.size());
  int32_t one = 0; char onec = 0;
  auto ptr = [&](std::vector<int32_t>& v){ return v.empty() ? &one : v.data(); };
  hipstr_hapgen_out_t o; memset(&o, 0, sizeof o);
  o.status = ptr(status); o.blk_start = ptr(blk_start); o.blk_end = ptr(blk_end); o.blk_nopts = ptr(blk_nopts); o.opt_off = opt_off.data(); o.seq = seq.empty() ? &onec : seq.data();
  o.n_spanning = ptr(n_spanning); o.n_samples_spanning = ptr(n_ss); o.n_distinct = ptr(n_distinct); o.left_trim = ptr(lt); o.right_trim = ptr(rt);
  o.min_aln_start = ptr(mn); o.max_aln_stop = ptr(mx);
  if (want_optional){
    o.ext_off = ext_off.data(); o.ext_len = ext_len.data(); o.dist_len = dist_len.data(); o.dist_rep = dist_rep.data(); o.dist_reads = dist_reads.data();
    o.dist_strong = dist_strong.data(); o.dist_frac = dist_frac.data();
  }
  std::vector<int32_t> stop; std::string err;
  CHECK(hipstr_hg::check(&b, &rq, &o, true, stop, err) == 0);
  hipstr_hg::hapgen_host(&b, &rq, stop.data(), &o);
  // ---- against the restatement
  size_t g = 0; int64_t dist = 0; long built = 0, options = 0;
  for (size_t l = 0; l < nl; l++){
    g_locus = (int)l;
    const Want w = restate(loci[l]);
    CHECK(status[l] == w.status);
    for (int k = 0; k < 3; k++){
      CHECK(blk_start[3*l+(size_t)k] == w.bs[k] && blk_end[3*l+(size_t)k] == w.be[k] && blk_nopts[3*l+(size_t)k] == (int)w.opts[k].size());
      for (const std::string& s : w.opts[k]){
        CHECK(opt_off[g+1] - opt_off[g] == (int32_t)s.size() && memcmp(seq.data() + opt_off[g], s.data(), s.size()) == 0);
        g++; options++;
      }
    }
    CHECK(n_spanning[l] == w.tot_reads && n_ss[l] == w.tot_samples && n_distinct[l] == w.distinct);
    if (want_optional){
      int counted = 0, sum = 0;
      for (int r = read_off[l]; r < read_off[l+1]; r++){
        CHECK((ext_len[(size_t)r] < 0) == (ext_off[(size_t)r] < 0));
        if (ext_len[(size_t)r] >= 0){ counted++; CHECK(ext_off[(size_t)r] + ext_len[(size_t)r] <= base_off[(size_t)r+1] - base_off[(size_t)r]); }
      }
      CHECK(counted == w.tot_reads);
      for (int d = 0; d < w.distinct; d++){
        sum += dist_reads[(size_t)(dist + d)];
        const int rep = dist_rep[(size_t)(dist + d)];
        CHECK(rep >= read_off[l] && rep < read_off[l+1] && ext_len[(size_t)rep] == dist_len[(size_t)(dist + d)]);
        CHECK(d == 0 || dist_len[(size_t)(dist + d)] >= dist_len[(size_t)(dist + d - 1)]);
      }
      CHECK(sum == w.tot_reads);
    }
    dist += w.distinct;
    built += w.status == 0;
  }
  CHECK(opt_off[0] == 0 && (size_t)opt_off[g] <= seq.size() && g <= 3*nl + n);
  // ---- the batch
  hipstr_hapgen_batch_t* hb = hipstr_hg::assemble_batch(&b, &rq, &o);
  CHECK(hb->batch.n_loci == built);
  int64_t kept_reads = 0;
  for (int k = 0; k < hb->batch.n_loci; k++){
    const int l = hb->locus[k];
    CHECK(status[(size_t)l] == 0 && hb->batch.period[k] == period[(size_t)l] && hb->batch.stutter[6*k + 5] == stutter[6*(size_t)l + 5]);
    CHECK(hb->batch.hap_off[k+1] - hb->batch.hap_off[k] == blk_nopts[3*(size_t)l + 1] && hb->batch.blk_nopts[3*k + 1] == blk_nopts[3*(size_t)l + 1]);
    CHECK(hb->batch.read_off[k+1] - hb->batch.read_off[k] == read_off[(size_t)l+1] - read_off[(size_t)l]);
    for (int r = hb->batch.read_off[k], src = read_off[(size_t)l]; r < hb->batch.read_off[k+1]; r++, src++){
      const int len = hb->batch.base_off[r+1] - hb->batch.base_off[r];
      CHECK(len == base_off[(size_t)src+1] - base_off[(size_t)src] && memcmp(hb->batch.bases + hb->batch.base_off[r], bases.data() + base_off[(size_t)src], (size_t)len) == 0);
      CHECK(hb->batch.read_start[r] == read_start[(size_t)src] && hb->batch.cigar_off[r+1] - hb->batch.cigar_off[r] == cigar_off[(size_t)src+1] - cigar_off[(size_t)src]);
    }
    kept_reads += hb->batch.read_off[k+1] - hb->batch.read_off[k];
  }
  for (size_t l = 0; l < nl; l++) CHECK(hb->status[l] == status[l]);
  CHECK(hb->batch.n_loci == 0 || hb->batch.read_off[hb->batch.n_loci] == kept_reads);
  delete hb;
  totals[0] += (long)nl; totals[1] += (long)n; totals[2] += built; totals[3] += options;
}

}  // namespace

int main(){
  std::mt19937_64 rng(20261019);
  long totals[4] = {0, 0, 0, 0};
  const int shapes[8][2] = { {0, 0}, {1, 0}, {3, 5}, {10, 40}, {16, 150}, {20, 100}, {12, 60}, {18, 80} };
  for (int c = 0; c < 8; c++){
    g_case = c;
    run_case(rng, shapes[c][0], shapes[c][1], c % 2 == 0, c % 3 != 0, c != 5, totals);
  }
  printf("ok %ld %ld %ld %ld\n", totals[0], totals[1], totals[2], totals[3]);
  return 0;
}
