// census_host_check.cpp — the per-item pieces of the census kernels (hipstr_amd/csrc/census_layout.h: string hash, classing, key counting, the
// test of seq_stutter_genotyper.cpp:869, the candidate order) run on the host, lane by lane as census.hip runs them, against a plain loop over
// std::map / std::set.  Stand-alone: build with a host compiler and run it directly, e.g.
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o census_host_check tools/census_host_check.cpp && ./census_host_check
// Exit status 0 and "ok" when every random locus agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../hipstr_amd/csrc/census_layout.h"

static bool by_len_then_bytes(const std::string& a, const std::string& b){ return a.size() != b.size() ? a.size() < b.size() : a < b; }

int main(){
  std::mt19937 rng(20261018);
  int n_cand_total = 0, n_dup_total = 0;
  for (int trial = 0; trial < 400; trial++){
    const int nq = (int)(rng() % 90), n_samp = 1 + (int)(rng() % 4), nr = (int)(rng() % 400);
    const int min_reads = trial % 7 == 0 ? 3 : 2;
    const double min_frac = trial % 5 == 0 ? 0.25 : 0.15;
    // requests: strings from a small alphabet so that contents repeat; some long, some empty, some differing in one byte only
    std::vector<std::string> strs(nq);
    std::vector<int32_t> off(1, 0);
    std::string seq;
    for (int q = 0; q < nq; q++){
      const int kind = (int)(rng() % 10);
      int len = kind == 0 ? 0 : kind == 1 ? 60 + (int)(rng() % 10) : 1 + (int)(rng() % 4);
      std::string s;
      for (int i = 0; i < len; i++) s += "AC"[rng() % 2];
      if (kind == 1 && q > 0 && strs[q-1].size() > 50){ s = strs[q-1]; if (rng() % 2) s[rng() % 2 ? 0 : s.size() - 1] ^= 2; }
      strs[q] = s; seq += s; off.push_back((int32_t)seq.size());
    }
    std::set<std::string> options;
    for (int o = 0; o < 3 && nq; o++) options.insert(strs[rng() % nq]);
    // reads: (sample, request, spans, stutter)
    std::vector<int> rs(nr), rq(nr), span(nq), stut(nq);
    for (int q = 0; q < nq; q++){ span[q] = rng() % 4 != 0; stut[q] = rng() % 3 != 0; }
    for (int r = 0; r < nr; r++){ rs[r] = (int)(rng() % n_samp); rq[r] = nq ? (int)(rng() % (nq + 1)) - 1 : -1; }

    // ---- the plain loop (:852-872)
    std::vector<int> counts(n_samp, 0);
    std::vector<std::map<std::string, int>> sc(n_samp);
    for (int r = 0; r < nr; r++){
      if (rq[r] < 0 || !span[rq[r]]) continue;
      if (stut[rq[r]]) sc[rs[r]][strs[rq[r]]]++;
      counts[rs[r]]++;
    }
    std::set<std::string> want_set;
    for (int s = 0; s < n_samp; s++)
      for (const auto& kv : sc[s])
        if (kv.second >= min_reads && 1.0*kv.second/counts[s] >= min_frac && !options.count(kv.first)) want_set.insert(kv.first);
    std::vector<std::string> want(want_set.begin(), want_set.end());
    std::sort(want.begin(), want.end(), by_len_then_bytes);

    // ---- the kernel's phases, lane by lane
    std::vector<int32_t> hash(nq), cls(nq), flags(nq, 0), keys;
    for (int q = 0; q < nq; q++) hash[q] = (int32_t)hs_census_hash(seq.data() + off[q], off[q+1] - off[q]);
    for (int q = 0; q < nq; q++) cls[q] = hs_census_class_of(q, hash.data(), off.data(), seq.data());
    for (int q = 0; q < nq; q++){          // the class is the lowest request with the same content
      int first = q;
      for (int p = 0; p < q; p++) if (strs[p] == strs[q]){ first = p; break; }
      if (cls[q] != first){ printf("trial %d: class of request %d is %d, want %d\n", trial, q, cls[q], first); return 1; }
      n_dup_total += first != q;
    }
    std::vector<int> n_span(n_samp, 0);
    for (int r = 0; r < nr; r++){
      if (rq[r] < 0 || !span[rq[r]]) continue;
      n_span[rs[r]]++;
      if (stut[rq[r]]) keys.push_back(rs[r]*nq + cls[rq[r]]);
    }
    std::shuffle(keys.begin(), keys.end(), rng);        // the order the atomics arrive in is not defined
    for (size_t i = 0; i < keys.size(); i++){
      const int s = keys[i] / nq, c = keys[i] - s*nq;
      if (hs_census_qualifies(hs_census_count_key(keys.data(), (int)keys.size(), keys[i]), n_span[s], min_reads, min_frac)) flags[c] |= HS_CENSUS_QUAL;
    }
    for (int q = 0; q < nq; q++)
      if ((flags[q] & HS_CENSUS_QUAL) && cls[q] == q && !options.count(strs[q])) flags[q] |= HS_CENSUS_CAND;
    std::vector<int> at(nq, -1); int n_cand = 0;
    for (int q = 0; q < nq; q++)
      if (flags[q] & HS_CENSUS_CAND){ at[q] = hs_census_rank_of(q, nq, flags.data(), off.data(), seq.data()); n_cand++; }
    if (n_cand != (int)want.size()){ printf("trial %d: %d candidates, want %zu\n", trial, n_cand, want.size()); return 1; }
    std::vector<int> got(n_cand, -1);
    for (int q = 0; q < nq; q++) if (at[q] >= 0){
      if (at[q] >= n_cand || got[at[q]] != -1){ printf("trial %d: rank %d of request %d is taken or out of range\n", trial, at[q], q); return 1; }
      got[at[q]] = q;
    }
    for (int k = 0; k < n_cand; k++) if (strs[got[k]] != want[k]){ printf("trial %d: candidate %d differs\n", trial, k); return 1; }
    n_cand_total += n_cand;
  }
  // the two quotients that are exactly the double 0.15, and their neighbours
  if (!hs_census_qualifies(3, 20, 2, 0.15) || !hs_census_qualifies(6, 40, 2, 0.15) || hs_census_qualifies(3, 21, 2, 0.15) || hs_census_qualifies(2, 14, 2, 0.15) ||
      !hs_census_qualifies(2, 13, 2, 0.15) || hs_census_qualifies(1, 1, 2, 0.15)){ printf("threshold cases differ\n"); return 1; }
  if (n_cand_total < 100 || n_dup_total < 1000){ printf("the random loci do not bite: %d candidates, %d repeated strings\n", n_cand_total, n_dup_total); return 1; }
  printf("ok: 400 loci, %d candidates, %d repeated strings\n", n_cand_total, n_dup_total);
  return 0;
}
