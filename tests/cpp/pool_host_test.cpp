// pool_host_test.cpp — stand-alone check of the read pooler's host twin (hipstr_amd/csrc/pool_host.cpp), meant to be built with
// -fsanitize=address,undefined (tests/test_pool_host.py does):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan -fno-sanitize-recover=all tests/cpp/pool_host_test.cpp hipstr_amd/csrc/pool_host.cpp -o pool_host_test
// Fuzzed loci (0-400 reads of 1-300 bases, duplicates so that pools of 1-60 and more occur, prefixes of one another, bytes >= 0x80 in the
// qualities) and the edge shapes (no loci, loci without reads, reads of length 0) go through pool_reads_host into arrays of EXACTLY the
// documented sizes, and are compared with a quadratic restatement: a read joins the first earlier read with the same bytes; the median is
// std::sort over signed chars, entry n / 2.  Then the pooled batch is assembled and its reads checked.  Prints "ok <loci> <reads> <pools>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../hipstr_amd/csrc/pool_host.h"

namespace {

struct Host {            // a batch with the smallest consistent haplotype tables and one '=' run per read
  std::vector<int32_t> blk_start, blk_end, blk_nopts, period, opt_off, hap_off, read_off, base_off, read_start, cigar_off, cigar_len;
  std::vector<double> stutter; std::string seq, bases, quals, cigar_op;
  hipstr_batch_t b;
  void finish(){
    const int nl = (int)period.size();
    memset(&b, 0, sizeof b);
    b.n_loci = nl;
    b.blk_start = blk_start.data(); b.blk_end = blk_end.data(); b.blk_nopts = blk_nopts.data(); b.period = period.data(); b.stutter = stutter.data();
    b.opt_off = opt_off.data(); b.seq = seq.data(); b.hap_off = hap_off.data(); b.read_off = read_off.data(); b.base_off = base_off.data();
    b.bases = bases.data(); b.quals = quals.data(); b.read_start = read_start.data(); b.cigar_off = cigar_off.data(); b.cigar_op = cigar_op.data();
    b.cigar_len = cigar_len.data();
  }
};

#define CHECK(c) do { if (!(c)){ fprintf(stderr, "pool_host_test: %s failed at line %d (case %d)\n", #c, __LINE__, g_case); exit(1); } } while (0)
int g_case = 0;

void run_case(std::mt19937_64& rng, int n_loci, int max_reads, int max_len, long totals[3]){
  Host h;
  h.opt_off.push_back(0); h.hap_off.push_back(0); h.read_off.push_back(0); h.base_off.push_back(0); h.cigar_off.push_back(0);
  auto rnd = [&](int lo, int hi){ return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
  for (int l = 0; l < n_loci; l++){
    for (int k = 0; k < 3; k++){ h.blk_start.push_back(100 + 10*k); h.blk_end.push_back(110 + 10*k); h.blk_nopts.push_back(1); h.seq += "ACGTACGTAC"; h.opt_off.push_back((int32_t)h.seq.size()); }
    h.period.push_back(4); for (int k = 0; k < 6; k++) h.stutter.push_back(0.01);
    h.hap_off.push_back(h.hap_off.back() + 1);
    const int n = rnd(0, max_reads), k = std::max(1, n/rnd(1, 40));
    std::vector<std::string> seqs((size_t)k);
    for (int j = 0; j < k; j++){
      if (j % 5 == 1){ seqs[j] = seqs[j-1].substr(0, seqs[j-1].size() ? seqs[j-1].size() - 1 : 0); continue; }       // a prefix of its neighbour
      const int len = (max_len == 0 || rnd(0, 30) == 0) ? 0 : rnd(1, max_len);
      for (int i = 0; i < len; i++) seqs[j] += "ACGTacgtN"[rnd(0, 8)];
    }
    for (int r = 0; r < n; r++){
      const std::string& s = seqs[(size_t)rnd(0, k - 1)];
      h.bases += s;
      for (size_t i = 0; i < s.size(); i++) h.quals += (char)(rnd(0, 9) == 0 ? rnd(0x80, 0xFF) : rnd(33, 126));
      h.base_off.push_back((int32_t)h.bases.size()); h.read_start.push_back(r);
      h.cigar_op += '='; h.cigar_len.push_back(std::max<int>(1, (int)s.size())); h.cigar_off.push_back((int32_t)h.cigar_op.size());
    }
    h.read_off.push_back(h.read_off.back() + n);
  }
  if (h.cigar_len.empty()) h.cigar_len.push_back(0);
  h.finish();
  const hipstr_batch_t* b = &h.b;
  const size_t nr = (size_t)h.read_off.back(), nb = h.bases.size();
  // arrays of exactly the documented sizes (the sanitizer sees one byte too many)
  std::vector<int32_t> pool_index(nr), n_pools((size_t)n_loci), pool_off((size_t)n_loci + 1), pool_rep(nr), pool_size(nr), qoff(nr + 1);
  std::vector<char> pq(nb);
  hipstr_pool_out_t o = { pool_index.data(), n_pools.data(), pool_off.data(), pool_rep.data(), pool_size.data(), qoff.data(), pq.data() };
  hipstr_pool::pool_reads_host(b, &o);
  // the restatement
  CHECK(pool_off[0] == 0 && qoff[0] == 0);
  size_t P = 0, Q = 0;
  for (int l = 0; l < n_loci; l++){
    std::vector<int> first;
    for (int r = h.read_off[l]; r < h.read_off[l+1]; r++){
      const std::string s = h.bases.substr((size_t)h.base_off[r], (size_t)(h.base_off[r+1] - h.base_off[r]));
      int p = -1;
      for (size_t j = 0; j < first.size() && p < 0; j++){
        const int f = first[j];
        if (h.bases.substr((size_t)h.base_off[f], (size_t)(h.base_off[f+1] - h.base_off[f])) == s) p = (int)j;
      }
      if (p < 0){ p = (int)first.size(); first.push_back(r); }
      CHECK(pool_index[(size_t)r] == p);
    }
    CHECK(n_pools[(size_t)l] == (int)first.size() && pool_off[(size_t)l] == (int)P && pool_off[(size_t)l + 1] == (int)(P + first.size()));
    for (size_t j = 0; j < first.size(); j++, P++){
      const int f = first[j], len = h.base_off[f+1] - h.base_off[f];
      std::vector<int> mem;
      for (int r = h.read_off[l]; r < h.read_off[l+1]; r++) if (pool_index[(size_t)r] == (int)j) mem.push_back(r);
      CHECK(pool_rep[P] == f && pool_size[P] == (int)mem.size() && qoff[P] == (int)Q);
      for (int i = 0; i < len; i++){
        std::vector<signed char> v;
        for (int r : mem) v.push_back((signed char)h.quals[(size_t)h.base_off[r] + (size_t)i]);
        std::sort(v.begin(), v.end());
        CHECK((signed char)pq[Q + (size_t)i] == v[v.size()/2]);
      }
      Q += (size_t)len;
      CHECK(qoff[P + 1] == (int)Q);
    }
  }
  // the pooled batch
  hipstr_pooled_batch* pb = hipstr_pool::assemble_pooled_batch(b, &o);
  const hipstr_batch_t* q = &pb->batch;
  CHECK(q->n_loci == n_loci && q->realign_read == NULL && q->realign_hap == NULL);
  for (int l = 0; l <= n_loci; l++) CHECK(q->read_off[l] == pool_off[(size_t)l] && q->hap_off[l] == h.hap_off[(size_t)l]);
  for (size_t p = 0; p < P; p++){
    const int f = pool_rep[p], len = h.base_off[f+1] - h.base_off[f];
    CHECK(q->base_off[p+1] - q->base_off[p] == len && q->read_start[p] == h.read_start[(size_t)f]);
    CHECK(len == 0 || memcmp(q->bases + q->base_off[p], h.bases.data() + h.base_off[f], (size_t)len) == 0);
    CHECK(len == 0 || memcmp(q->quals + q->base_off[p], pq.data() + qoff[p], (size_t)len) == 0);
    CHECK(q->cigar_off[p+1] - q->cigar_off[p] == 1 && q->cigar_op[q->cigar_off[p]] == '=' && q->cigar_len[q->cigar_off[p]] == h.cigar_len[(size_t)f]);
  }
  for (size_t r = 0; r < nr; r++) CHECK(pb->pool_index[r] == pool_index[r]);
  delete pb;
  totals[0] += n_loci; totals[1] += (long)nr; totals[2] += (long)P;
}

}  // namespace

int main(){
  std::mt19937_64 rng(20261018);
  long totals[3] = { 0, 0, 0 };
  run_case(rng, 0, 0, 0, totals); g_case++;          // no loci
  run_case(rng, 5, 0, 10, totals); g_case++;         // loci without reads
  run_case(rng, 4, 30, 0, totals); g_case++;         // reads of length 0 only
  run_case(rng, 3, 12, 1, totals); g_case++;         // one-base reads
  for (int c = 0; c < 6; c++){ run_case(rng, 8, 400, 300, totals); g_case++; }
  printf("ok %ld %ld %ld\n", totals[0], totals[1], totals[2]);
  return 0;
}
