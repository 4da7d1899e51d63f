// record_reads_host_test — a stand-alone program over hipstr_amd/csrc/record_reads_host.cpp and the kernels' lane and wavefront bodies
// (record_reads_layout.h, compiled as plain C++), built by tests/test_record_reads_host.py with -fsanitize=address,undefined.  Every array
// a body reads is a vector of exactly the length it may read, so a read beside it stops the program.
//   record_reads_host_test self           seeded CIGARs and samples: the lane body against the host twin's walk, the wavefront's steps
//                                         against the host twin's sort; the refusals of both checks; prints "ok"
//   record_reads_host_test cases IN OUT   the golden driver's lines ("C start region_start region_end n (op len)*", "H n (value)*") ->
//                                         "got bp_diff" and the condensed string per line, from the host twin; the bodies must agree
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../hipstr_amd/csrc/record_reads_host.h"
#include "../../hipstr_amd/csrc/record_reads_layout.h"

namespace rr = hipstr_record_reads;

static int g_bad = 0, g_checked = 0;
static uint64_t g_x = 88172645463325252ull;
static uint64_t next(uint64_t m){ g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return m ? g_x % m : 0; }

// the lane body and the host twin on one read; returns got, *bp
static int both_cigar(const std::vector<uint8_t>& op, const std::vector<int32_t>& len, int start, int rs, int re, int32_t* bp){
  int32_t a = 12345, b = 54321;
  const int lane = hs_rr_cigar_lane(op.data(), len.data(), (int)op.size(), start, rs, re, &a);
  const bool host = rr::extract_cigar(op.data(), len.data(), (int)op.size(), start, rs, re, &b);
  g_checked++;
  if (lane != (host ? 1 : 0) || a != b){
    g_bad++;
    fprintf(stderr, "cigar at %d, region %d..%d, %zu runs: lane body %d %d, host twin %d %d\n", start, rs, re, op.size(), lane, a, (int)host, b);
  }
  *bp = b;
  return host ? 1 : 0;
}

// hs_rr_hist_kernel's phases for one sample, its 64 lanes one after another; LDS arrays as vectors of the length that is used
static int wave_histogram(const std::vector<int32_t>& v, int32_t skip, std::vector<int32_t>* value, std::vector<int32_t>* count){
  const int n = (int)v.size();
  std::vector<int32_t> raw;
  for (int base = 0; base < n; base += HS_RR_WAVE)
    for (int lane = 0; lane < HS_RR_WAVE; lane++){ const int i = base + lane; if (i < n && v[i] != skip) raw.push_back(v[i]); }
  const int m = (int)raw.size();
  std::vector<int32_t> sorted((size_t)m, 0), head_at;
  std::vector<char> hit((size_t)m, 0);
  for (int lane = 0; lane < HS_RR_WAVE; lane++)
    for (int i = lane; i < m; i += HS_RR_WAVE){
      const int r = hs_rr_rank(raw.data(), m, i);
      if (r < 0 || r >= m || hit[r]){ g_bad++; fprintf(stderr, "rank %d of element %d of %d is taken or outside\n", r, i, m); return -1; }
      hit[r] = 1; sorted[r] = raw[i];
    }
  for (int base = 0; base < m; base += HS_RR_WAVE)
    for (int lane = 0; lane < HS_RR_WAVE; lane++){ const int k = base + lane; if (k < m && hs_rr_is_head(sorted.data(), k)) head_at.push_back(k); }
  const int np = (int)head_at.size();
  value->assign((size_t)np, 0); count->assign((size_t)np, 0);
  for (int p = 0; p < np; p++){ (*value)[p] = sorted[head_at[p]]; (*count)[p] = (p + 1 < np ? head_at[p + 1] : m) - head_at[p]; }
  return np;
}

static std::string condensed(const std::vector<int32_t>& v, int32_t skip){
  std::vector<int32_t> hv(v.size()), hc(v.size()), wv, wc;
  const int np = rr::condense(v.data(), (int)v.size(), skip, hv.data(), hc.data());
  const int wp = wave_histogram(v, skip, &wv, &wc);
  g_checked++;
  bool same = np == wp;
  for (int p = 0; same && p < np; p++) same = hv[p] == wv[p] && hc[p] == wc[p];
  if (!same){ g_bad++; fprintf(stderr, "a sample of %zu reads: %d pairs from the wavefront's steps, %d from the host twin (or they differ)\n", v.size(), wp, np); }
  int kept = 0, total = 0;
  for (int32_t x : v) kept += x != skip;
  for (int p = 0; p < np; p++){ total += hc[p]; if (p && hv[p] <= hv[p - 1]){ g_bad++; fprintf(stderr, "values do not ascend\n"); } }
  if (total != kept){ g_bad++; fprintf(stderr, "counts sum to %d, %d reads count\n", total, kept); }
  if (np == 0) return ".";
  std::string s;
  for (int p = 0; p < np; p++) s += (p ? ";" : "") + std::to_string(hv[p]) + "|" + std::to_string(hc[p]);
  return s;
}

static void expect(const std::string& got, const char* part, const char* what){
  if (got.find(part) == std::string::npos){ g_bad++; fprintf(stderr, "%s: \"%s\" lacks \"%s\"\n", what, got.c_str(), part); }
}

static int self_test(){
  const char letters[] = "MIDNSHP=X";
  for (int t = 0; t < 40000; t++){
    const int n = 1 + (int)next(t%50 ? 7 : 40);
    std::vector<uint8_t> op((size_t)n); std::vector<int32_t> len((size_t)n);
    for (int i = 0; i < n; i++){ const uint64_t k = next(16); op[i] = (uint8_t)letters[k < 8 ? 0 : k - 7]; len[i] = 1 + (int32_t)next(op[i] == 'M' ? 40 : 9); }
    const int start = (int)next(60), rs = (int)next(140) - 10, re = rs + (int)next(50);
    int32_t bp;
    both_cigar(op, len, start, rs, re, &bp);
  }
  {                             // positions at the top of int32: the check allows start + all lengths == INT32_MAX
    std::vector<uint8_t> op = {'M', 'I', 'M'}; std::vector<int32_t> len = {1000, 7, 2147483647 - 1000 - 7 - 5000};
    int32_t bp;
    if (!both_cigar(op, len, 5000, 5500, 2147483646 - 8, &bp) || bp != 7){ g_bad++; fprintf(stderr, "the top of int32\n"); }
    both_cigar(op, len, 5000, 5500, 2147483647, &bp);
  }
  for (int t = 0; t < 3000; t++){
    const int n = t < 200 ? t : (int)next(t%40 ? 150 : 1300), spread = 1 + (int)next(t%7 ? 12 : 400);
    std::vector<int32_t> v((size_t)n);
    for (int i = 0; i < n; i++) v[i] = next(6) == 0 ? INT32_MIN : (int32_t)next(2*spread + 1) - spread;
    condensed(v, INT32_MIN);
    if (t%10 == 0) condensed(v, 0);
  }
  if (condensed({INT32_MAX, INT32_MIN + 1, 0, -1, INT32_MAX}, INT32_MIN) != "-2147483647|1;-1|1;0|1;2147483647|2"){ g_bad++; fprintf(stderr, "the ends of int32\n"); }

  // the checks' refusals
  {
    int32_t read_off[2] = {0, 2}, start[2] = {5, 6}, coff[3] = {0, 1, 3}, len[3] = {10, 4, 6}, rs[1] = {8}, re[1] = {9}, pad[1] = {2};
    uint8_t op[3] = {'M', 'S', 'M'};
    hipstr_cigar_request_t rq = {1, read_off, start, coff, op, len, rs, re, pad};
    int64_t nr, nc; std::vector<int32_t> ps, pe;
    expect(rr::check_cigars(&rq, &nr, &nc, &ps, &pe) + "ok", "ok", "a valid request");
    if (nr != 2 || nc != 3 || ps[0] != 6 || pe[0] != 11){ g_bad++; fprintf(stderr, "check_cigars' outputs\n"); }
    uint8_t got[2]; int32_t bp[2];
    rr::cigars(&rq, ps.data(), pe.data(), got, bp);
    if (got[0] != 1 || bp[0] != 0 || got[1] != 0 || bp[1] != 0){ g_bad++; fprintf(stderr, "cigars: %d %d %d %d\n", got[0], bp[0], got[1], bp[1]); }
    start[1] = -1; expect(rr::check_cigars(&rq, &nr, &nc, &ps, &pe), "negative read_start", "start"); start[1] = 6;
    coff[1] = 0; expect(rr::check_cigars(&rq, &nr, &nc, &ps, &pe), "without CIGAR runs", "empty read"); coff[1] = 1;
    len[1] = 0; expect(rr::check_cigars(&rq, &nr, &nc, &ps, &pe), "non-positive", "length"); len[1] = 4;
    op[2] = 'm'; expect(rr::check_cigars(&rq, &nr, &nc, &ps, &pe), "no SAM letter", "op"); op[2] = 'M';
    pad[0] = -1; expect(rr::check_cigars(&rq, &nr, &nc, &ps, &pe), "below its region_start", "pad"); pad[0] = 2;
    re[0] = INT32_MAX; expect(rr::check_cigars(&rq, &nr, &nc, &ps, &pe), "outside int32", "region"); re[0] = 9;
    len[2] = INT32_MAX - 9; expect(rr::check_cigars(&rq, &nr, &nc, &ps, &pe), "leave int32", "positions"); len[2] = 6;
    read_off[0] = 1; expect(rr::check_cigars(&rq, &nr, &nc, &ps, &pe), "begin at 0", "read_off"); read_off[0] = 0;
  }
  {
    int32_t na[2] = {1, 1}, nsamp[2] = {3, 2}, read_off[3] = {0, 4, 5}, label[5] = {0, 0, 2, 2, 1};
    hipstr_post_batch_t pb; memset(&pb, 0, sizeof pb);
    pb.n_loci = 2; pb.n_alleles = na; pb.n_samples = nsamp; pb.read_off = read_off; pb.sample_label = label;
    std::vector<int32_t> begin, count;
    expect(rr::sample_runs(&pb, &begin, &count) + "ok", "ok", "a valid layout");
    const int32_t wb[5] = {0, 0, 2, 0, 4}, wc[5] = {2, 0, 2, 0, 1};
    if (begin.size() != 5 || memcmp(count.data(), wc, sizeof wc) || begin[0] != wb[0] || begin[2] != wb[2] || begin[4] != wb[4]){ g_bad++; fprintf(stderr, "sample_runs\n"); }
    label[3] = 1; expect(rr::sample_runs(&pb, &begin, &count), "grouped by ascending", "order"); label[3] = 2;
    label[4] = 2; expect(rr::sample_runs(&pb, &begin, &count), "out of range", "label"); label[4] = 1;
    nsamp[1] = -1; expect(rr::sample_runs(&pb, &begin, &count), "negative sample count", "samples"); nsamp[1] = 2;
    read_off[1] = 6; expect(rr::sample_runs(&pb, &begin, &count), "ascend", "read_off"); read_off[1] = 4;
  }
  printf("%d comparisons, %d failures\n", g_checked, g_bad);
  if (g_bad) return 1;
  printf("ok\n");
  return 0;
}

static int cases(const char* in_path, const char* out_path){
  std::ifstream in(in_path);
  FILE* out = fopen(out_path, "w");
  if (!in || !out){ fprintf(stderr, "cannot open files\n"); return 2; }
  std::string kind;
  while (in >> kind){
    if (kind == "C"){
      int start, rs, re, n;
      in >> start >> rs >> re >> n;
      std::vector<uint8_t> op((size_t)n); std::vector<int32_t> len((size_t)n);
      for (int i = 0; i < n; i++){ char t; in >> t >> len[i]; op[i] = (uint8_t)t; }
      int32_t bp;
      const int got = both_cigar(op, len, start, rs, re, &bp);
      fprintf(out, "%d %d\n", got, bp);
    } else {
      int n;
      in >> n;
      std::vector<int32_t> v((size_t)n);
      for (int i = 0; i < n; i++) in >> v[i];
      fprintf(out, "%s\n", condensed(v, INT32_MIN).c_str());
    }
  }
  fclose(out);
  return g_bad ? 1 : 0;
}

int main(int argc, char** argv){
  if (argc == 2 && !strcmp(argv[1], "self")) return self_test();
  if (argc == 4 && !strcmp(argv[1], "cases")) return cases(argv[2], argv[3]);
  fprintf(stderr, "usage: record_reads_host_test self | cases IN OUT\n");
  return 2;
}
