// record_alleles_host_test — a stand-alone program over hipstr_amd/csrc/record_alleles_host.cpp and the per-option steps of hs_ra_kernel
// (record_alleles_layout.h, compiled as plain C++), built by tests/test_record_alleles_host.py with -fsanitize=address,undefined.  The
// wavefront is replayed with its 64 lanes one after another over the same steps; its pool and window are vectors of exactly the bytes
// that may be touched.
//   record_alleles_host_test self           seeded loci: the replayed wavefront against the host twin; prints "ok"
//   record_alleles_host_test cases IN OUT   the golden driver's cases (integration/genotype_flow.cpp --record-cases) -> its output format
//                                           from the host twin ("status N" instead of a record for a refused locus); the replay must agree
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hipstr_amd/csrc/record_alleles_host.h"
#include "../../hipstr_amd/csrc/record_alleles_layout.h"

namespace ra = hipstr_rec_alleles;
static int g_bad = 0, g_checked = 0;
static uint64_t g_x = 88172645463325252ull;
static uint64_t next(uint64_t m){ g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return m ? g_x % m : 0; }

// hs_ra_kernel for one locus
static void wave_locus(const std::vector<std::string>& options, int32_t start0, int32_t end0, int32_t rs32, int32_t re32, const std::string& window, ra::Locus* out){
  const int V = (int)options.size();
  std::string seq; std::vector<int32_t> off(1, 0);
  for (const std::string& o : options){ seq += o; off.push_back((int32_t)seq.size()); }
  const int o0 = off[0], n0 = off[1] - off[0];
  const int64_t gap_l = (int64_t)rs32 - start0, gap_r = (int64_t)end0 - re32;
  const int max_lt = (int)(gap_l < 0 ? 0 : gap_l > n0 ? n0 : gap_l), max_rt = (int)(gap_r < 0 ? 0 : gap_r > n0 ? n0 : gap_r);
  int lt = 0, rt = 0;
  bool go = true;
  for (int t = 0; t < max_lt && go; t++){
    bool any = false;
    for (int i = 0; i < V; i++) any = any || hs_ra_left_stop(seq.data(), off[i], off[i + 1] - off[i], o0, n0, t);
    go = !any;
    if (go) lt = t + 1;
  }
  go = true;
  for (int t = 0; t < max_rt && go; t++){
    bool any = false;
    for (int i = 0; i < V; i++) any = any || hs_ra_right_stop(seq.data(), off[i], off[i + 1] - off[i], o0, n0, lt, t);
    go = !any;
    if (go) rt = t + 1;
  }
  const int64_t start = (int64_t)start0 + lt, end = (int64_t)end0 - rt, rs = rs32, re = re32, w0 = rs - HS_RA_WIN_PAD, w1 = w0 + (int64_t)window.size();
  const int64_t lf = start >= rs ? start - rs : 0, rf = end <= re ? re - end : 0;
  int status = 0;
  if (lf > 0 && (rs < 0 || rs + lf > w1)) status = HS_RA_OUTSIDE;
  if (rf > 0 && (end < 0 || end < w0 || end + rf > w1)) status = HS_RA_OUTSIDE;
  int64_t pos = rs < start ? rs : start;
  int pad = 0;
  if (lf == 0){
    const char first = n0 - lt - rt > 0 ? seq[(size_t)(o0 + lt)] : (char)0;
    bool want = false;
    for (int i = 1; i < V; i++) want = want || off[i + 1] - off[i] - lt - rt <= 0 || seq[(size_t)(off[i] + lt)] != first;
    if (want){ pad = 1; pos -= 1; if (pos < 0 || pos < w0 || pos >= w1) status = HS_RA_OUTSIDE; }
  }
  pos += 1;
  *out = ra::Locus();
  if (status){ out->status = status; return; }
  std::vector<std::string> pool((size_t)V);
  for (int i = 0; i < V; i++){
    const int mid = off[i + 1] - off[i] - lt - rt;
    std::string& s = pool[(size_t)i];
    if (pad) s.push_back(hs_ra_upper(window.at((size_t)(pos - 1 - w0))));
    for (int64_t k = 0; k < lf; k++) s.push_back(hs_ra_upper(window.at((size_t)(rs - w0 + k))));
    for (int k = 0; k < mid; k++) s.push_back(seq.at((size_t)(off[i] + lt + k)));
    for (int64_t k = 0; k < rf; k++) s.push_back(hs_ra_upper(window.at((size_t)(end - w0 + k))));
  }
  bool dup = false;
  std::vector<int32_t> o2n((size_t)V), n2o((size_t)V, -1), bp((size_t)V);
  for (int i = 0; i < V; i++){
    int r = i == 0 ? 0 : 1;
    for (int j = 0; j < V; j++){
      if (j == i) continue;
      const int c = hs_ra_order(pool[(size_t)j].data(), (int)pool[(size_t)j].size(), pool[(size_t)i].data(), (int)pool[(size_t)i].size());
      if (c == 0) dup = true;
      if (c < 0 && i >= 1 && j >= 1) r++;
    }
    o2n[(size_t)i] = r; bp[(size_t)i] = (int32_t)pool[(size_t)i].size() - (int32_t)pool[0].size();
  }
  if (dup){ out->status = HS_RA_DUPLICATE; return; }
  for (int i = 0; i < V; i++) n2o.at((size_t)o2n[(size_t)i]) = i;
  out->pos = (int32_t)pos; out->left_trim = (int32_t)(lt - lf - pad); out->right_trim = (int32_t)(rt - rf);
  out->alleles = pool; out->bp_diff = bp; out->old_to_new = o2n; out->new_to_old = n2o;
}

static bool same(const ra::Locus& a, const ra::Locus& b){
  return a.status == b.status && a.pos == b.pos && a.left_trim == b.left_trim && a.right_trim == b.right_trim && a.alleles == b.alleles &&
         a.bp_diff == b.bp_diff && a.old_to_new == b.old_to_new && a.new_to_old == b.new_to_old;
}

static ra::Locus both(const char* what, const std::vector<std::string>& options, int start, int end, int rs, int re, const std::string& window){
  ra::Locus h, w;
  ra::alleles_of(options, start, end, rs, re, window.data(), (int32_t)window.size(), &h);
  wave_locus(options, start, end, rs, re, window, &w);
  g_checked++;
  if (!same(h, w)){ g_bad++; fprintf(stderr, "%s: host twin (status %d pos %d trims %d %d) and the replayed wavefront (status %d pos %d trims %d %d) differ\n", what,
                                     h.status, h.pos, h.left_trim, h.right_trim, w.status, w.pos, w.left_trim, w.right_trim); }
  return h;
}

static int self_test(){
  const char letters[] = "ACGTacgt";
  std::string chrom;
  for (int i = 0; i < 600; i++) chrom.push_back(letters[next(8)]);
  int statuses[3] = {0, 0, 0};
  for (int t = 0; t < 6000; t++){
    const int rs = 60 + (int)next(300), re = rs + 1 + (int)next(60);
    const int start = rs + (int)next(70) - 50, end = re + (int)next(70) - 20;
    const int V = 1 + (int)next(t%20 ? 6 : 90), alphabet = t%3 ? 4 : 2;
    std::string pre, suf;
    for (int i = (int)next(14); i > 0; i--) pre.push_back(letters[next((uint64_t)alphabet)]);
    for (int i = (int)next(14); i > 0; i--) suf.push_back(letters[next((uint64_t)alphabet)]);
    std::vector<std::string> options;
    for (int i = 0; i < V; i++){
      std::string m;
      for (int k = (int)next(t%5 ? 7 : 3); k > 0; k--) m.push_back(next(40) ? letters[next((uint64_t)alphabet)] : (char)(0x80 + next(100)));
      options.push_back(next(30) ? pre + m + suf : m);
    }
    const int w0 = rs - HS_RA_WIN_PAD, w1 = re + HS_RA_WIN_PAD - (int)(t%11 ? 0 : next(50));
    const std::string window = chrom.substr((size_t)w0, (size_t)(w1 - w0));
    const ra::Locus h = both("fuzz", options, start, end, rs, re, window);
    statuses[h.status]++;
    std::vector<int32_t> o2n, n2o;
    if (h.status == 0 && !ra::reorder(h.alleles, &o2n, &n2o)){ g_bad++; fprintf(stderr, "reorder refuses what alleles_of took\n"); }
  }
  if (!statuses[0] || !statuses[1] || !statuses[2]){ g_bad++; fprintf(stderr, "the fuzz reached statuses %d %d %d\n", statuses[0], statuses[1], statuses[2]); }
  // the flank strings
  std::vector<std::string> lf, rf;
  if (!ra::flank_options({"ACGT", "ACG"}, {"TTT"}, "CACACA", 2, 1, &lf, &rf) || lf[0] != "ACGTCA" || lf[1] != "ACGCA" || rf[0] != "ATTT"){ g_bad++; fprintf(stderr, "flank_options, extended\n"); }
  if (!ra::flank_options({"ACGT", "ACG"}, {"TTT"}, "CACACA", -2, 0, &lf, &rf) || lf[0] != "AC" || lf[1] != "A" || rf[0] != "TTT"){ g_bad++; fprintf(stderr, "flank_options, cut\n"); }
  if (ra::flank_options({"ACGT", "AC"}, {"TTT"}, "CACACA", -2, 0, &lf, &rf) || !lf.empty()){ g_bad++; fprintf(stderr, "flank_options, :1023\n"); }
  if (ra::flank_options({"ACGT"}, {"TTT"}, "CACACA", 3, 3, &lf, &rf) || ra::flank_options({"ACGT"}, {"TTT"}, "CACACA", 0, -1, &lf, &rf)){ g_bad++; fprintf(stderr, "flank_options, :1016 / :1037\n"); }
  printf("%d comparisons (statuses %d %d %d), %d failures\n", g_checked, statuses[0], statuses[1], statuses[2], g_bad);
  if (g_bad) return 1;
  printf("ok\n");
  return 0;
}

static int cases(const char* in_path, const char* out_path){
  std::ifstream in(in_path);
  FILE* out = fopen(out_path, "w");
  if (!in || !out){ fprintf(stderr, "cannot open files\n"); return 2; }
  auto seq = [](const std::string& s){ return s == "-" ? std::string() : s; };
  auto show = [](const std::string& s){ return s.empty() ? "-" : s.c_str(); };
  std::string line;
  while (std::getline(in, line)){
    if (line.empty()) continue;
    std::istringstream hd(line);
    std::string word, name, chrom; int rs = 0, re = 0;
    hd >> word >> name >> rs >> re;
    std::getline(in, line);
    { std::istringstream ls(line); ls >> word >> chrom; }
    std::vector<std::string> options; int start1 = 0, end1 = 0;
    for (int b = 0; b < 3; b++){
      std::getline(in, line);
      std::istringstream ls(line);
      int idx = 0, start = 0, end = 0, n = 0; std::string s;
      ls >> word >> idx >> start >> end >> n;
      for (int o = 0; o < n; o++){ ls >> s; if (b == 1) options.push_back(seq(s)); }
      if (b == 1){ start1 = start; end1 = end; }
    }
    const int w0 = rs - HS_RA_WIN_PAD, w1 = re + HS_RA_WIN_PAD < (int)chrom.size() ? re + HS_RA_WIN_PAD : (int)chrom.size();
    const std::string window = std::string((size_t)(w0 < 0 ? -w0 : 0), '.') + chrom.substr((size_t)(w0 < 0 ? 0 : w0), (size_t)(w1 - (w0 < 0 ? 0 : w0)));
    const ra::Locus h = both(name.c_str(), options, start1, end1, rs, re, window);
    fprintf(out, "case %s\n", name.c_str());
    if (h.status){ fprintf(out, "status %d\n", h.status); continue; }
    fprintf(out, "pos %d\ntrim %d %d\nalleles %zu", h.pos, h.left_trim, h.right_trim, h.alleles.size());
    for (const std::string& s : h.alleles) fprintf(out, " %s", show(s));
    fprintf(out, "\nold_to_new");
    for (int32_t v : h.old_to_new) fprintf(out, " %d", v);
    fprintf(out, "\nnew_to_old");
    for (int32_t v : h.new_to_old) fprintf(out, " %d", v);
    fprintf(out, "\n");
  }
  fclose(out);
  return g_bad ? 1 : 0;
}

int main(int argc, char** argv){
  if (argc == 2 && !strcmp(argv[1], "self")) return self_test();
  if (argc == 4 && !strcmp(argv[1], "cases")) return cases(argv[2], argv[3]);
  fprintf(stderr, "usage: record_alleles_host_test self | cases IN OUT\n");
  return 2;
}
