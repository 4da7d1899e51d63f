// record_host_test — a stand-alone program over hipstr_amd/csrc/record_host.cpp and the device's lane body (record_layout.h, compiled as
// plain C++), built by tests/test_record_host.py with -fsanitize=address,undefined.
//   record_host_test self                 sweeps the golden's index rules (count pairs 0..24 x 0..24, 2x2 tables with cells 0..12) and
//                                         seeded large quadruples: the lane body against the host twin (1e-9 absolute, infinities and the
//                                         empty total's 1 and the equal counts' 0.0 equal), the record's loops on a small batch, the refusals; prints "ok"
//   record_host_test pvalues IN OUT       quadruples "u1 u2 rv1 rv2" per line -> the host twin's "ab fs" as hexadecimal bit patterns
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../hipstr_amd/csrc/record_host.h"
#include "../../hipstr_amd/csrc/record_layout.h"

namespace hr = hipstr_record;

static uint64_t bits(double x){ uint64_t u; memcpy(&u, &x, 8); return u; }
static int g_bad = 0, g_checked = 0, g_differ = 0;

static void same(const char* what, double dev, double host, int a, int b, int c, int d){
  g_checked++;
  const bool inf_h = isinf(host), inf_d = isinf(dev);
  bool ok;
  if (inf_h || inf_d || host == 1.0) ok = bits(dev) == bits(host);          // (1: the empty total)
  else ok = fabs(dev - host) <= 1e-9;
  if (bits(dev) != bits(host)) g_differ++;
  if (!ok){ g_bad++; fprintf(stderr, "%s(%d %d %d %d): lane body %a, host twin %a\n", what, a, b, c, d, dev, host); }
}

static void check(const double* t, int u1, int u2, int r1, int r2){
  if (u1 + u2 <= HS_REC_TABLE_READS){
    same("ab", hs_rec_allele_bias(t, u1, u2), hr::allele_bias(u1, u2), u1, u2, r1, r2);
    same("fs", hs_rec_strand_bias(t, u1, r1, u2, r2), hr::strand_bias(u1, r1, u2, r2), u1, u2, r1, r2);
  } else {                      // beyond the table: the host twin alone (it must not fault)
    hr::allele_bias(u1, u2); hr::strand_bias(u1, r1, u2, r2);
  }
}

static int self_test(){
  std::vector<double> table(3*(size_t)HS_REC_TABLE_N);
  hr::fill_table(table.data(), HS_REC_TABLE_N);
  const double* t = table.data();
  for (int i = 0; i < 625; i++) check(t, i/25, i%25, 0, 0);
  for (int a = 1; a <= 2500; a += 7) if (hs_rec_allele_bias(t, a, a) != 0.0 || hr::allele_bias(a, a) != 0.0){ g_bad++; fprintf(stderr, "equal counts %d\n", a); }
  for (int i = 0; i < 28561; i++){
    const int n11 = i/2197, n12 = i/169%13, n21 = i/13%13, n22 = i%13;
    check(t, n11 + n12, n21 + n22, n12, n22);
  }
  uint64_t x = 88172645463325252ull;
  auto next = [&](uint64_t m){ x ^= x << 13; x ^= x >> 7; x ^= x << 17; return m ? x % m : 0; };
  for (int n = 160; n <= 180; n++) for (int k = 0; 2*k < n; k++) check(t, k, n - k, (int)next(k + 1), (int)next(n - k + 1));
  for (int n = 1; n <= 5003; n += (n < 60 ? 1 : 37)) for (int k = 0; k <= 3 && 2*k < n; k++) check(t, n - k, k, (int)next(n - k + 1), (int)next(k + 1));
  for (int k = 1; k <= 2499; k += (k < 100 ? 1 : 113)) check(t, k, k + 1, k/2, (k + 1)/2);
  for (int i = 0; i < 400; i++){
    const int n = 200 + (int)next(4801), w = 3*(int)sqrt((double)n);
    int a = n/2 + (int)next(2*w + 1) - w;
    a = a < 0 ? 0 : a > n ? n : a;
    check(t, a, n - a, i%3 ? (int)next(a + 1) : a/2, i%3 ? (int)next(n - a + 1) : (n - a)/2);
  }
  check(t, 2500, 2500, 1250, 1250); check(t, 2500, 2500, 0, 2500); check(t, 4000, 6000, 100, 5000); check(t, 5000, 5001, 0, 0);
  if (hr::bdtr(4, 9, 0.5) != 0x1.0000000000001p-1){ g_bad++; fprintf(stderr, "bdtr(4, 9, .5) = %a\n", hr::bdtr(4, 9, 0.5)); }
  if (hr::allele_bias(4, 5) != 0.0 || hs_rec_allele_bias(t, 4, 5) != 0.0){ g_bad++; fprintf(stderr, "the clamp at n = 2k + 1\n"); }

  // the record's loops: 2 loci (diploid, haploid) x 4 samples
  const int32_t n_alleles[2] = {3, 2}, n_samples[2] = {4, 4}, n_variants[2] = {2, 2}, h2a[5] = {0, 1, 1, 0, 1};
  const uint8_t haploid[2] = {0, 1}, reported[8] = {1, 1, 1, 0, 1, 1, 1, 1}, masked[8] = {0, 0, 1, 0, 0, 0, 0, 1};
  int32_t map_gt[16] = {0, 1, 1, 2, 0, 0, 1, 1, 0, 0, 1, 1, -1, -1, 0, 0};
  const int32_t na[8] = {20, 40, 20, 20, 10, 20, 0, 20}, ns[8] = {1, 2, 3, 4, 5, 6, 0, 8}, nst[8] = {2, 2, 2, 2, 2, 2, 0, 2}, nfi[8] = {3, 7, 2, 0, 0, 3, 0, 9};
  int32_t u1[8] = {7, 9, 1, 1, 1, 1, 0, 1}, u2[8] = {3, 9, 1, 1, 1, 1, 0, 1}, r1[8] = {2, 4, 0, 0, 0, 0, 0, 0}, r2[8] = {3, 1, 0, 0, 0, 0, 0, 0};
  hipstr_record_request_t rq; memset(&rq, 0, sizeof rq);
  rq.n_variants = n_variants; rq.hap_to_allele = h2a; rq.sample_reported = reported; rq.sample_masked = masked;
  rq.n_aligned = na; rq.n_snp = ns; rq.n_stutter = nst; rq.n_flank_indel = nfi; rq.uniq_one = u1; rq.uniq_two = u2; rq.rv_uniq_one = r1; rq.rv_uniq_two = r2;
  int32_t status[8], gt[16], dab[8], loc[7][2], ac[4];
  double ab[8], fs[8];
  hipstr_record_out_t out = { status, gt, ab, dab, fs, loc[0], loc[1], loc[2], loc[3], loc[4], loc[5], loc[6], ac };
  std::string why = hr::fields(2, n_alleles, n_samples, haploid, map_gt, &rq, &out);
  const int32_t want_status[8] = {0, 3, 2, -1, 0, 0, 1, 2};
  if (!why.empty() || memcmp(status, want_status, sizeof status)){ g_bad++; fprintf(stderr, "fields: %s / status\n", why.c_str()); }
  // locus 0: sample 0 passes (3 > 0.15f*20 is false), sample 1 is filtered (7 > 6), sample 2 masked, sample 3 has no column
  if (loc[0][0] != 1 || loc[1][0] != 1 || loc[2][0] != 2 || ac[0] != 1 || ac[1] != 1 || loc[3][0] != 20 || loc[6][0] != 3){ g_bad++; fprintf(stderr, "fields: locus 0\n"); }
  // locus 1 (haploid): samples 4, 5 pass; 6 has no reads and stays in DP's loop; 7 is masked AND over the fraction: NFILT, not NSKIP
  if (loc[0][1] != 0 || loc[1][1] != 1 || loc[2][1] != 2 || ac[2] != 1 || ac[3] != 1 || loc[3][1] != 30 || loc[4][1] != 11){ g_bad++; fprintf(stderr, "fields: locus 1\n"); }
  if (ab[0] != hr::allele_bias(7, 3) || fs[0] != hr::strand_bias(7, 2, 3, 3) || dab[0] != 10 || ab[1] != 1.01 || ab[4] != 1.01){ g_bad++; fprintf(stderr, "fields: p-values\n"); }
  map_gt[9] = 1;                // a haploid heterozygote among the counted samples
  if (hr::fields(2, n_alleles, n_samples, haploid, map_gt, &rq, &out).find("haploid") == std::string::npos){ g_bad++; fprintf(stderr, "haploid het not refused\n"); }
  map_gt[9] = 0; r1[0] = 8;
  if (hr::fields(2, n_alleles, n_samples, haploid, map_gt, &rq, &out).find("exceeds") == std::string::npos){ g_bad++; fprintf(stderr, "rv > uniq not refused\n"); }
  r1[0] = 2; u2[3] = -1;
  if (hr::fields(2, n_alleles, n_samples, haploid, map_gt, &rq, &out).find("negative") == std::string::npos){ g_bad++; fprintf(stderr, "negative count not refused\n"); }

  printf("%d comparisons, %d not bit-identical, %d outside the bound\n", g_checked, g_differ, g_bad);
  if (g_bad) return 1;
  printf("ok\n");
  return 0;
}

int main(int argc, char** argv){
  if (argc == 2 && !strcmp(argv[1], "self")) return self_test();
  if (argc == 4 && !strcmp(argv[1], "pvalues")){
    FILE* in = fopen(argv[2], "r"); FILE* out = fopen(argv[3], "w");
    if (!in || !out){ fprintf(stderr, "cannot open files\n"); return 2; }
    int a, b, r1, r2;
    while (fscanf(in, "%d %d %d %d", &a, &b, &r1, &r2) == 4)
      fprintf(out, "%llx %llx\n", (unsigned long long)bits(hr::allele_bias(a, b)), (unsigned long long)bits(hr::strand_bias(a, r1, b, r2)));
    fclose(in); fclose(out);
    return 0;
  }
  fprintf(stderr, "usage: record_host_test self | pvalues IN OUT\n");
  return 2;
}
