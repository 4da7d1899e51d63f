// record_layout.h — what record.hip's kernels and the host share: the argument blocks, and the body of one lane — the AB and FS p-values
// of a count quadruple as the device computes them.  The body is plain C++ over cr_math.h (tests/cpp/record_host_test.cpp runs it on the
// host against record_host.cpp).
//
// How the device form differs from the host twin (record_host.cpp), and why it needs no pow, gamma or lgamma of its own:
//   * x is always 0.5: pow(0.5, integer) is an exact power of two (down through the subnormals, then 0), log(0.5) one constant, and
//     incbet's swap of the tails never happens (a = n - k >= b = k + 1 because k is the smaller count);
//   * gamma, lgam and libm's lgamma are needed at integers only: a table of three doubles per integer, filled once by the host twin's own
//     functions (hipstr_record::fill_table), up to HS_REC_TABLE_N;
//   * exp, log and log10 are the correctly rounded ones of cr_math.h, so a result differs from the host's only where the host's libm is
//     not correctly rounded.
// Every loop has its bound in its head: 300 terms of a continued fraction, b terms of the power series, max - min + 1 (at most
// HS_REC_TABLE_N) steps of a Fisher tail.
#pragma once
#include <stdint.h>
#include "cr_math.h"

#define HS_REC_THREADS 64                        // one wavefront per workgroup: up to 64 samples of ONE locus, as they come
#define HS_REC_TABLE_READS 5000                  // == HIPSTR_RECORD_TABLE_READS
#define HS_REC_TABLE_N (HS_REC_TABLE_READS + 3)  // integers 0 .. reads + 2
#define HS_REC_NOT_APPLICABLE 1.01

#define HS_REC_ERR_NO_PAIR 1                     // a sample that passes every filter without a MAP pair
#define HS_REC_ERR_HAPLOID_HET 2                 // a haploid locus with a heterozygous genotype that would be counted
#define HS_REC_ERR_MAP_RANGE 4                   // map_gt outside [-1, A)

struct hs_rec_pv_dev_t {                         // hipstr_bias_pvalues
  const double* table;                           // [3*HS_REC_TABLE_N]
  const int32_t *u1, *u2, *rv1, *rv2;
  double *ab, *fs;
  int64_t n;
};

struct hs_rec_locus_t { int32_t samp_off, n_samples, hap_off, n_alleles, var_off, n_variants, haploid, first_group; };
struct hs_rec_dev_t {                            // hipstr_record_fields
  const double* table;
  const hs_rec_locus_t* loci;                    // [n_loci]
  const int32_t* group_locus;                    // [n_groups] locus of every workgroup
  const int32_t* map_gt;                         // [2*n_samp] the posterior run's
  const int32_t* hap_to_allele;
  const uint8_t *reported, *masked;              // NULL = all / none
  const int32_t* counts[8];                      // [n_samp] each: n_aligned, n_snp, n_stutter, n_flank_indel, uniq_one, uniq_two, rv_uniq_one, rv_uniq_two
  int32_t *status, *gt, *dab;                    // [n_samp], [2*n_samp], [n_samp]
  double *ab, *fs;
  int32_t* locus_out;                            // [7*n_loci]: n_skip, n_filt, an, dp, dsnp, dstutter, dflankindel (zeroed before the launch)
  int32_t* allele_count;                         // [sum V] (zeroed)
  int32_t* error;                                // [1] HS_REC_ERR_* (zeroed)
  int32_t n_loci, n_groups; int64_t n_samp;
  float frac;
};

#define HS_REC_MACHEP 1.11022302462515654042E-16
#define HS_REC_MAXLOG 7.09782712893383996732E2
#define HS_REC_MINLOG (-7.451332191019412076235E2)
#define HS_REC_MAXGAM 171.624376956302725
#define HS_REC_LOG_HALF (-0x1.62e42fefa39efp-1)   // RN(log 0.5): what a correctly rounded libm returns

// 0.5^e for an integer e >= 0, exact: normal to 2^-1022, subnormal to 2^-1074, then 0 (2^-1075 is a tie that rounds to even)
CR_FN double hs_rec_pow_half(int e){
  if (e <= 1022) return cr_from_bits((uint64_t)(1023 - e) << 52);
  if (e <= 1074) return cr_from_bits(1ull << (1074 - e));
  return 0.0;
}
CR_FN double hs_rec_inf(){ return cr_from_bits(0x7ff0000000000000ull); }
// the table's columns at an integer; outside the table +inf (what lgamma gives at the non-positive integers a Fisher walk may touch
// below its support; the table's own row 0 holds the same)
CR_FN double hs_rec_tab(const double* t, int i, int col){ return (i < 0 || i >= HS_REC_TABLE_N) ? hs_rec_inf() : t[3*i + col]; }
#define HS_REC_GAMMA(i)  hs_rec_tab(t, (int)(i), 0)
#define HS_REC_LGAM(i)   hs_rec_tab(t, (int)(i), 1)
#define HS_REC_LGAMMA(i) hs_rec_tab(t, (int)(i), 2)

// incbcf / incbd at x = 0.5 (second: z = x/(1-x) = 1)
CR_FN double hs_rec_cfrac(double a, double b, bool second){
  double k1 = a, k2 = second ? b - 1.0 : a + b, k3 = a, k4 = a + 1.0, k5 = 1.0, k6 = second ? a + b : b - 1.0, k7 = a + 1.0, k8 = a + 2.0;
  const double z = second ? 0.5/(1.0 - 0.5) : 0.5, d2 = second ? -1.0 : 1.0, d6 = -d2;
  const double big = 4.503599627370496e15, biginv = 2.22044604925031308085e-16, thresh = 3.0*HS_REC_MACHEP;
  double pkm2 = 0.0, qkm2 = 1.0, pkm1 = 1.0, qkm1 = 1.0, ans = 1.0, r = 1.0;
  for (int n = 0; n < 300; n++){
    double xk = -(z*k1*k2)/(k3*k4);
    double pk = pkm1 + pkm2*xk, qk = qkm1 + qkm2*xk;
    pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;
    xk = (z*k5*k6)/(k7*k8);
    pk = pkm1 + pkm2*xk; qk = qkm1 + qkm2*xk;
    pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;
    if (qk != 0) r = pk/qk;
    double tt = 1.0;
    if (r != 0){ tt = fabs((ans - r)/r); ans = r; }
    if (tt < thresh) break;
    k1 += 1.0; k2 += d2; k3 += 2.0; k4 += 2.0; k5 += 1.0; k6 += d6; k7 += 2.0; k8 += 2.0;
    if (fabs(qk) + fabs(pk) > big){ pkm2 *= biginv; pkm1 *= biginv; qkm2 *= biginv; qkm1 *= biginv; }
    if (fabs(qk) < biginv || fabs(pk) < biginv){ pkm2 *= big; pkm1 *= big; qkm2 *= big; qkm1 *= big; }
  }
  return ans;
}

// pseries at x = 0.5 for integer b (here b = 2: the only b with b*x <= 1 that reaches incbet): the factor (n - b) makes the term with
// n == b zero, which ends the series — the bound in the loop's head is never what stops it
CR_FN double hs_rec_pseries(const double* t, double a, double b){
  const double ai = 1.0/a;
  double u = (1.0 - b)*0.5, v = u/(a + 1.0);
  const double t1 = v, z = HS_REC_MACHEP*ai;
  double tm = u, n = 2.0, s = 0.0;
  while (fabs(v) > z && n <= b){
    u = (n - b)*0.5/n;
    tm *= u;
    v = tm/(a + n);
    s += v;
    n += 1.0;
  }
  s += t1;
  s += ai;
  u = a*HS_REC_LOG_HALF;
  if ((a + b) < HS_REC_MAXGAM && fabs(u) < HS_REC_MAXLOG){
    const double g = HS_REC_GAMMA(a + b)/(HS_REC_GAMMA(a)*HS_REC_GAMMA(b));
    s = s*g*hs_rec_pow_half((int)a);
  } else {
    const double y = HS_REC_LGAM(a + b) - HS_REC_LGAM(a) - HS_REC_LGAM(b) + u + cr_log(s);
    s = y < HS_REC_MINLOG ? 0.0 : cr_exp(y);
  }
  return s;
}

// bdtr(k, n, 0.5) for 0 <= k < n - k, n + 1 < HS_REC_TABLE_N
CR_FN double hs_rec_bdtr_half(const double* t, int k, int n){
  if (k == 0) return hs_rec_pow_half(n);
  const double a = n - k, b = k + 1;
  if (b*0.5 <= 1.0) return hs_rec_pseries(t, a, b);
  double y = 0.5*(a + b - 2.0) - (a - 1.0);
  const double w = y < 0.0 ? hs_rec_cfrac(a, b, false) : hs_rec_cfrac(a, b, true)/0.5;
  y = a*HS_REC_LOG_HALF;
  double r = b*HS_REC_LOG_HALF;
  if ((a + b) < HS_REC_MAXGAM && fabs(y) < HS_REC_MAXLOG && fabs(r) < HS_REC_MAXLOG){
    r = hs_rec_pow_half(k + 1);
    r *= hs_rec_pow_half(n - k);
    r /= a;
    r *= w;
    r *= HS_REC_GAMMA(a + b)/(HS_REC_GAMMA(a)*HS_REC_GAMMA(b));
    return r;
  }
  y += r + HS_REC_LGAM(a + b) - HS_REC_LGAM(a) - HS_REC_LGAM(b);
  y += cr_log(w/a);
  return y < HS_REC_MINLOG ? 0.0 : cr_exp(y);
}

// log10, correctly rounded (but for arguments within 2^-98 of a rounding boundary): cr_log_core's double-double times 1/ln 10
CR_FN double hs_rec_log10(double x){
  if (x == 0.0) return cr_from_bits(0xfff0000000000000ull);
  if (x == 1.0) return 0.0;
  cr_dd c; c.h = 0x1.bcb7b1526e50ep-2; c.l = 0x1.95355baaafad3p-57;          // 1/ln 10 = h + l to 2^-110
  return cr_dd_mul(cr_log_core(x), c).h;
}

CR_FN double hs_rec_allele_bias(const double* t, int one, int two){
  const int total = one + two;
  if (total == 0) return 1.0;
  if (one == two) return 0.0;
  const double pv = 2*hs_rec_bdtr_half(t, one < two ? one : two, total);
  return hs_rec_log10(pv < 1.0 ? pv : 1.0);
}

CR_FN double hs_rec_lbinom(const double* t, int n, int k){
  if (k == 0 || n == k) return 0.0;
  return HS_REC_LGAMMA(n + 1) - HS_REC_LGAMMA(k + 1) - HS_REC_LGAMMA(n - k + 1);
}
CR_FN double hs_rec_hypergeo(const double* t, int n11, int n1_, int n_1, int n){
  return cr_exp(hs_rec_lbinom(t, n1_, n11) + hs_rec_lbinom(t, n - n1_, n_1 - n11) - hs_rec_lbinom(t, n, n_1));
}
// one step of kt_fisher_exact's walk: from `at` (probability p) to `to`
CR_FN double hs_rec_walk(const double* t, int to, int* at, double p, int n1_, int n_1, int n){
  const int from = *at;
  *at = to;
  if (to%11 && to + n - n1_ - n_1){
    if (to == from + 1) return p*((double)(n1_ - from)/to*(n_1 - from)/(to + n - n1_ - n_1));
    if (to == from - 1) return p*((double)from/(n1_ - to)*(from + n - n1_ - n_1)/(n_1 - to));
  }
  return hs_rec_hypergeo(t, to, n1_, n_1, n);
}
// log10(min(1, two)) of kt_fisher_exact(u1 - rv1, rv1, u2 - rv2, rv2); u1 + u2 + 1 < HS_REC_TABLE_N
CR_FN double hs_rec_strand_bias(const double* t, int u1, int rv1, int u2, int rv2){
  const int n11 = u1 - rv1, n1_ = u1, n_1 = n11 + (u2 - rv2), n = u1 + u2;
  const int hi = n_1 < n1_ ? n_1 : n1_;
  int lo = n1_ + n_1 - n;
  if (lo < 0) lo = 0;
  if (lo == hi) return 0.0;                      // two = 1
  int at = n11;
  const double q = hs_rec_hypergeo(t, n11, n1_, n_1, n);
  double p = hs_rec_walk(t, lo, &at, q, n1_, n_1, n), left = 0.0, right = 0.0;
  for (int i = lo + 1; p < 0.99999999*q && i <= hi; ++i){ left += p; p = hs_rec_walk(t, i, &at, p, n1_, n_1, n); }
  if (p < 1.00000001*q) left += p;
  p = hs_rec_walk(t, hi, &at, p, n1_, n_1, n);
  for (int j = hi - 1; p < 0.99999999*q && j >= 0; --j){ right += p; p = hs_rec_walk(t, j, &at, p, n1_, n_1, n); }
  if (p < 1.00000001*q) right += p;
  double two = left + right;
  if (two > 1.0) two = 1.0;
  return hs_rec_log10(two < 1.0 ? two : 1.0);
}
