// record_host.cpp — see record_host.h.  Every routine follows the operation order of the reference's compiled code (lib/cephes: bdtr.c,
// incbet.c, gamma.c, polevl.c; lib/htslib/kfunc.c), so that with the same libm the results are the same bits.
#include "record_host.h"

#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace hipstr_record {
namespace {

const double MACHEP = 1.11022302462515654042E-16;      // 2^-53
const double MAXLOG = 7.09782712893383996732E2;
const double MINLOG = -7.451332191019412076235E2;
const double MAXGAM = 171.624376956302725;
const double BIG = 4.503599627370496e15, BIGINV = 2.22044604925031308085e-16;

// Horner, highest coefficient first; horner1: the leading coefficient is an implied 1
double horner(double x, const double* c, int n){
  double r = c[0];
  for (int i = 1; i <= n; i++) r = r*x + c[i];
  return r;
}
double horner1(double x, const double* c, int n){
  double r = x + c[0];
  for (int i = 1; i < n; i++) r = r*x + c[i];
  return r;
}

// gamma on [2, 3): rational approximation
const double GP[7] = { 1.60119522476751861407E-4, 1.19135147006586384913E-3, 1.04213797561761569935E-2, 4.76367800457137231464E-2,
                       2.07448227648435975150E-1, 4.94214826801497100753E-1, 9.99999999999999996796E-1 };
const double GQ[8] = { -2.31581873324120129819E-5, 5.39605580493303397842E-4, -4.45641913851797240494E-3, 1.18139785222060435552E-2,
                       3.58236398605498653373E-2, -2.34591795718243348568E-1, 7.14304917030273074085E-2, 1.00000000000000000320E0 };
// Stirling's series for gamma, 33 <= x <= 172
const double STIR[5] = { 7.87311395793093628397E-4, -2.29549961613378126380E-4, -2.68132617805781232825E-3, 3.47222221605458667310E-3,
                         8.33333333333482257126E-2 };
const double MAXSTIR = 143.01608, SQTPI = 2.50662827463100050242E0;
// log gamma: Stirling's expansion, and the rational approximation on [2, 3)
const double LA[5] = { 8.11614167470508450300E-4, -5.95061904284301438324E-4, 7.93650340457716943945E-4, -2.77777777730099687205E-3,
                       8.33333333333331927722E-2 };
const double LB[6] = { -1.37825152569120859100E3, -3.88016315134637840924E4, -3.31612992738871184744E5, -1.16237097492762307383E6,
                       -1.72173700820839662146E6, -8.53555664245765465627E5 };
const double LC[6] = { -3.51815701436523470549E2, -1.70642106651881159223E4, -2.20528590553854454839E5, -1.13933444367982507207E6,
                       -2.53252307177582951285E6, -2.01889141433532773231E6 };
const double LS2PI = 0.91893853320467274178, MAXLGM = 2.556348e305;

double stirling_gamma(double x){
  double w = 1.0/x;
  w = 1.0 + w*horner(w, STIR, 4);
  double y = exp(x);
  if (x > MAXSTIR){                  // pow would overflow: in two halves
    const double v = pow(x, 0.5*x - 0.25);
    y = v*(v/y);
  } else
    y = pow(x, x - 0.5)/y;
  return SQTPI*y*w;
}

// incbet's two continued fractions share everything but the sign pattern of their coefficients: `second` selects incbd (argument
// z = x/(1-x), k2 falling and k6 rising) against incbcf (argument x, k2 rising and k6 falling)
double continued_fraction(double a, double b, double x, bool second){
  double k1 = a, k2 = second ? b - 1.0 : a + b, k3 = a, k4 = a + 1.0, k5 = 1.0, k6 = second ? a + b : b - 1.0, k7 = a + 1.0, k8 = a + 2.0;
  const double z = second ? x/(1.0 - x) : x, d2 = second ? -1.0 : 1.0, d6 = -d2;
  double pkm2 = 0.0, qkm2 = 1.0, pkm1 = 1.0, qkm1 = 1.0, ans = 1.0, r = 1.0;
  const double thresh = 3.0*MACHEP;
  for (int n = 0; n < 300; n++){
    double xk = -(z*k1*k2)/(k3*k4);
    double pk = pkm1 + pkm2*xk, qk = qkm1 + qkm2*xk;
    pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;
    xk = (z*k5*k6)/(k7*k8);
    pk = pkm1 + pkm2*xk; qk = qkm1 + qkm2*xk;
    pkm2 = pkm1; pkm1 = pk; qkm2 = qkm1; qkm1 = qk;
    if (qk != 0) r = pk/qk;
    double t = 1.0;
    if (r != 0){ t = fabs((ans - r)/r); ans = r; }
    if (t < thresh) break;
    k1 += 1.0; k2 += d2; k3 += 2.0; k4 += 2.0; k5 += 1.0; k6 += d6; k7 += 2.0; k8 += 2.0;
    if (fabs(qk) + fabs(pk) > BIG){ pkm2 *= BIGINV; pkm1 *= BIGINV; qkm2 *= BIGINV; qkm1 *= BIGINV; }
    if (fabs(qk) < BIGINV || fabs(pk) < BIGINV){ pkm2 *= BIG; pkm1 *= BIG; qkm2 *= BIG; qkm1 *= BIG; }
  }
  return ans;
}

// the power series, for small b*x
double power_series(double a, double b, double x){
  const double ai = 1.0/a;
  double u = (1.0 - b)*x, v = u/(a + 1.0);
  const double t1 = v, z = MACHEP*ai;
  double t = u, n = 2.0, s = 0.0;
  while (fabs(v) > z){
    u = (n - b)*x/n;
    t *= u;
    v = t/(a + n);
    s += v;
    n += 1.0;
  }
  s += t1;
  s += ai;
  u = a*log(x);
  if ((a + b) < MAXGAM && fabs(u) < MAXLOG){
    t = gamma_pos(a + b)/(gamma_pos(a)*gamma_pos(b));
    s = s*t*pow(x, a);
  } else {
    t = lgam_pos(a + b) - lgam_pos(a) - lgam_pos(b) + u + log(s);
    s = t < MINLOG ? 0.0 : exp(t);
  }
  return s;
}

// log of the binomial coefficient over libm's lgamma (kfunc.c); the re-entrant form: same value, no write to signgam
double lgamma_of(double x){ int sign; return lgamma_r(x, &sign); }
double log_binomial(int n, int k){
  if (k == 0 || n == k) return 0;
  return lgamma_of(n + 1) - lgamma_of(k + 1) - lgamma_of(n - k + 1);
}
double hypergeometric(int n11, int n1_, int n_1, int n){
  return exp(log_binomial(n1_, n11) + log_binomial(n - n1_, n_1 - n11) - log_binomial(n, n_1));
}
// The walk along n11 with fixed margins: one step up or down updates the probability by a ratio, except at the multiples of 11 and at the
// lower end of the support, where it is evaluated afresh.
struct Walk {
  int n11, n1_, n_1, n; double p;
  double start(int a, int r, int c, int t){ n11 = a; n1_ = r; n_1 = c; n = t; return p = hypergeometric(n11, n1_, n_1, n); }
  double move(int to){
    if (to%11 && to + n - n1_ - n_1){
      if (to == n11 + 1){
        p *= (double)(n1_ - n11)/to*(n_1 - n11)/(to + n - n1_ - n_1);
        n11 = to;
        return p;
      }
      if (to == n11 - 1){
        p *= (double)n11/(n1_ - to)*(n11 + n - n1_ - n_1)/(n_1 - to);
        n11 = to;
        return p;
      }
    }
    n11 = to;
    return p = hypergeometric(n11, n1_, n_1, n);
  }
};

}  // namespace

double gamma_pos(double x){
  if (x > 33.0) return stirling_gamma(x);
  double z = 1.0;
  while (x >= 3.0){ x -= 1.0; z *= x; }
  while (x < 2.0){ z /= x; x += 1.0; }
  if (x == 2.0) return z;
  x -= 2.0;
  return z*horner(x, GP, 6)/horner(x, GQ, 7);
}

double lgam_pos(double x){
  if (x < 13.0){
    double z = 1.0, p = 0.0, u = x;
    while (u >= 3.0){ p -= 1.0; u = x + p; z *= u; }
    while (u < 2.0){ z /= u; p += 1.0; u = x + p; }
    if (z < 0.0) z = -z;
    if (u == 2.0) return log(z);
    p -= 2.0;
    x = x + p;
    p = x*horner(x, LB, 5)/horner1(x, LC, 6);
    return log(z) + p;
  }
  if (x > MAXLGM) return INFINITY;
  double q = (x - 0.5)*log(x) - x + LS2PI;
  if (x > 1.0e8) return q;
  const double p = 1.0/(x*x);
  if (x >= 1000.0)
    q += ((7.9365079365079365079365e-4*p - 2.7777777777777777777778e-3)*p + 0.0833333333333333333333)/x;
  else
    q += horner(p, LA, 4)/x;
  return q;
}

double incbet(double aa, double bb, double xx){
  if (aa <= 0.0 || bb <= 0.0) return 0.0;
  if (xx <= 0.0 || xx >= 1.0) return xx == 1.0 ? 1.0 : 0.0;
  bool flipped = false;
  double a, b, x, xc, t;
  if (bb*xx <= 1.0 && xx <= 0.95) return power_series(aa, bb, xx);
  double w = 1.0 - xx;
  if (xx > aa/(aa + bb)){ flipped = true; a = bb; b = aa; xc = xx; x = w; }      // x beyond the mean: the other tail
  else { a = aa; b = bb; xc = w; x = xx; }
  if (flipped && b*x <= 1.0 && x <= 0.95)
    t = power_series(a, b, x);
  else {
    double y = x*(a + b - 2.0) - (a - 1.0);
    w = y < 0.0 ? continued_fraction(a, b, x, false) : continued_fraction(a, b, x, true)/xc;
    // times x^a (1-x)^b Gamma(a+b) / (a Gamma(a) Gamma(b))
    y = a*log(x);
    t = b*log(xc);
    if ((a + b) < MAXGAM && fabs(y) < MAXLOG && fabs(t) < MAXLOG){
      t = pow(xc, b);
      t *= pow(x, a);
      t /= a;
      t *= w;
      t *= gamma_pos(a + b)/(gamma_pos(a)*gamma_pos(b));
    } else {
      y += t + lgam_pos(a + b) - lgam_pos(a) - lgam_pos(b);
      y += log(w/a);
      t = y < MINLOG ? 0.0 : exp(y);
    }
  }
  if (flipped) t = t <= MACHEP ? 1.0 - MACHEP : 1.0 - t;
  return t;
}

double bdtr(int k, int n, double p){
  if (p < 0.0 || p > 1.0 || k < 0 || n < k) return 0.0;
  if (k == n) return 1.0;
  const double dn = n - k;
  if (k == 0) return pow(1.0 - p, dn);
  return incbet(dn, k + 1, 1.0 - p);
}

double fisher_two(int n11, int n12, int n21, int n22){
  const int n1_ = n11 + n12, n_1 = n11 + n21, n = n11 + n12 + n21 + n22;
  const int hi = n_1 < n1_ ? n_1 : n1_;
  int lo = n1_ + n_1 - n;
  if (lo < 0) lo = 0;
  if (lo == hi) return 1.0;
  Walk wk;
  const double q = wk.start(n11, n1_, n_1, n);
  double p = wk.move(lo), left = 0.0, right = 0.0;
  for (int i = lo + 1; p < 0.99999999*q && i <= hi; ++i){ left += p; p = wk.move(i); }
  if (p < 1.00000001*q) left += p;
  p = wk.move(hi);
  for (int j = hi - 1; p < 0.99999999*q && j >= 0; --j){ right += p; p = wk.move(j); }
  if (p < 1.00000001*q) right += p;
  const double two = left + right;
  return two > 1.0 ? 1.0 : two;
}

double allele_bias(int one, int two){
  const int total = one + two;
  if (total == 0) return 1;
  if (one == two) return 0.0;
  const double pvalue = 2*bdtr(std::min(one, two), total, 0.5);
  return log10(std::min(1.0, pvalue));
}

double strand_bias(int uniq_one, int rv_one, int uniq_two, int rv_two){
  return log10(std::min(1.0, fisher_two(uniq_one - rv_one, rv_one, uniq_two - rv_two, rv_two)));
}

std::string check_counts(int32_t u1, int32_t u2, int32_t rv1, int32_t rv2){
  if (u1 < 0 || u2 < 0 || rv1 < 0 || rv2 < 0) return "a negative read count";
  if (rv1 > u1 || rv2 > u2) return "rv_uniq exceeds uniq";
  if ((int64_t)u1 + u2 > INT32_MAX) return "read counts too large";
  return "";
}

void fill_table(double* t, int n){
  for (int i = 0; i < n; i++){
    t[3*i] = i == 0 ? INFINITY : (i > 171 ? INFINITY : gamma_pos(i));
    t[3*i + 1] = i == 0 ? INFINITY : lgam_pos(i);
    t[3*i + 2] = lgamma_of((double)i);
  }
}

bool null_request(const hipstr_record_request_t* rq){
  return !rq || !rq->n_variants || !rq->hap_to_allele || !rq->n_aligned || !rq->n_snp || !rq->n_stutter || !rq->n_flank_indel || !rq->uniq_one ||
         !rq->uniq_two || !rq->rv_uniq_one || !rq->rv_uniq_two;
}
bool null_out(const hipstr_record_out_t* out){
  return !out || !out->status || !out->gt || !out->ab || !out->dab || !out->fs || !out->n_skip || !out->n_filt || !out->an || !out->dp ||
         !out->dsnp || !out->dstutter || !out->dflankindel || !out->allele_count;
}

std::string check_request(int n_loci, const int32_t* n_alleles, const int32_t* n_samples, const hipstr_record_request_t* rq){
  if (!(rq->max_flank_indel_frac >= 0)) return "max_flank_indel_frac must not be negative";
  int64_t ho = 0, so = 0;
  for (int l = 0; l < n_loci; l++){
    const int V = rq->n_variants[l], A = n_alleles[l], S = n_samples[l];
    if (V < 1) return "n_variants below 1";
    if (A < 1 || S < 0) return "allele or sample count out of range";
    for (int a = 0; a < A; a++)
      if (rq->hap_to_allele[ho + a] < 0 || rq->hap_to_allele[ho + a] >= V) return "hap_to_allele outside [0, n_variants)";
    for (int64_t s = so; s < so + S; s++){
      const std::string why = check_counts(rq->uniq_one[s], rq->uniq_two[s], rq->rv_uniq_one[s], rq->rv_uniq_two[s]);
      if (!why.empty()) return why;
      if (rq->n_aligned[s] < 0 || rq->n_snp[s] < 0 || rq->n_stutter[s] < 0 || rq->n_flank_indel[s] < 0) return "a negative read count";
    }
    ho += A; so += S;
  }
  return "";
}

std::string fields(int n_loci, const int32_t* n_alleles, const int32_t* n_samples, const uint8_t* haploid, const int32_t* map_gt,
                   const hipstr_record_request_t* rq, hipstr_record_out_t* out){
  const std::string why = check_request(n_loci, n_alleles, n_samples, rq);
  if (!why.empty()) return why;
  const float frac = flank_frac_of(rq);
  // first pass: what would be refused (nothing is written before that is known)
  int64_t ho = 0, so = 0;
  for (int l = 0; l < n_loci; l++){
    const int A = n_alleles[l], S = n_samples[l];
    const bool hap = haploid && haploid[l];
    for (int64_t s = so; s < so + S; s++){
      const int ha = map_gt[2*s], hb = map_gt[2*s + 1];
      if (ha < -1 || ha >= A || hb < -1 || hb >= A || (ha < 0) != (hb < 0)) return "map_gt outside [-1, n_alleles)";
      const bool reported = !rq->sample_reported || rq->sample_reported[s], masked = rq->sample_masked && rq->sample_masked[s];
      if (!reported || rq->n_aligned[s] == 0 || masked || over_flank_frac(rq->n_flank_indel[s], rq->n_aligned[s], frac)) continue;
      if (ha < 0) return "a sample with reads and without a MAP pair";
      if (hap && rq->hap_to_allele[ho + ha] != rq->hap_to_allele[ho + hb]) return "a heterozygous genotype at a haploid locus";
    }
    ho += A; so += S;
  }
  ho = so = 0;
  int64_t vo = 0;
  for (int l = 0; l < n_loci; l++){
    const int A = n_alleles[l], S = n_samples[l], V = rq->n_variants[l];
    const bool hap = haploid && haploid[l];
    int32_t* ac = out->allele_count + vo;
    for (int v = 0; v < V; v++) ac[v] = 0;
    int32_t skip = 0, filt = 0, an = 0, dp = 0, dsnp = 0, dstutter = 0, dfi = 0;
    for (int64_t s = so; s < so + S; s++){
      const int ha = map_gt[2*s], hb = map_gt[2*s + 1];
      const int g0 = ha < 0 ? -1 : rq->hap_to_allele[ho + ha], g1 = hb < 0 ? -1 : rq->hap_to_allele[ho + hb];
      const bool reported = !rq->sample_reported || rq->sample_reported[s], masked = rq->sample_masked && rq->sample_masked[s];
      const int32_t na = rq->n_aligned[s];
      const bool over = na > 0 && over_flank_frac(rq->n_flank_indel[s], na, frac);
      // :1163-1187
      if (reported && na != 0){
        if (over) filt++;
        else if (masked) skip++;
        else if (hap){ ac[g0]++; an++; }
        else { ac[g0]++; ac[g1]++; an += 2; }
      }
      // :1238-1254
      if (reported && !masked && !over){ dp += na; dsnp += rq->n_snp[s]; dstutter += rq->n_stutter[s]; dfi += rq->n_flank_indel[s]; }
      // :1326-1375
      const int status = !reported ? HIPSTR_RECORD_NOT_REPORTED : na == 0 ? HIPSTR_RECORD_NO_READS : masked ? HIPSTR_RECORD_MASKED :
                         over ? HIPSTR_RECORD_FLANK_INDEL_FRAC : HIPSTR_RECORD_PASS;
      out->status[s] = status; out->gt[2*s] = g0; out->gt[2*s + 1] = g1;
      if (status == HIPSTR_RECORD_PASS && !hap && ha != hb){
        out->ab[s] = allele_bias(rq->uniq_one[s], rq->uniq_two[s]);
        out->dab[s] = rq->uniq_one[s] + rq->uniq_two[s];
        out->fs[s] = strand_bias(rq->uniq_one[s], rq->rv_uniq_one[s], rq->uniq_two[s], rq->rv_uniq_two[s]);
      } else {
        out->ab[s] = out->fs[s] = HIPSTR_RECORD_NOT_APPLICABLE; out->dab[s] = 0;
      }
    }
    out->n_skip[l] = skip; out->n_filt[l] = filt; out->an[l] = an;
    out->dp[l] = dp; out->dsnp[l] = dsnp; out->dstutter[l] = dstutter; out->dflankindel[l] = dfi;
    ho += A; so += S; vo += V;
  }
  return "";
}

}  // namespace hipstr_record
