// record_host.h — the host twin of the record fields (record_host.cpp; plain C++, no HIP): the two numerical routines behind the AB and FS
// p-values of SeqStutterGenotyper::write_vcf_record — cephes' bdtr (incbet with incbcf, incbd and pseries; gamma and lgam) and htslib's
// kt_fisher_exact (hypergeo_acc) — restated from their algorithms in the reference's operation order over the host's libm, and the three
// sample loops of the record (seq_stutter_genotyper.cpp:1159-1187, :1238-1254, :1326-1375).  Compiled with -ffp-contract=off like the rest
// of the library; equals the compiled reference bit for bit (tests/golden/record_pvalues.npz).
#pragma once
#include <stdint.h>
#include <string>

#include "../../include/hipstr_hmm.h"

namespace hipstr_record {

// cephes, "UNK" configuration with DENORMAL (lib/cephes/mconf.h, const.c)
double gamma_pos(double x);                     // gamma(x) for x >= 1 (the arguments that occur are integers n - k, k + 1, n + 1)
double lgam_pos(double x);                      // lgam(x) for x >= 1
double incbet(double a, double b, double x);    // 0 < x < 1, a, b > 0
double bdtr(int k, int n, double p);            // 0 <= k <= n
// kt_fisher_exact's `two`
double fisher_two(int n11, int n12, int n21, int n22);

// compute_allele_bias (:965-982) and the strand bias of :1371-1374
double allele_bias(int one, int two);
double strand_bias(int uniq_one, int rv_one, int uniq_two, int rv_two);

// "" or the refusal of a count quadruple
std::string check_counts(int32_t u1, int32_t u2, int32_t rv1, int32_t rv2);

// The device's table: for i in [0, n) the triple gamma_pos(i), lgam_pos(i), libm's lgamma(i) at t[3*i ..]; i = 0 holds +inf (never read
// by a valid quadruple; the Fisher walk below its lower end reads lgamma there, as libm gives it).  gamma is +inf from 172 on.
void fill_table(double* t, int n);

// The record's loops.  n_alleles / haploid: per locus (haploid may be NULL); map_gt: [2*n_samp].  Returns "" or the refusal (nothing
// written then).
std::string fields(int n_loci, const int32_t* n_alleles, const int32_t* n_samples, const uint8_t* haploid, const int32_t* map_gt,
                   const hipstr_record_request_t* rq, hipstr_record_out_t* out);
// the request's and the outputs' null checks; the counts' checks over all samples
bool null_request(const hipstr_record_request_t* rq);
bool null_out(const hipstr_record_out_t* out);
std::string check_request(int n_loci, const int32_t* n_alleles, const int32_t* n_samples, const hipstr_record_request_t* rq);
inline float flank_frac_of(const hipstr_record_request_t* rq){ return rq->max_flank_indel_frac == 0 ? 0.15f : rq->max_flank_indel_frac; }      // genotyper.cpp:343
// (float)n_flank_indel > frac*(float)n_aligned, each operation rounded to float (:1169, :1246, :1347)
inline bool over_flank_frac(int32_t n_flank_indel, int32_t n_aligned, float frac){
  const float rhs = frac*(float)n_aligned;
  return (float)n_flank_indel > rhs;
}

}  // namespace hipstr_record
