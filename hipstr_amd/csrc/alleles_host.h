// alleles_host.h — the host form of the allele-set update (alleles_host.cpp; plain C++, no HIP): the checks and the counts and offsets
// both forms start from, one locus' strings, mapping and mask at a time, and genotype()'s policy around it (hipstr_alleles_step).
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/hipstr_hmm.h"

// the library-owned result: the rebuilt haplotype side, the two batches that point into it
struct hipstr_alleles {
  std::vector<int32_t> blk_nopts, opt_off, hap_off, mapping, new_n, h2a[3];
  std::vector<char> seq;
  std::vector<uint8_t> realign, added;
  hipstr_batch_t batch, batch_all;
};

namespace hipstr_al {

// What follows from the flags and the add counts alone (no string is touched): per locus where its old and new options and haplotypes
// start, per new option where its bytes come from, and — in the result — blk_nopts, opt_off, hap_off, new_n, added, every array sized.
struct Plan {
  const hipstr_alleles_request_t* rq = NULL;
  const hipstr_batch_t* b = NULL;
  int nl = 0;
  std::vector<int32_t> o_opt0, n_opt0;       // [nl+1] first old / new option of a locus
  std::vector<int32_t> n_src;                // [new options] >= 0: offset into b->seq; < 0: -1 - offset into rq->add_seq
  std::vector<uint8_t> on;                   // [nl] 0 = the identity
};
// every refusal of include/hipstr_hmm.h; 0 = fine, else err is the message (nothing of `a` is to be used)
int plan(const hipstr_alleles_request_t* rq, Plan& P, hipstr_alleles& a, std::string& err);
// the new option strings of locus l into a.seq
void gather_locus(const Plan& P, int l, hipstr_alleles& a);
// mapping, mask and hap_to_allele rows of a locus that is off
void identity_locus(const Plan& P, int l, hipstr_alleles& a);
// the same of a locus that is on (its strings gathered): the table and the byte comparisons; counts[0] += probes, counts[1] += comparisons
void map_locus(const Plan& P, int l, hipstr_alleles& a, int hash_bits, int64_t counts[2]);
// the two batches, once every array is final
void finish(const Plan& P, hipstr_alleles& a);
// the whole batch on the host; NULL + err on a refusal.  counts: loci on the device (0), loci done by the host code, probes, comparisons
hipstr_alleles* apply_host(const hipstr_alleles_request_t* rq, int hash_bits, int64_t counts[4], std::string& err);

// genotype()'s policy for one census: the request for apply, the phases after it and the per-locus numbers; nothing of the caller's is written
struct Step {
  std::vector<uint8_t> on, keep;
  std::vector<int32_t> add_off, add_seq_off, phase, status, n_added, n_removed, n_affected;
  std::vector<char> add_seq;
  int32_t any_added = 0;
  hipstr_alleles_request_t rq;
};
int step_plan(const hipstr_batch_t* pooled, const hipstr_census_out_t* census, const int32_t* phase, int32_t max_total_haplotypes, Step& S, std::string& err);

}  // namespace hipstr_al
