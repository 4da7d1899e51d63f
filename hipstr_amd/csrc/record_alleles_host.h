// record_alleles_host.h — the host twin of record_alleles.hip (record_alleles_host.cpp; plain C++, no HIP): SeqStutterGenotyper::get_alleles
// (seq_stutter_genotyper.cpp:691-769), reorder_alleles (:673-689) and the flank option strings of :1013-1040, on std::string as the
// reference has them.  Equals the compiled reference on tests/golden/record_alleles_*.npz.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/hipstr_hmm.h"

namespace hipstr_rec_alleles {

struct Locus {                        // one locus' result
  int32_t status = 0, pos = 0, left_trim = 0, right_trim = 0;
  std::vector<std::string> alleles;   // block-option order; empty for a failed locus
  std::vector<int32_t> bp_diff, old_to_new, new_to_old;
};

// get_alleles + reorder_alleles.  options: block 1's; win[i] = chrom_seq[region_start - 40 + i], win_len bytes.
void alleles_of(const std::vector<std::string>& options, int32_t start, int32_t end, int32_t region_start, int32_t region_stop,
                const char* win, int32_t win_len, Locus* out);
// allele 0 first, the rest by (length, bytes); false when two strings are equal (the maps are not written then)
bool reorder(const std::vector<std::string>& alleles, std::vector<int32_t>* old_to_new, std::vector<int32_t>* new_to_old);
// :1013-1040 from the returned pair; false where an assert would fire or the reference's substr throws (the outputs are cleared)
bool flank_options(const std::vector<std::string>& lopts, const std::vector<std::string>& ropts, const std::string& ref_str, int left_trim, int right_trim,
                   std::vector<std::string>* lflanks, std::vector<std::string>* rflanks);

// "" or the refusal of a call's arguments; on success the options' count of block 1 summed over the loci
std::string check(const hipstr_batch_t* b, const hipstr_record_alleles_request_t* rq, const hipstr_record_alleles_out_t* out, int64_t* n_var);
// block `blk` of locus l as strings; opt_base: the index of the locus' first option in opt_off
std::vector<std::string> block_options(const hipstr_batch_t* b, int64_t opt_base, int l, int blk);
// The outputs from the loci's results (status flags for the flanks are or-ed in here).  "" or the refusal (a capacity): nothing is written then.
std::string emit(const hipstr_batch_t* b, std::vector<Locus>& loci, hipstr_record_alleles_out_t* out);

}  // namespace hipstr_rec_alleles
