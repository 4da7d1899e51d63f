// record_reads_host.h — the host twin of record_reads.hip (record_reads_host.cpp; plain C++, no HIP): ExtractCigar
// (extract_indels.cpp:18-90) per read, Genotyper::condense_read_counts (genotyper.h:50-63) per sample, and the read loop of
// GenotyperBamProcessor::learn_stutter_model (genotyper_bam_processor.cpp:113-139).  Equals the compiled reference on
// tests/golden/record_reads_*.npz.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/hipstr_hmm.h"

namespace hipstr_record_reads {

// One read: true and bp_diff, or false (bp_diff = 0).  Stated over the runs' positions, not as the reference's two walks: run i begins at
// at[i] and ends before at[i+1] on the reference.
bool extract_cigar(const uint8_t* op, const int32_t* len, int n, int32_t start, int32_t region_start, int32_t region_end, int32_t* bp_diff);

// "" or the refusal of a request; on success n_reads / n_runs and the padded regions [n_loci] each
std::string check_cigars(const hipstr_cigar_request_t* rq, int64_t* n_reads, int64_t* n_runs, std::vector<int32_t>* pad_start, std::vector<int32_t>* pad_end);
void cigars(const hipstr_cigar_request_t* rq, const int32_t* pad_start, const int32_t* pad_end, uint8_t* got, int32_t* bp_diff);

// The samples of a batch as runs of reads: begin[s], count[s] for s in sample_total_ll's order (a sample without reads: count 0).
// "" or the refusal.
std::string sample_runs(const hipstr_post_batch_t* pb, std::vector<int32_t>* begin, std::vector<int32_t>* count);
// One sample: the distinct values other than skip, ascending, with their counts, at value[0 ..] / count[0 ..]; returns the number of pairs
int condense(const int32_t* v, int n, int32_t skip, int32_t* value, int32_t* count);

}  // namespace hipstr_record_reads
