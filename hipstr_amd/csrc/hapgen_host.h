// hapgen_host.h — the host twin of the haplotype generator (hapgen_host.cpp; plain C++, no HIP): the single statement of what
// hipstr_hapgen_* computes (include/hipstr_hmm.h), one locus at a time, appended to the caller's arrays, and the assembly of the batch
// build_haplotype leaves behind.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/hipstr_hmm.h"

struct hipstr_hapgen_batch { std::vector<uint8_t> mem; hipstr_batch_t batch; const int32_t* locus; const int32_t* status; };

namespace hipstr_hg {

enum { LEFT_PAD = 5, RIGHT_PAD = 5, REF_FLANK_LEN = 35, WIN_PAD = 40 };      // HaplotypeGenerator.h:59-62

inline char fold(char c){ return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }      // uppercase(): toupper in the C locale

// Where the next locus' results go: options / sequence bytes / distinct strings written so far.
struct Sink { hipstr_hapgen_out_t* out; int64_t opts, seq, dist; };

// Every refusal of include/hipstr_hmm.h; on success stop[r] is the stop every later step compares (rq->read_stop, or start + =,X,D runs),
// for reads read_off[0] .. read_off[n_loci].  need_stutter: hipstr_hapgen_batch's extra requirement.  0 = fine, else err is the message.
int check(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, const hipstr_hapgen_out_t* out, bool need_stutter, std::vector<int32_t>& stop, std::string& err);
// 0 / 1 / 2 of a locus from its region and the bounds of its flagged reads (64-bit arithmetic)
int locus_status(int64_t region_start, int64_t region_stop, int64_t chrom_len, int64_t min_flagged_start, int64_t max_flagged_stop);
// trim (HaplotypeGenerator.cpp:12-80) from what it needs of the sequences: the shortest length and the common prefix / suffix up to 5
void trim_amounts(int min_len, int ideal_min_length, int common_prefix, int common_suffix, int& left_trim, int& right_trim);
// Locus l, appended: every per-locus output, the reads' ext_off / ext_len, the options from s.opts / s.seq on (opt_off[s.opts] is written
// by the caller of the first locus), the dist_* entries from s.dist on.  check() has passed.
void locus_host(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, const int32_t* stop, int l, Sink& s);
void hapgen_host(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, const int32_t* stop, hipstr_hapgen_out_t* out);
// room for every output of a call (hipstr_hapgen_batch, the plan)
struct Arrays {
  std::vector<int32_t> i32; std::vector<char> seq; std::vector<double> frac; hipstr_hapgen_out_t out;
  Arrays(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq);
};
// the batch of hipstr_hapgen_batch from a result of (b, rq); the caller frees it with delete
hipstr_hapgen_batch_t* assemble_batch(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, const hipstr_hapgen_out_t* o);

}  // namespace hipstr_hg
