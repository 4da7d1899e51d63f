// record_reads_host.cpp — see record_reads_host.h.
#include "record_reads_host.h"

#include <algorithm>
#include <limits.h>

namespace hipstr_record_reads {

namespace {
inline bool on_ref(uint8_t t){ return t == 'M' || t == '=' || t == 'X' || t == 'D'; }
inline bool is_match(uint8_t t){ return t == 'M' || t == '=' || t == 'X'; }
inline bool sam_op(uint8_t t){ return t == 'M' || t == 'I' || t == 'D' || t == 'N' || t == 'S' || t == 'H' || t == 'P' || t == '=' || t == 'X'; }
}  // namespace

bool extract_cigar(const uint8_t* op, const int32_t* len, int n, int32_t start, int32_t region_start, int32_t region_end, int32_t* bp_diff){
  *bp_diff = 0;
  thread_local std::vector<int64_t> at;
  at.resize((size_t)n + 1);
  at[0] = start;
  for (int i = 0; i < n; i++) at[i + 1] = at[i] + (on_ref(op[i]) ? len[i] : 0);
  if (region_start < start || region_end >= at[n]) return false;                      // :39-40
  // the walk from the front visits the runs that begin before the region and remembers the last match among them (:43-53)
  int first = 0;
  for (int i = 0; i < n && at[i] < region_start; i++) if (is_match(op[i])) first = i;
  if (first == 0 && !is_match(op[0])) return false;                                   // :54-58
  // the walk from the back visits the runs that end behind the region's last base and remembers the lowest match among them (:64-75)
  int last = n - 1;
  for (int i = n - 1; i >= 0 && at[i + 1] > region_end; i--) if (is_match(op[i])) last = i;
  if (last == n - 1 && !is_match(op[n - 1])) return false;                            // :76-80
  int64_t d = 0;
  for (int i = first; i <= last; i++){
    if (op[i] == 'D') d -= len[i];
    else if (op[i] == 'I') d += len[i];
  }
  *bp_diff = (int32_t)d;
  return true;
}

std::string check_cigars(const hipstr_cigar_request_t* rq, int64_t* n_reads, int64_t* n_runs, std::vector<int32_t>* pad_start, std::vector<int32_t>* pad_end){
  const int nl = rq->n_loci;
  if (rq->read_off[0] != 0) return "read_off must begin at 0";
  for (int l = 0; l < nl; l++) if (rq->read_off[l + 1] < rq->read_off[l]) return "read_off must ascend";
  const int64_t nr = rq->read_off[nl];
  if (rq->cigar_off[0] != 0) return "cigar_off must begin at 0";
  pad_start->resize((size_t)nl); pad_end->resize((size_t)nl);
  for (int l = 0; l < nl; l++){
    const int64_t a = (int64_t)rq->region_start[l] - rq->pad[l], b = (int64_t)rq->region_stop[l] + rq->pad[l];
    if (a < INT32_MIN || a > INT32_MAX || b < INT32_MIN || b > INT32_MAX) return "a padded region outside int32";
    if (b < a) return "a padded region_end below its region_start (ExtractCigar asserts)";
    (*pad_start)[l] = (int32_t)a; (*pad_end)[l] = (int32_t)b;
  }
  for (int64_t r = 0; r < nr; r++){
    if (rq->read_start[r] < 0) return "a negative read_start (ExtractCigar asserts)";
    const int32_t c0 = rq->cigar_off[r], c1 = rq->cigar_off[r + 1];
    if (c1 <= c0) return "a read without CIGAR runs";
    int64_t sum = rq->read_start[r];
    for (int32_t c = c0; c < c1; c++){
      if (rq->cigar_len[c] <= 0) return "a CIGAR run of non-positive length";
      if (!sam_op(rq->cigar_op[c])) return "a CIGAR op that is no SAM letter (MIDNSHP=X)";
      sum += rq->cigar_len[c];
    }
    if (sum > INT32_MAX) return "a read whose positions leave int32";
  }
  *n_reads = nr; *n_runs = rq->cigar_off[nr];
  return "";
}

void cigars(const hipstr_cigar_request_t* rq, const int32_t* pad_start, const int32_t* pad_end, uint8_t* got, int32_t* bp_diff){
  for (int l = 0; l < rq->n_loci; l++)
    for (int32_t r = rq->read_off[l]; r < rq->read_off[l + 1]; r++){
      const int32_t c0 = rq->cigar_off[r];
      got[r] = extract_cigar(rq->cigar_op + c0, rq->cigar_len + c0, rq->cigar_off[r + 1] - c0, rq->read_start[r], pad_start[l], pad_end[l], &bp_diff[r]) ? 1 : 0;
    }
}

std::string sample_runs(const hipstr_post_batch_t* pb, std::vector<int32_t>* begin, std::vector<int32_t>* count){
  const int nl = pb->n_loci;
  int64_t ns = 0;
  for (int l = 0; l < nl; l++){
    if (pb->n_samples[l] < 0) return "a negative sample count";
    ns += pb->n_samples[l];
    if (ns > INT32_MAX - 1) return "too many samples for one call";
  }
  if (pb->read_off[0] != 0) return "read_off must begin at 0";
  for (int l = 0; l < nl; l++) if (pb->read_off[l + 1] < pb->read_off[l]) return "read_off must ascend";
  begin->assign((size_t)ns, 0); count->assign((size_t)ns, 0);
  int64_t so = 0;
  for (int l = 0; l < nl; l++){
    const int S = pb->n_samples[l];
    int prev = -1;
    for (int32_t r = pb->read_off[l]; r < pb->read_off[l + 1]; r++){
      const int s = pb->sample_label[r];
      if (s < 0 || s >= S) return "sample_label out of range";
      if (s < prev) return "reads of a locus must be grouped by ascending sample label (genotyper.h:112-119)";
      if (s != prev) (*begin)[(size_t)(so + s)] = r;
      (*count)[(size_t)(so + s)]++;
      prev = s;
    }
    so += S;
  }
  return "";
}

int condense(const int32_t* v, int n, int32_t skip, int32_t* value, int32_t* count){
  thread_local std::vector<int32_t> kept;
  kept.clear();
  for (int i = 0; i < n; i++) if (v[i] != skip) kept.push_back(v[i]);
  std::sort(kept.begin(), kept.end());
  int np = 0;
  for (size_t i = 0; i < kept.size(); i++){
    if (i > 0 && kept[i] == kept[i - 1]) count[np - 1]++;
    else { value[np] = kept[i]; count[np] = 1; np++; }
  }
  return np;
}

}  // namespace hipstr_record_reads
