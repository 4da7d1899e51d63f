// record_reads_layout.h — what record_reads.hip's kernels and the host share: the caps, the argument blocks, and the bodies of a lane — the
// CIGAR walk of one read, and the per-element steps of a sample's histogram (rank in the sorted order, run head).  The bodies are plain
// C++ (tests/cpp/record_reads_host_test.cpp runs them on the host against record_reads_host.cpp).
//
// Every loop has its bound in its head: a read's runs (at most HS_RR_CIGAR_RUNS on the device), a sample's values (at most
// HS_RR_HIST_READS on the device).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define HS_RR_FN static __host__ __device__ __attribute__((unused)) inline
#else
#define HS_RR_FN static __attribute__((unused)) inline
#endif

#define HS_RR_CIGAR_THREADS 256       // reads per workgroup of the CIGAR kernel, one lane each
#define HS_RR_CIGAR_RUNS 4096         // == HIPSTR_CIGAR_DEVICE_RUNS: a read with more runs is the host twin's (one lane would hold its wavefront)
#define HS_RR_WAVE 64                 // the histogram kernels: one wavefront per sample
#define HS_RR_HIST_READS 1024         // == HIPSTR_HISTOGRAM_DEVICE_READS: three int32 arrays of this length in LDS (12 KB)
#define HS_RR_SCAN_CHUNK 256          // samples per chunk of the scan (one workgroup, the base carried from chunk to chunk)

struct hs_rr_cigar_dev_t {            // hipstr_cigar_bp_diffs
  const int32_t *read_locus, *read_start, *cigar_off;      // [n_reads], [n_reads], [n_reads+1]
  const uint8_t* cigar_op; const int32_t* cigar_len;       // [n_runs]
  const int32_t *pad_start, *pad_end;                      // [n_loci] region_start - pad, region_stop + pad
  uint8_t* got; int32_t* bp_diff;                          // [n_reads]
  int32_t n_reads, n_loci;
};

struct hs_rr_unit_t { int32_t read_begin, n_reads, big_off, pad_; };       // a sample: its reads; big_off >= 0: condensed by the host, pairs at big_*[big_off ..]
struct hs_rr_hist_dev_t {             // hipstr_sample_histograms
  const hs_rr_unit_t* units;          // [n_samp]
  const int32_t* value;               // [n_reads]
  const int32_t *big_value, *big_count;                    // the host's pairs of the samples beyond the cap
  int32_t* n_pairs;                   // [n_samp]: uploaded with the host's counts, the kernel writes the rest
  int32_t *tmp_value, *tmp_count;     // [n_reads]: a sample's pairs at its first read
  int32_t *pair_off, *hist_value, *hist_count;             // [n_samp+1], [n_reads], [n_reads]
  int32_t n_samp, n_reads, skip;
};

// ---- ExtractCigar for one read (extract_indels.cpp:18-90); the caller has checked that start + every length summed stays in int32
HS_RR_FN bool hs_rr_ref_op(uint8_t t){ return t == 'M' || t == '=' || t == 'X' || t == 'D'; }
HS_RR_FN bool hs_rr_match_op(uint8_t t){ return t == 'M' || t == '=' || t == 'X'; }
HS_RR_FN int hs_rr_cigar_lane(const uint8_t* op, const int32_t* len, int n, int start, int region_start, int region_end, int32_t* bp_diff){
  *bp_diff = 0;
  int span = 0;
  for (int i = 0; i < n; i++) if (hs_rr_ref_op(op[i])) span += len[i];
  if (region_start < start || region_end >= start + span) return 0;                   // :39-40
  int pos = start, first = 0;
  for (int i = 0; i < n && pos < region_start; i++){                                  // :43-53
    if (hs_rr_ref_op(op[i])) pos += len[i];
    if (hs_rr_match_op(op[i])) first = i;
  }
  if (first == 0 && !hs_rr_match_op(op[0])) return 0;                                 // :54-58
  int last = n - 1;
  pos = start + span;
  for (int i = n - 1; i >= 0 && pos > region_end; i--){                               // :64-75
    if (hs_rr_ref_op(op[i])) pos -= len[i];
    if (hs_rr_match_op(op[i])) last = i;
  }
  if (last == n - 1 && !hs_rr_match_op(op[n - 1])) return 0;                          // :76-80
  int d = 0;
  for (int i = first; i <= last; i++) d += op[i] == 'I' ? len[i] : op[i] == 'D' ? -len[i] : 0;
  *bp_diff = d;
  return 1;
}

// ---- a sample's histogram: element i of the m kept values goes to the number of values that sort before it (equal values in index order)
HS_RR_FN int hs_rr_rank(const int32_t* v, int m, int i){
  const int32_t x = v[i];
  int r = 0;
  for (int j = 0; j < m; j++) r += (v[j] < x || (v[j] == x && j < i)) ? 1 : 0;
  return r;
}
HS_RR_FN bool hs_rr_is_head(const int32_t* sorted, int k){ return k == 0 || sorted[k] != sorted[k - 1]; }
