// em_input_layout.h — device-side description of the step between a resident traceback result and the stutter EM (em_input.hip:
// hipstr_em_train_dev): the reads SeqStutterGenotyper::recompute_stutter_models hands to EMStutterGenotyper::train
// (seq_stutter_genotyper.cpp:1542-1581), selected, compacted and prepared (allele sizes, the reads' allele indices, the initial allele
// frequencies of em_stutter_genotyper.cpp:10-20) where the records lie.  Every size decision of the stage is taken here; em_input.hip's
// kernels and its host side call these functions, hipstr_debug_em_input_plan reports them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HS_EMI_HD __host__ __device__
#else
#define HS_EMI_HD
#endif

#define HS_EMI_THREADS 256             // threads of every workgroup of the stage (four wavefronts)
#define HS_EMI_WAVE 64                 // reads of a (locus, sample) run a wavefront takes per step
#define HS_EMI_SCAN_CHUNK 256          // runs per chunk of the exclusive scan (a thread per run; the base is carried from chunk to chunk)
#define HS_EMI_SPAN_LIMIT 10000        // == entries of the table of integer logarithms (mathops.cpp:13-21; checked against the table at run time):
                                       // a locus whose sizes, ref_allele included, span fewer values than this is prepared on the device
#define HS_EMI_BITMAP_WORDS ((HS_EMI_SPAN_LIMIT + 31)/32)      // the presence bitmap over [lo, hi] in LDS: 313 words, 1.25 KB
#define HS_EMI_NO_STR_DATA (-100000)   // == HIPSTR_NO_STR_DATA
#define HS_EMI_NO_READ 0x7fffffff      // "no entering read without STR data": what the check word starts from

// steps of HS_EMI_WAVE reads a wavefront makes over a run
HS_EMI_HD constexpr inline int64_t hs_emi_run_steps(int64_t n_reads){ return (n_reads + HS_EMI_WAVE - 1)/HS_EMI_WAVE; }
// reads of the last step (0: the run is empty)
HS_EMI_HD constexpr inline int hs_emi_last_step(int64_t n_reads){ return n_reads <= 0 ? 0 : (int)(n_reads - (hs_emi_run_steps(n_reads) - 1)*HS_EMI_WAVE); }
// workgroups of a launch with a wavefront per run (select, scatter)
HS_EMI_HD constexpr inline int64_t hs_emi_run_workgroups(int64_t n_runs){ return (n_runs + HS_EMI_THREADS/64 - 1)/(HS_EMI_THREADS/64); }
// chunks of the scan over n_runs run counts, and the runs of chunk c
HS_EMI_HD constexpr inline int64_t hs_emi_scan_chunks(int64_t n_runs){ return (n_runs + HS_EMI_SCAN_CHUNK - 1)/HS_EMI_SCAN_CHUNK; }
HS_EMI_HD constexpr inline int hs_emi_scan_chunk_len(int64_t n_runs, int64_t c){
  return (int)(n_runs - c*HS_EMI_SCAN_CHUNK < HS_EMI_SCAN_CHUNK ? n_runs - c*HS_EMI_SCAN_CHUNK : HS_EMI_SCAN_CHUNK);
}
// the locus' sizes (ref_allele included) lie in [lo, hi]: does the presence bitmap hold them — the device prepares the locus — or does the
// whole call take the host's preparation (a span of the table's length or more: em_prepare's pairwise test of the effective differences)
HS_EMI_HD constexpr inline bool hs_emi_bitmap_fits(int64_t lo, int64_t hi){ return hi - lo < HS_EMI_SPAN_LIMIT; }
HS_EMI_HD constexpr inline int hs_emi_bitmap_words(int64_t lo, int64_t hi){ return (int)((hi - lo)/32 + 1); }
// does a locus of n_sizes alleles still evaluate its initial allele frequencies on the device (beyond: "too many distinct allele sizes", decided on the host)
HS_EMI_HD constexpr inline bool hs_emi_sizes_fit(int64_t n_sizes){ return n_sizes + 1 < HS_EMI_SPAN_LIMIT; }
// where a locus' allele sizes and log frequencies start: it can have one allele per entering read and ref_allele, so the entering reads in
// front of it plus one slot per locus in front of it always suffice (no scan over the allele counts)
HS_EMI_HD constexpr inline int64_t hs_emi_bps_off(int64_t em_read_off_l, int64_t l){ return em_read_off_l + l; }

// One (locus, sample) run is a unit of the posterior run (post_layout.h: hs_post_unit_t — read_begin, n_reads, samp_index): they lie on the
// device since hipstr_post_upload.  Per locus:
struct hs_emi_locus_t {
  int32_t unit_first, n_units;     // the locus' runs (its samples, in order)
  int32_t samp_begin;              // global slot of the locus' first sample
  int32_t blk_start, blk_end;      // of block 1
  int32_t pad;
};

struct hs_post_unit_t;
struct hs_emi_dev_t {
  const hs_post_unit_t* units;     // the posterior run's
  const hs_emi_locus_t* loci;
  const int32_t* unit_locus;       // [n_units]
  int32_t  n_units, n_loci, ref_allele, n_reads;
  const double*  log_p1;           // the posterior run's, [n_reads]
  const double*  log_p2;
  const int32_t* seed;             // [n_reads]
  const int32_t* read_req;         // [n_reads]
  const int32_t* stutter_size, *aln_start, *aln_stop, *str_seq_off;      // the resident result's, [n_req] / [n_req+1]
  // scratch, written by hs_emi_select_kernel for every read of every run
  int32_t* read_bps;               // [n_reads] num_bps of an entering read
  uint8_t* read_in;                // [n_reads] 1 = the read enters
  int32_t* run_base;               // [n_units+1] hs_emi_scan_kernel: compact position of the run's first entering read
  // what comes home, one block: (hs_emi_select_kernel) run_count, lo / hi, check; (hs_emi_scan_kernel) em_read_off; (hs_emi_alleles_kernel) n_sizes
  int32_t* run_count;              // [n_units] entering reads of the run
  int32_t* lo, *hi;                // [n_loci] smallest / largest size, ref_allele included (they start from ref_allele: hs_emi_init_kernel)
  int32_t* check;                  // [1] lowest entering read whose request has no STR data (starts from HS_EMI_NO_READ)
  int32_t* em_read_off;            // [n_loci+1]
  int32_t* n_sizes;                // [n_loci] alleles of the locus, or -1: not prepared here (hs_emi_bitmap_fits)
  // the EM's seven per-read and per-allele arrays
  int32_t* num_bps;                // [n_reads capacity] compact
  int32_t* sample_label, *weight, *obs;
  double*  c_log_p1, *c_log_p2;
  int32_t* bps;                    // [n_reads + n_loci capacity] a locus' sizes at hs_emi_bps_off
  double*  gtp;                    // same offsets
};
