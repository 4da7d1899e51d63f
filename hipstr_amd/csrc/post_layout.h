// post_layout.h — device-side description of a posterior batch (post_kernels.hip, api.hip).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

// ---- launch decisions of the posterior stage: the one place each is taken.  post_kernels.hip and hipstr_post_launch (api.hip) call them,
// hipstr_debug_post_plan reports them (tests/test_stage_routes.py pins a case on each side of every limit)
#define HS_POST_THREADS 256            // threads of a posterior workgroup
#define HS_POST_ECHUNK 2048            // exponentials summed per LDS chunk; the register path's read tiles live in the same buffer
#define HS_POST_REGS 8                 // diplotypes per thread a unit may have to stay in registers (256 x 8 = HS_POST_ECHUNK: its exponentials fit the LDS chunk)
#define HS_POST_SPLIT_WGS 2048         // workgroups a split accumulation aims at
#define HS_POST_SPLIT_MAX_UNITS 1024   // from this many units on the accumulation is never split
#if defined(__HIPCC__) || defined(__CUDACC__)
#define HS_POST_HD __host__ __device__
#else
#define HS_POST_HD
#endif
// a unit of nd = A^2 diplotypes keeps them in registers (one launch only: a split launch takes the chunked path for every unit)
HS_POST_HD inline bool hs_post_in_registers(int nd){ return nd <= HS_POST_THREADS*HS_POST_REGS; }
// reads per LDS tile of the register path: two addends per (read, allele) + a weight per read
HS_POST_HD inline int hs_post_reads_per_tile(int A, int n_reads){
  const int fit = HS_POST_ECHUNK / (2*A + 1), rt = n_reads < fit ? n_reads : fit;
  return rt > 1 ? rt : 1;
}
// workgroups per unit of the accumulation (1 = hs_posterior_kernel alone): from the LARGEST unit, applied to every unit of the launch
inline int hs_post_split(int max_nd, size_t n_units){
  const size_t by_size = (size_t)(max_nd + HS_POST_THREADS - 1)/HS_POST_THREADS;
  const size_t by_count = n_units < HS_POST_SPLIT_MAX_UNITS ? (HS_POST_SPLIT_WGS + n_units - 1)/n_units : 1;
  return (int)(by_size < by_count ? by_size : by_count);
}

// One (locus, sample) pair: the unit a workgroup processes.
struct hs_post_unit_t {
  int64_t post_off;        // offset of this sample's [A x A] block in log_post
  int64_t prior_off;       // offset of this sample's [A x A] block in log_prior (the EM shares one block per locus)
  int64_t ll_off;          // offset in log_aln_probs of the row of this sample's FIRST read
  int32_t n_alleles;
  int32_t read_begin;      // global read index of the sample's first read (reads of a sample are contiguous)
  int32_t n_reads;
  int32_t samp_index;      // global sample slot
  double  log_hom_prior;   // Genotyper::log_homozygous_prior   (genotyper.cpp:20-25)
  double  log_het_prior;   // Genotyper::log_heterozygous_prior (genotyper.cpp:27-32)
};

struct hs_post_dev_t {
  const hs_post_unit_t* units;
  const double*  log_aln_probs;
  const double*  log_p1;
  const double*  log_p2;
  const int32_t* read_weight;
  const double*  log_prior;      // optional prior array (NULL = hom/het defaults of the unit)
  const int32_t* unit_active;    // optional per-unit flag: 0 = skip (loci whose EM has converged); NULL = all
  double*        log_post;
  double*        sample_total;
  int32_t*       map_gt;
  double         log_thresh, log_half;
  int32_t        raw;            // HIPSTR_DEBUG_HOST_LIBM: leave the accumulated log P(reads, diplotype) unnormalised — the host takes the log-sum-exp with its libm
  // optional indirection (the device-resident EM loop, em.hip): workgroup b takes unit unit_list[b] if b < *n_list and leaves otherwise —
  // the launch is sized by a bound the host knows, the live units by a count only the device knows.  NULL = workgroup b takes unit b.
  const int32_t* unit_list;
  const int32_t* n_list;
  int32_t        sym_prior;      // the prior array is symmetric in the two alleles (the EM's: log f(a1) + log f(a2)): see the symmetric accumulation in post_kernels.hip
};

// One (locus, sample) pair of the genotype extraction (Genotyper::extract_genotypes_and_likelihoods, genotyper.cpp:129-251).
struct hs_gt_unit_t {
  int64_t post_off;        // this sample's [A x A] posteriors
  int64_t tot_off;         // scratch: this sample's [V x V] total_log_phased_posteriors
  int64_t gl_off, pgl_off; // this sample's pieces of the GL/PL and PHASEDGL outputs
  int32_t n_alleles, n_variants;
  int32_t samp_index;
  int32_t haploid;
  int32_t map_off;         // into h2a / gmem (per locus: A entries)
  int32_t goff_off;        // into goff (per locus: V+1 entries, relative to map_off)
  double  hom_corr, het_corr;     // priors to take out again (genotyper.cpp:197-198)
  double  gl_ncfg, pgl_ncfg;      // corrections for the number of averaged haplotype configurations (:201-209)
};

struct hs_gt_dev_t {
  const hs_gt_unit_t* units;
  const double*  log_post;
  const double*  sample_total;
  const int32_t* map_gt;          // MAP haplotype pair per sample (hs_posterior_kernel)
  const int32_t* h2a;             // hap_to_allele
  const int32_t* gmem;            // haplotypes of a locus sorted by (variant, haplotype index)
  const int32_t* goff;            // start of every variant's haplotypes in gmem
  double*  tot;                   // scratch
  int32_t* best_gt;               // [2*n_samp]
  double*  log_phased, *log_unphased, *hap_log_phased, *hap_log_unphased, *gl_diff;   // [n_samp]
  double*  gls;  int32_t* pls;  double* pgls;
  int32_t  calc_any, calc_gls, calc_pls, calc_pgls;
  double   log_thresh;
  int32_t  tot_given;            // HIPSTR_DEBUG_HOST_LIBM: `tot` (and log_unphased) come from the host
};

// hipstr_post_extract_vcf: the genotype kernel's GL / PL / PHASEDGL pieces gathered into the sorted allele order of the record
// (seq_stutter_genotyper.cpp:1436-1481), best_gt renumbered in place, and the per-variant BPDIFFS / AC gathers
struct hs_gt_perm_dev_t {
  const hs_gt_unit_t* units;      // the genotype kernel's
  const int32_t* unit_var;        // [n_units] where the unit's locus begins in the per-variant arrays
  const int32_t *new_to_old, *old_to_new;      // [sum V], per locus
  const int32_t* n2o_abs;         // [sum V] new_to_old plus the locus' begin
  const double* gls; const int32_t* pls; const double* pgls;      // block-option order
  double* gls_out; int32_t* pls_out; double* pgls_out;            // VCF order; NULL = not asked for
  int32_t* best_gt;               // [2*n_samp]
  const int32_t *bp_in, *ac_in;   // [sum V] or NULL
  int32_t *bp_out, *ac_out;
  int32_t n_var;
};
// row i of the lower triangle that holds entry k (k = i(i+1)/2 + j, j <= i): the square root is within one of it
HS_POST_HD inline int hs_gt_tri_row(int64_t k){
  int i = (int)((sqrt(8.0*(double)k + 1.0) - 1.0)*0.5);
  if ((int64_t)(i + 1)*(i + 2)/2 <= k) i++;
  if ((int64_t)i*(i + 1)/2 > k) i--;
  return i;
}

// ---- read assignment (assign.hip, hipstr_post_assign): SeqStutterGenotyper::write_vcf_record's per-read loop (seq_stutter_genotyper.cpp:1079-1157)
// and retrace_alignments' pick (:805-841) on the resident MAP pairs.  The unit is hs_post_unit_t again; lanes are reads.
#define HS_ASSIGN_THREADS 256          // threads of an assignment workgroup (four wavefronts)
#define HS_ASSIGN_WAVE_READS 256       // a launch whose largest unit has at most this many reads gives every unit ONE wavefront, four units per workgroup
#define HS_ASSIGN_DIRECT_MAX 4096      // a locus of up to this many (pool, haplotype) keys gets a direct first-occurrence table, a larger one a hashed table
#define HS_ASSIGN_EMPTY 0x7f7f7f7f     // what a byte-wise fill with 0x7f leaves in the tables: above every read index and every key
// wavefronts per unit of an assignment launch (1: four units share a workgroup, each loops over its reads 64 at a time; 4: a unit has the
// workgroup and loops 256 at a time): from the LARGEST unit, applied to every unit of the launch, as hs_post_split is
HS_POST_HD inline int hs_assign_waves_per_unit(int max_unit_reads){ return max_unit_reads <= HS_ASSIGN_WAVE_READS ? 1 : HS_ASSIGN_THREADS/64; }
// workgroups of that launch
HS_POST_HD inline int64_t hs_assign_workgroups(int64_t n_units, int waves_per_unit){
  const int per_wg = HS_ASSIGN_THREADS/64/waves_per_unit;
  return (n_units + per_wg - 1)/per_wg;
}
// slots of a locus' first-occurrence table: n_keys = pools x haplotypes entries addressed by the key itself, or — hashed — the power of two
// from twice the locus' reads (a read adds at most one key: the table stays at most half full); *hashed says which
HS_POST_HD inline int64_t hs_assign_table_slots(int64_t n_keys, int64_t n_reads, int* hashed){
  if (n_keys <= HS_ASSIGN_DIRECT_MAX){ *hashed = 0; return n_keys; }
  int64_t h = 64; while (h < 2*n_reads) h <<= 1;
  *hashed = 1; return h;
}

// One locus of the request compaction.  Table of the locus at tab + tab_off: direct [first read: slots][request: slots],
// hashed [key: slots][first read: slots][request: slots].
struct hs_assign_locus_t {
  int64_t tab_off;
  int32_t slots, hashed;
  int32_t read_begin, n_reads;     // un-pooled reads of the locus
  int32_t n_alleles, pool_off;     // pool_off: hipstr_batch_t::read_off of the pooled batch (request = pool_off + pool index)
};

struct hs_assign_dev_t {
  const hs_post_unit_t* units;     // the posterior run's
  const double*  log_aln_probs;
  const double*  log_p1;
  const double*  log_p2;
  const int32_t* map_gt;           // MAP haplotype pair per sample (hs_posterior_kernel)
  const int32_t* unit_locus;       // [n_units] locus << 1 | haploid
  const hs_assign_locus_t* loci;
  const int32_t* seed;             // [n_reads]
  const uint8_t* reverse;          // [n_reads] or NULL
  const int32_t* pool_index;       // [n_reads] or NULL = no request list
  int32_t  n_units, n_loci, rule, cap_req;
  double   log_half, strand_tolerance;
  // per read
  int32_t* best_hap, *read_strand, *read_req;
  double*  log_phase_one;
  // per sample: n_aligned, n_snp, n_strand_one, n_strand_two, uniq_one, uniq_two, rv_uniq_one, rv_uniq_two back to back, [8][n_samp]
  int32_t* counters;  int32_t n_samp;
  double*  phase1, *phase2;
  // request compaction
  int32_t* tab;
  int32_t* locus_count;            // [n_loci] distinct keys per locus (zeroed before the launch)
  int32_t* locus_base;             // [n_loci] requests in front of the locus
  int32_t* n_req, *req_read, *req_allele;
};

// ---- read counts from a resident traceback result (assign.hip: hs_trace_stats_kernel; hipstr_assign_trace_stats_dev): the counts of
// seq_stutter_genotyper.cpp:1124-1127 and the ml_bp of :1150-1154.  The unit is a run of consecutive reads of one (locus, sample) pair — the
// pair's reads when the labels ascend, as they do in a posterior batch — one wavefront each, four per workgroup, lanes are reads 64 at a
// time; a sample's counts are integer sums over its runs (zeroed before the launch).  One launch route.
#define HS_TSTAT_NO_STR_DATA (-100000)     // == HIPSTR_NO_STR_DATA
#define HS_TSTAT_NO_ML_BP INT32_MIN        // == HIPSTR_NO_ML_BP
struct hs_tstat_unit_t { int32_t read_begin, n_reads, samp, locus; };       // samp: global sample slot
struct hs_tstat_locus_t {
  int64_t hap_begin, var_begin;            // the locus' entries of hap_to_allele / allele_bp_diff
  int32_t start_bound, stop_bound;         // spans iff aln_start < start_bound && aln_stop > stop_bound (region_start > 4 ? region_start - 4 : 0; region_stop + 4)
};
struct hs_tstat_dev_t {
  const hs_tstat_unit_t*  units;
  const hs_tstat_locus_t* loci;
  int32_t n_units;
  const int32_t* read_req, *best_hap;      // [n_reads]
  const int32_t* hap_to_allele, *allele_bp_diff;
  const int32_t* stutter_size, *flank_ins, *flank_del, *aln_start, *aln_stop;     // the resident result's, [n_req]
  int32_t* n_stutter, *n_flank_indel;      // [n_samp], zeroed before the launch
  int32_t* ml_bp;                          // [n_reads]
};
