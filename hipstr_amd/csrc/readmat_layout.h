// readmat_layout.h — device-side description of the resident read x haplotype matrix (readmat.hip, api.hip: hipstr_rm_*).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HS_RM_HD __host__ __device__
#else
#define HS_RM_HD
#endif

// ---- launch decisions of the matrix kernels: the one place each is taken.  readmat.hip and hipstr_rm_scatter / hipstr_rm_remap (api.hip) call
// them, hipstr_debug_rm_plan reports them.
#define HS_RM_THREADS 256              // threads of a workgroup (four wavefronts, each with a work item list entry of its own)
#define HS_RM_NARROW_MAX 32            // a locus of up to this many haplotypes packs several work items into a wavefront
#define HS_RM_UNALIGNED (-100000.0)    // what the reference gives columns it has not aligned yet (seq_stutter_genotyper.cpp:374)
#define HS_RM_PAIR 0x80000000u         // bit of a mate group's word: the group is (first mate, second mate) = rows (i, i + 1)
// Lanes run along the haplotype columns of a work item — a mate group of the scatter, a row of the remap.  Narrow route (A <= HS_RM_NARROW_MAX):
// an item takes the power of two of lanes that holds its A columns, a wavefront 64 / lanes items.  Wide route: an item has the wavefront and
// steps over its columns 64 at a time.
HS_RM_HD inline int hs_rm_item_lanes(int A){
  if (A > HS_RM_NARROW_MAX) return 64;
  int w = 1; while (w < A) w <<= 1;
  return w;
}
HS_RM_HD inline int hs_rm_items_per_wave(int A){ return 64 / hs_rm_item_lanes(A); }
HS_RM_HD inline int hs_rm_column_steps(int A){ const int w = hs_rm_item_lanes(A); return (A + w - 1) / w; }
inline int64_t hs_rm_waves(int A, int64_t n_items){ const int per = hs_rm_items_per_wave(A); return (n_items + per - 1) / per; }

// One wavefront's share: items [first, first + 64 / lanes) of a locus (clipped to the locus' count by the kernel).
struct hs_rm_wave_t { int32_t locus, first; };

// One locus of a scatter.
struct hs_rm_locus_t {
  int64_t mat_off;         // the locus' [R x A] block in the matrix
  int64_t src_off;         // the locus' [P x A] block in the pooled batch's aln_probs (hs_locus_t::out_off)
  int32_t n_alleles;
  int32_t lanes_log2;      // log2 of hs_rm_item_lanes(A)
  int32_t read_begin;      // first un-pooled read of the locus
  int32_t pool_begin;      // first pooled read of the locus in the pooled batch
  int32_t group_begin, n_groups;      // the locus' mate groups in groups[]
  int32_t mask_off;        // the locus' realign_hap flags in mask[], or -1: every haplotype was realigned (no flag is read)
  int32_t pad;
};

// pooled reads' seeds come from the batch's own read records (layout.h hs_read_t: 16 bytes, seed third)
struct hs_rm_scatter_t {
  const hs_rm_wave_t*  waves;
  const hs_rm_locus_t* loci;
  const uint32_t* groups;        // per mate group: first row (global un-pooled read index) | HS_RM_PAIR
  const int32_t*  pool_index;    // [n_reads]
  const uint8_t*  copy_read;     // [n_reads] or NULL = all
  const uint8_t*  mask;
  const double*   src;           // hs_dev_t::aln_probs of the pooled batch
  const int32_t*  pool_reads;    // hs_dev_t::reads of the pooled batch, as dwords
  double*  ll;
  int32_t* seeds;
  int64_t  n_waves;
};

// One locus of a column remap.
struct hs_rm_remap_locus_t {
  int64_t old_off, new_off;
  int32_t old_A, new_A;
  int32_t lanes_log2;      // of the NEW allele count
  int32_t n_reads;
  int32_t inv_off;         // the locus' inverse mapping in inv[]: old column of every new column, or -1
  int32_t pad;
};
struct hs_rm_remap_t {
  const hs_rm_wave_t* waves;
  const hs_rm_remap_locus_t* loci;
  const int32_t* inv;
  const double*  old_ll;
  double*  new_ll;
  int64_t  n_waves;
};
