// readmat.hip — upkeep of the resident read x haplotype matrix (log_aln_probs_, R x A per locus) on gfx950.
//
// hs_rm_scatter_kernel: the second half of SeqStutterGenotyper::calc_hap_aln_probs (seq_stutter_genotyper.cpp:530-564) — the rows of the
// pooled forward pass copied to the pools' reads, the two mates of a pair summed, earlier rounds' values kept where nothing was realigned.
// hs_rm_remap_kernel: the column re-layout of add_and_remove_alleles (:371-386).
//
// Both are bandwidth-bound.  Lanes run along the haplotype columns, so a wavefront's loads and stores of a row are consecutive addresses; a
// locus with few haplotypes (the usual one has 4-32) packs 64 / lanes work items into a wavefront (readmat_layout.h), whose rows follow each
// other in memory.  The scatter's work item is a MATE GROUP — a read alone, or a first mate with its second mate — and one lane of one item
// writes column j of BOTH rows of a pair: the reference's second loop reads row i - 1 as the first loop left it, and no other item ever
// touches that row, so there is nothing to order between work items (no second pass, no atomics).  The only arithmetic is the mates' one
// IEEE double addition (the library is built with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "readmat_layout.h"

extern "C" __global__ void __launch_bounds__(HS_RM_THREADS) hs_rm_scatter_kernel(const hs_rm_scatter_t d){
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x*(HS_RM_THREADS/64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= d.n_waves) return;
  const hs_rm_wave_t wv = d.waves[w];
  const hs_rm_locus_t L = d.loci[wv.locus];
  const int A = L.n_alleles, W = 1 << L.lanes_log2;
  const int sub = lane & (W - 1), gi = wv.first + (lane >> L.lanes_log2);
  if (gi >= L.n_groups) return;
  const uint32_t g = d.groups[L.group_begin + gi];
  const bool pair = (g & HS_RM_PAIR) != 0;
  const int i0 = (int)(g & ~HS_RM_PAIR), i1 = i0 + 1;                 // rows of the group (i1: the second mate)
  const bool c0 = d.copy_read ? d.copy_read[i0] != 0 : true;          // :533
  const bool c1 = pair && (d.copy_read ? d.copy_read[i1] != 0 : true);
  if (!c0 && !c1) return;                                             // neither loop touches the group
  int p0 = 0, p1 = 0, s0 = 0, s1 = 0;
  if (c0){ p0 = d.pool_index[i0]; s0 = d.pool_reads[4*(int64_t)(L.pool_begin + p0) + 2]; }
  if (c1){ p1 = d.pool_index[i1]; s1 = d.pool_reads[4*(int64_t)(L.pool_begin + p1) + 2]; }
  if (sub == 0){                                                      // :538
    if (c0) d.seeds[i0] = s0;
    if (c1) d.seeds[i1] = s1;
  }
  double* row0 = d.ll + L.mat_off + (int64_t)(i0 - L.read_begin)*A;
  double* row1 = row0 + A;
  // a pool without a seed: its row of zeros (HapAligner.cpp:333-337), whatever the batch's buffer holds there
  const double* src0 = d.src + L.src_off + (int64_t)p0*A;
  const double* src1 = d.src + L.src_off + (int64_t)p1*A;
  const uint8_t* mask = L.mask_off >= 0 ? d.mask + L.mask_off : NULL;
  for (int j = sub; j < A; j += W){
    if (mask && !mask[j]) continue;                                   // :541, :558 — only where some haplotype was not realigned
    if (!pair){
      row0[j] = s0 < 0 ? 0.0 : src0[j];                               // :542
      continue;
    }
    const double a = c0 ? (s0 < 0 ? 0.0 : src0[j]) : row0[j];         // row i - 1 as the first loop leaves it (:555)
    if (c1){
      const double total = a + (s1 < 0 ? 0.0 : src1[j]);              // :559
      row0[j] = total; row1[j] = total;                               // :560-561
    } else row0[j] = a;                                               // the second mate is not copied: no sum (:552)
  }
}

extern "C" __global__ void __launch_bounds__(HS_RM_THREADS) hs_rm_remap_kernel(const hs_rm_remap_t d){
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x*(HS_RM_THREADS/64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= d.n_waves) return;
  const hs_rm_wave_t wv = d.waves[w];
  const hs_rm_remap_locus_t L = d.loci[wv.locus];
  const int W = 1 << L.lanes_log2;
  const int sub = lane & (W - 1), r = wv.first + (lane >> L.lanes_log2);
  if (r >= L.n_reads) return;
  const double* old_row = d.old_ll + L.old_off + (int64_t)r*L.old_A;
  double* new_row = d.new_ll + L.new_off + (int64_t)r*L.new_A;
  const int32_t* inv = d.inv + L.inv_off;
  for (int j = sub; j < L.new_A; j += W){                             // one lane per NEW column: the stores of a row are consecutive
    const int s = inv[j];
    new_row[j] = s >= 0 ? old_row[s] : HS_RM_UNALIGNED;               // :374, :381
  }
}

// n doubles set to v (a fresh matrix: -100000 everywhere)
extern "C" __global__ void __launch_bounds__(HS_RM_THREADS) hs_rm_fill_kernel(double* __restrict__ p, int64_t n, double v){
  const int64_t stride = (int64_t)gridDim.x*HS_RM_THREADS;
  for (int64_t i = (int64_t)blockIdx.x*HS_RM_THREADS + threadIdx.x; i < n; i += stride) p[i] = v;
}
