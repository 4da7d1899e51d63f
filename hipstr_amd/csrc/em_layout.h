// em_layout.h — launch decisions of the stutter EM (em.hip): the one place each is taken.  The kernels and hipstr_em_train call them,
// hipstr_debug_em_plan reports them (tests/test_em_routes.py pins a case on each side of every limit).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define HS_EM_THREADS 256          // threads of a per-locus workgroup
#define HS_EM_PARTS 8              // workgroups per locus in the two big M-step reductions
#define HS_EM_TILE 2048            // rows of a slice whose live rows are listed at a time (hs_em_mstep_part)
#define HS_EM_CHUNK 32             // positions of the allele-frequency scans per round of prepared exponentials (em_gt_priors)
#define HS_EM_MAXA_LDS 64          // alleles whose chains run side by side (lanes of the first wavefront); more alleles: several sweeps
#define HS_EM_GMAX_WAVE_MAXA 64    // hs_em_gmax: up to this many alleles a wavefront takes a sample (lanes = the second allele)
#define HS_EM_GMAX_WAVES (HS_EM_THREADS/64)   // ... and the samples are dealt to this many wavefronts
#define HS_EM_INIT_THREADS 256     // loci per workgroup of hs_em_init
#define HS_EM_COMPACT_THREADS 1024 // loci per chunk of hs_em_compact's scan (one workgroup; the bases are carried from chunk to chunk)
#define HS_EM_UNITS_THREADS 256    // samples hs_em_units writes per pass over a locus
#define HS_EM_PRUNE_C 4.0e-6       // what a row's phase term may exceed 0 by: rows are pruned by gmax + this (hs_em_mstep_part)
#define HS_EM_TERM_FLOOR (-37.43)  // a term below 2^-54 of a total >= 1 leaves it as it is and is not formed (em_gt_priors)
#if defined(__HIPCC__) || defined(__CUDACC__)
#define HS_EM_HD __host__ __device__
#else
#define HS_EM_HD
#endif
// hs_em_gmax: a wavefront per sample (lanes = the second allele), or a thread per (sample, allele)
HS_EM_HD constexpr bool hs_em_gmax_wave(int A){ return A <= HS_EM_GMAX_WAVE_MAXA; }
// em_gt_priors' two LDS buffers of a chunk (exponentials, values); the row tiles live in the same bytes
HS_EM_HD constexpr int hs_em_lds_doubles(){ return 2*HS_EM_CHUNK*HS_EM_MAXA_LDS; }
// odd row stride of a row tile: the per-row walks of neighbouring threads fall into different banks
HS_EM_HD constexpr int hs_em_row_stride(int A){ return A | 1; }
// posterior rows (sample, allele_1) per LDS tile; 0: a row does not fit (thousands of alleles) and the rows are read straight from memory
HS_EM_HD constexpr int hs_em_row_tile_rows(int A){
  return HS_EM_THREADS < hs_em_lds_doubles()/hs_em_row_stride(A) ? HS_EM_THREADS : hs_em_lds_doubles()/hs_em_row_stride(A);
}
// alleles of the sweep that starts at allele a0, and the sweeps of a locus
HS_EM_HD constexpr int hs_em_sweep_alleles(int A, int a0){ return HS_EM_MAXA_LDS < A - a0 ? HS_EM_MAXA_LDS : A - a0; }
HS_EM_HD constexpr int hs_em_sweeps(int A){ return (A + HS_EM_MAXA_LDS - 1)/HS_EM_MAXA_LDS; }
// the chain of an allele: a row log-sum-exp per sample, then a posterior per (sample, allele_1); positions of the chunk at c0
HS_EM_HD constexpr int64_t hs_em_chain_len(int S, int A){ return (int64_t)S + (int64_t)S*A; }
HS_EM_HD constexpr int hs_em_chunk_len(int64_t ntot, int64_t c0){ return (int)((int64_t)HS_EM_CHUNK < ntot - c0 ? (int64_t)HS_EM_CHUNK : ntot - c0); }
// first (read, source allele) row of slice k of a locus' R*A rows (slice k ends where slice k + 1 begins)
HS_EM_HD constexpr int hs_em_slice_begin(int total, int k){ return (int)((int64_t)total*k/HS_EM_PARTS); }
// the device-resident loop
HS_EM_HD constexpr unsigned hs_em_init_blocks(int n_loci){ return (unsigned)((n_loci + HS_EM_INIT_THREADS - 1)/HS_EM_INIT_THREADS); }
HS_EM_HD constexpr int hs_em_compact_chunks(int n_loci){ return (n_loci + HS_EM_COMPACT_THREADS - 1)/HS_EM_COMPACT_THREADS; }
// last value of the host's round counter: round r is queued while the count of round r - 1 travels, so the stop signal of the last
// round allowed (max_iter) arrives one round later
HS_EM_HD constexpr int hs_em_last_round(int max_iter){ return max_iter + 1; }
