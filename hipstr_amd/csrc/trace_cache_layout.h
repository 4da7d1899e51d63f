// trace_cache_layout.h — device-side description of the ragged gather of resident traceback records and of the trace cache built on it
// (trace_cache.hip: hipstr_trace_dev_gather, hipstr_trace_cache_*): SeqStutterGenotyper::retrace_alignments' trace_cache_
// (seq_stutter_genotyper.cpp:805-841, re-keyed at :401-409) for a batch of loci.  Every size decision of the stage is taken here;
// trace_cache.hip's kernels and its host side call these functions, tests/test_trace_cache_host.py pins them through
// hipstr_debug_trace_cache_plan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HS_TC_HD __host__ __device__
#else
#define HS_TC_HD
#endif

#define HS_TC_POOLS 7                  // == HS_TRACE_DEV_POOLS: hap_aln, str_seq, flank_seq, indel, snp, cigar, aln_str
#define HS_TC_ARRAYS 10                // == HS_TRACE_DEV_ARRAYS
#define HS_TC_FLANK_POOL 2             // the pool with two pieces per record (left flank, right flank)
#define HS_TC_PIECES 8                 // pieces of a record over all pools
#define HS_TC_WAVE 64
#define HS_TC_LEN_THREADS 256          // threads of a workgroup of the lengths kernel (a thread per output record)
#define HS_TC_TOTALS_BYTES 64          // what comes home from a gather: the seven pool totals as int64, one pad word

// pieces of pool p in a handle of n records, and where pool p's pieces start in the [HS_TC_PIECES*n] scratch arrays (lens, from, incl)
HS_TC_HD constexpr inline int64_t hs_tc_pool_pieces(int p, int64_t n){ return p == HS_TC_FLANK_POOL ? 2*n : n; }
HS_TC_HD constexpr inline int64_t hs_tc_pool_at(int p, int64_t n){ return (p <= HS_TC_FLANK_POOL ? p : p + 1)*n; }
// workgroups of the lengths kernel; steps of HS_TC_WAVE pieces the scan's wavefront makes over a pool (its carry crosses each boundary)
HS_TC_HD constexpr inline int64_t hs_tc_len_workgroups(int64_t n_out){ return (n_out + HS_TC_LEN_THREADS - 1)/HS_TC_LEN_THREADS; }
HS_TC_HD constexpr inline int64_t hs_tc_scan_steps(int p, int64_t n_out){ return (hs_tc_pool_pieces(p, n_out) + HS_TC_WAVE - 1)/HS_TC_WAVE; }
// workgroups of the copy kernel: a wavefront per output record; one for the empty gather, which still writes the seven leading zeros
HS_TC_HD constexpr inline int64_t hs_tc_copy_workgroups(int64_t n_out){ return n_out > 0 ? n_out : 1; }
// does a pool of this many elements still fit the 32-bit offsets.  The scan sums a step's 64 lengths modulo 2^32 and carries the steps'
// sums in 64 bits; a step whose sum passes 2^32 reports HS_TC_TOTAL_WRAPPED in place of a total, which does not fit either.
HS_TC_HD constexpr inline bool hs_tc_pool_fits(int64_t total){ return total >= 0 && total <= 0x7fffffff; }
#define HS_TC_TOTAL_WRAPPED INT64_MAX

// ---- when hipstr_trace_cache_round compacts by itself.  Dead records (no key names them any more: their haplotype was removed, or their
// locus did not take them) cost device memory only; segments cost a row of the gather's source table and a cache block each.  A cache is
// compacted when more than half of at least HS_TC_COMPACT_MIN_DEAD records are dead, or when it holds more than HS_TC_MAX_SEGMENTS
// segments.  genotype() makes three to five rounds per pass, so a pass normally ends without one.
#define HS_TC_COMPACT_MIN_DEAD 4096
#define HS_TC_MAX_SEGMENTS 16
HS_TC_HD constexpr inline bool hs_tc_should_compact(int64_t n_live, int64_t n_dead, int64_t n_segments){
  return n_segments > HS_TC_MAX_SEGMENTS || (n_dead >= HS_TC_COMPACT_MIN_DEAD && n_dead > n_live);
}

// One source of a gather as the kernels see it: the arrays of its handle (api_internal.h: hipstr_trace_dev).
struct hs_tc_src_t {
  const double*  ll;
  const int32_t* max_index;
  const int32_t* scal[5];
  const int32_t* off[HS_TC_POOLS];
  const char*    arr[HS_TC_ARRAYS];
  int32_t n_req, pad;
};

struct hs_tc_dev_t {
  const hs_tc_src_t* src;              // [n_src]
  const int32_t* out_src;              // [n_out]
  const int32_t* out_idx;              // [n_out]
  int32_t* lens;                       // [HS_TC_PIECES*n_out] scratch: a piece's elements (pool p at hs_tc_pool_at)
  int32_t* from;                       // same: its first element in the source's pool
  int32_t* incl;                       // same: the running total behind it == the result's off[p][piece + 1]
  int64_t* totals;                     // [HS_TC_POOLS] + pad: what comes home
  int32_t  n_out, n_src;
};

// the result, where the copy kernel writes (its handle's arrays)
struct hs_tc_out_t {
  double*  ll;
  int32_t* max_index;
  int32_t* scal[5];
  int32_t* off[HS_TC_POOLS];
  char*    arr[HS_TC_ARRAYS];
  int64_t  totals[HS_TC_POOLS];
};
