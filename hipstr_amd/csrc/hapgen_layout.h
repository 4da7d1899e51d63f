// hapgen_layout.h — device-side description of the haplotype generator (hapgen.hip: hipstr_hapgen; host twin: hapgen_host.cpp), and the
// few pieces of arithmetic both sides share word for word: the locus' status, trim's two amounts, the case fold.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pool_layout.h"      // the 64-bit hash: hs_pool_mix / hs_pool_hash_piece / hs_pool_hash_finish, HS_POOL_EMPTY_KEY, hs_pool_chunk_end

#define HS_HAPGEN_HD HS_POOL_HD

// ---- size decisions: the one place each is taken.  hapgen.hip's kernels and hipstr_hapgen call them, hipstr_debug_hapgen_plan reports them.
#define HS_HAPGEN_THREADS 256          // threads of a workgroup (four wavefronts)
#define HS_HAPGEN_LDS_READS 2048       // a locus of up to this many reads is grouped in LDS; a larger one is done by the host twin
#define HS_HAPGEN_MAX_SAMPLES 512      // samples of a locus whose per-sample counts the workgroup holds in LDS
#define HS_HAPGEN_MAX_DISTINCT 256     // distinct extracted strings (so at most this many + 1 options) of a locus the device finishes
#define HS_HAPGEN_HASH_STEP 16         // bytes a lane of the hash wavefront folds per step
#define HS_HAPGEN_MIN_SLOTS 64         // fewest slots of a locus' hash table
#define HS_HAPGEN_WS_MIB 256           // workspace budget of a chunk of whole loci (HIPSTR_HAPGEN_WS_MIB overrides it)
#define HS_HAPGEN_READ_FIXED 96        // bytes of per-read tables a read takes of the workspace, whatever its length
#define HS_HAPGEN_LOCUS_FIXED 160      // bytes of per-locus tables
#define HS_HAPGEN_MAX_LOCUS_BYTES 1073741824      // a locus whose reads take more goes to the host twin (device offsets are 32-bit)
#define HS_HAPGEN_LRES 16              // dwords of a locus' result record

#define HS_HAPGEN_LEFT_PAD 5           // HaplotypeGenerator.h:59-62
#define HS_HAPGEN_RIGHT_PAD 5
#define HS_HAPGEN_REF_FLANK 35
#define HS_HAPGEN_WIN_PAD 40           // the window starts this far in front of the region

// a locus' result record (dwords)
#define HS_HG_STATUS 0
#define HS_HG_REDO 1                   // 1 = hash collision, 2 = more distinct strings than HS_HAPGEN_MAX_DISTINCT: the host twin redoes the locus
#define HS_HG_B0S 2                    // start of block 0 (its end is the start of block 1)
#define HS_HG_B1S 3
#define HS_HG_B1E 4
#define HS_HG_B2E 5
#define HS_HG_NOPTS 6                  // options of block 1
#define HS_HG_SEQ 7                    // sequence bytes of the three blocks
#define HS_HG_SPAN 8
#define HS_HG_SAMP 9
#define HS_HG_DIST 10
#define HS_HG_LT 11
#define HS_HG_RT 12
#define HS_HG_MIN 13
#define HS_HG_MAX 14

HS_HAPGEN_HD inline char hs_hapgen_fold(char c){ return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }
HS_HAPGEN_HD inline int hs_hapgen_table_slots(int n_reads){
  int s = HS_HAPGEN_MIN_SLOTS; while (s < 2*n_reads) s <<= 1;
  return s;
}
// LDS of the grouping workgroup for a launch whose largest locus has n_reads reads and whose most-sampled locus n_samples samples: the
// table (keys 8 bytes a slot, leaders 4), two dwords per read (slot / distinct string; leader number / order by sample), two per sample
// (counted reads, fill cursor), per distinct string a double and nine dwords, and 64 dwords of scalars
HS_HAPGEN_HD inline size_t hs_hapgen_lds_bytes(int n_reads, int n_samples){
  return (size_t)hs_hapgen_table_slots(n_reads)*12 + (size_t)n_reads*8 + (size_t)n_samples*8 + (size_t)HS_HAPGEN_MAX_DISTINCT*8 +
         (size_t)(HS_HAPGEN_MAX_DISTINCT + 8)*36 + 256;
}
HS_HAPGEN_HD inline int hs_hapgen_on_device(int64_t n_reads, int64_t n_samples, int64_t bytes){
  return n_reads <= HS_HAPGEN_LDS_READS && n_samples <= HS_HAPGEN_MAX_SAMPLES && bytes <= HS_HAPGEN_MAX_LOCUS_BYTES;
}
// workspace a locus takes of a chunk: its reads' bases twice (the upload, the option bytes), its window twice, CIGAR runs, tables
HS_HAPGEN_HD inline int64_t hs_hapgen_locus_bytes(int64_t n_reads, int64_t bases, int64_t cigar_runs, int64_t window){
  return HS_HAPGEN_LOCUS_FIXED + n_reads*HS_HAPGEN_READ_FIXED + 2*bases + 5*cigar_runs + 2*window;
}
HS_HAPGEN_HD inline int hs_hapgen_hash_steps(int64_t len){ return (int)((len + 64*HS_HAPGEN_HASH_STEP - 1) / (64*HS_HAPGEN_HASH_STEP)); }

// 0 / 1 / 2 of a locus (HaplotypeGenerator.cpp:292, :305) from its region and the bounds of its flagged reads; 64-bit arithmetic, so a
// locus without flagged reads (INT32_MAX / INT32_MIN) is a plain 2
HS_HAPGEN_HD inline int hs_hapgen_status(int64_t region_start, int64_t region_stop, int64_t chrom_len, int64_t min_flagged_start, int64_t max_flagged_stop){
  if (region_start < HS_HAPGEN_REF_FLANK + HS_HAPGEN_LEFT_PAD || region_stop + HS_HAPGEN_REF_FLANK + HS_HAPGEN_RIGHT_PAD > chrom_len) return 1;
  if (min_flagged_start + 5 >= region_start - HS_HAPGEN_LEFT_PAD || max_flagged_stop - 5 <= region_stop + HS_HAPGEN_RIGHT_PAD) return 2;
  return 0;
}
// trim (HaplotypeGenerator.cpp:12-80) from what it needs of the sequences: the shortest length, and the common prefix / suffix of all of
// them counted up to min(5, min_len - ideal) — beyond that :20, :31 and :45-46 cut it off anyway
HS_HAPGEN_HD inline void hs_hapgen_trim(int min_len, int ideal, int common_prefix, int common_suffix, int* left_trim, int* right_trim){
  int lt = 0, rt = 0;
  if (min_len > ideal){                                                                                  // :16
    int ml = common_prefix < min_len - ideal ? common_prefix : min_len - ideal;                         // :20-42
    int mr = common_suffix < min_len - ideal ? common_suffix : min_len - ideal;
    if (ml > HS_HAPGEN_LEFT_PAD) ml = HS_HAPGEN_LEFT_PAD;                                                // :45-46
    if (mr > HS_HAPGEN_RIGHT_PAD) mr = HS_HAPGEN_RIGHT_PAD;
    if (ml > min_len - HS_HAPGEN_RIGHT_PAD) ml = min_len - HS_HAPGEN_RIGHT_PAD;                          // :49-50
    if (ml < 0) ml = 0;
    if (mr > min_len - HS_HAPGEN_LEFT_PAD) mr = min_len - HS_HAPGEN_LEFT_PAD;
    if (mr < 0) mr = 0;
    const int lo = ml < mr ? ml : mr;
    if (min_len - 2*lo <= ideal){                                                                        // :55-63
      lt = rt = lo;
      for (int step = 0; step < HS_HAPGEN_LEFT_PAD + HS_HAPGEN_RIGHT_PAD && min_len - lt - rt < ideal; step++){
        if (lt > rt) lt--; else rt--;
      }
    }
    else if (ml > mr){ rt = mr; lt = ml < min_len - ideal - mr ? ml : min_len - ideal - mr; }            // :64-73
    else { lt = ml; rt = mr < min_len - ideal - ml ? mr : min_len - ideal - ml; }
  }
  *left_trim = lt; *right_trim = rt;
}

// What the kernels take (by value).  Read indices and byte offsets are chunk-local; every array is a piece of the chunk's one device block.
struct hs_hapgen_dev_t {
  // uploaded, per read
  const int32_t* start;        // [n]
  const int32_t* stop;         // [n] the stop every comparison uses
  const int32_t* boff;         // [n] where the read's bases start
  const int32_t* coff;         // [n+1] its CIGAR runs
  const int32_t* sample;       // [n]
  const int32_t* rlocus;       // [n] its locus within the chunk
  const uint8_t* use;          // [n]
  const int32_t* clen;         // [runs]
  const char*    cop;          // [runs]
  const char*    bases;
  // uploaded, per locus
  const int32_t* lread_off;    // [nl+1] reads of a locus (a locus the host does has none here)
  const int32_t* rs0;          // [nl] region_start
  const int32_t* rp0;          // [nl] region_stop
  const int32_t* period;       // [nl]
  const int32_t* nsamp;        // [nl]
  const int32_t* chrom_fail;   // [nl] 1 = status 1 (the check of :292 needs the 64-bit chrom_len: taken on the host)
  const int32_t* woff;         // [nl+1] windows
  const char*    window;
  int32_t*  bounds;            // [4*nl] uploaded as INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN: min start / max stop of all, of the flagged reads
  // workspace
  uint64_t* hash;              // [n]
  int32_t*  osrc;              // [n+nl] per option of block 1 (a locus' options from lread_off + locus on): >= 0 an offset into bases, < 0: -1 - offset into window
  int32_t*  olen;              // [n+nl]
  int32_t*  l_opt;             // [nl+1] options in front of the locus
  int32_t*  l_seq;             // [nl+1] sequence bytes in front of it
  // results (one copy back): in this order in the block
  int32_t*  lres;              // [HS_HAPGEN_LRES*nl]
  int32_t*  ext_off;           // [n]
  int32_t*  ext_len;           // [n]
  int32_t*  dist_len;          // [n] per distinct string, a locus' from lread_off on, (length, bytes) order
  int32_t*  dist_rep;          // [n]
  int32_t*  dist_reads;        // [n]
  int32_t*  dist_strong;       // [n]
  double*   dist_frac;         // [n]
  int32_t*  opt_off;           // [n+3*nl+1]
  char*     seq;
  int32_t   n, nl, hash_bits, pad;
};
