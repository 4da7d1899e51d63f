// census_layout.h — device-side description of the allele census (census.hip, api.hip: hipstr_post_census): the stutter-candidate alleles of
// SeqStutterGenotyper::get_stutter_candidate_alleles (seq_stutter_genotyper.cpp:843-879) and the called / spanned marks of get_unused_alleles
// (:229-315) on the resident posteriors.  Every size decision of the stage is taken here; the per-item pieces of the kernels that need no
// device (string hash, classing, key counting, the candidate order) are plain functions of this header, so a host program can run them
// against a plain loop (tools/census_host_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HS_CENSUS_HD __host__ __device__
#else
#define HS_CENSUS_HD
#endif

// ---- launch decisions: the one place each is taken.  census.hip and hipstr_post_census (api.hip) call them, hipstr_debug_census_plan reports them.
#define HS_CENSUS_THREADS 256          // threads of a census workgroup (four wavefronts)
#define HS_CENSUS_WAVE_REQS 64         // a locus of at most this many requests ...
#define HS_CENSUS_WAVE_READS 256       // ... and this many un-pooled reads takes ONE wavefront, four loci per workgroup (route 0)
#define HS_CENSUS_LDS_INTS 12288       // 48 KiB: a larger locus whose workspace fits this many LDS dwords has a workgroup (route 1: three workgroups
                                       // share a CU's 160 KiB); beyond it the workspace lies in a global block (route 2)
#define HS_CENSUS_REQ_INTS 3           // workspace dwords per request: hash, class, flags
#define HS_CENSUS_ROUTE_WAVE 0
#define HS_CENSUS_ROUTE_LDS 1
#define HS_CENSUS_ROUTE_GLOBAL 2
// flags of a request
#define HS_CENSUS_SPAN 1               // its trace spans block 1: aln_start < blk_start && aln_stop > blk_end, both strict (:856-857, :274-275)
#define HS_CENSUS_QUAL 2               // canonical request of a class some sample counted often enough (:869)
#define HS_CENSUS_CAND 4               // ... and block 1 does not hold the string (:870): a candidate

// workspace of a locus: per request hash, class, flags; one key per read that spans with stutter (at most every read); the key counter
HS_CENSUS_HD inline int64_t hs_census_ws_ints(int64_t n_req, int64_t n_reads){ return HS_CENSUS_REQ_INTS*n_req + n_reads + 1; }
#define HS_CENSUS_WAVE_INTS (HS_CENSUS_REQ_INTS*HS_CENSUS_WAVE_REQS + HS_CENSUS_WAVE_READS + 1)
HS_CENSUS_HD inline int hs_census_route(int64_t n_req, int64_t n_reads){
  if (n_req <= HS_CENSUS_WAVE_REQS && n_reads <= HS_CENSUS_WAVE_READS) return HS_CENSUS_ROUTE_WAVE;
  return hs_census_ws_ints(n_req, n_reads) <= HS_CENSUS_LDS_INTS ? HS_CENSUS_ROUTE_LDS : HS_CENSUS_ROUTE_GLOBAL;
}
// workgroups of a route's launch over n loci
HS_CENSUS_HD inline int64_t hs_census_workgroups(int route, int64_t n_loci){
  const int per_wg = route == HS_CENSUS_ROUTE_WAVE ? HS_CENSUS_THREADS/64 : 1;
  return (n_loci + per_wg - 1)/per_wg;
}
// a global workspace starts on a 128-byte line of its own
HS_CENSUS_HD inline int64_t hs_census_ws_stride(int64_t n_req, int64_t n_reads){ return (hs_census_ws_ints(n_req, n_reads) + 31) & ~(int64_t)31; }

// ---- per-item pieces (host-testable)
// FNV-1a over the bytes of a string
HS_CENSUS_HD inline uint32_t hs_census_hash(const char* s, int len){
  uint32_t h = 2166136261u;
  for (int i = 0; i < len; i++){ h ^= (uint8_t)s[i]; h *= 16777619u; }
  return h;
}
HS_CENSUS_HD inline bool hs_census_same(const char* a, const char* b, int len){
  for (int i = 0; i < len; i++) if (a[i] != b[i]) return false;
  return true;
}
// class of request q of a locus: the lowest-numbered request of the locus with the same CONTENT — equal length, equal hash and then equal
// bytes.  off: the locus' entries of str_seq_off (off[q] .. off[q+1] are request q's bytes in seq); hash: the locus' hashes.
HS_CENSUS_HD inline int hs_census_class_of(int q, const int32_t* hash, const int32_t* off, const char* seq){
  const int len = off[q+1] - off[q], h = hash[q];
  for (int p = 0; p < q; p++)
    if (hash[p] == h && off[p+1] - off[p] == len && hs_census_same(seq + off[p], seq + off[q], len)) return p;
  return q;
}
// occurrences of `key` among n keys (integers: any order)
HS_CENSUS_HD inline int hs_census_count_key(const int32_t* keys, int n, int32_t key){
  int c = 0;
  for (int i = 0; i < n; i++) c += keys[i] == key ? 1 : 0;
  return c;
}
// the test of :869: at least min_reads reads, and — one double division, compared as written — at least min_frac of the sample's spanning reads
HS_CENSUS_HD inline bool hs_census_qualifies(int count, int n_spanning, int min_reads, double min_frac){
  return count >= min_reads && 1.0*count/n_spanning >= min_frac;
}
// orderByLengthAndSequence (stringops.cpp:35-39): shorter first, equal lengths bytewise
HS_CENSUS_HD inline bool hs_census_less(const char* a, int la, const char* b, int lb){
  if (la != lb) return la < lb;
  for (int i = 0; i < la; i++) if (a[i] != b[i]) return (uint8_t)a[i] < (uint8_t)b[i];
  return false;
}
// position of candidate q among the locus' candidates (distinct strings: a strict order), flags as left by the candidate test
HS_CENSUS_HD inline int hs_census_rank_of(int q, int n_req, const int32_t* flags, const int32_t* off, const char* seq){
  const int len = off[q+1] - off[q];
  int rank = 0;
  for (int p = 0; p < n_req; p++)
    if (p != q && (flags[p] & HS_CENSUS_CAND) && hs_census_less(seq + off[p], off[p+1] - off[p], seq + off[q], len)) rank++;
  return rank;
}

// One locus of a census.
struct hs_census_locus_t {
  int64_t ll_off;                  // the locus' [R x A] block in log_aln_probs
  int64_t ws_off;                  // route 2: the locus' workspace in ws (dwords)
  int32_t read_begin, n_reads;     // un-pooled reads
  int32_t req_begin, n_req;        // the locus' requests (grouped by locus, in locus order)
  int32_t samp_begin, n_samp;      // global sample slots
  int32_t n_alleles, hap_begin;    // haplotypes; hap_begin = hap_off[locus] (into hap_to_allele)
  int32_t blk_start, blk_end;      // of block 1
  int32_t opt_begin[3], n_opts[3]; // every block's options in opt_off's enumeration (into called / spanned)
  int32_t o1_begin;                // block 1's options in o1_off
  int32_t haploid;
};

struct hs_census_dev_t {
  const hs_census_locus_t* loci;
  const int32_t* list[3];          // loci of every route
  int32_t  n_list[3];
  int32_t  n_loci, n_req, cap_cand;
  // the posterior run's
  const double*  log_aln_probs;
  const double*  log_p1;
  const double*  log_p2;
  const int32_t* map_gt;
  // per read
  const int32_t* seed;
  const int32_t* read_req;
  const int32_t* read_samp;        // global sample slot of the read
  // per request: the five trace fields
  const int32_t* aln_start, *aln_stop, *stutter_size, *str_seq_off;
  const char*    str_seq;
  const int32_t* req_locus;
  // block 1's option strings
  const int32_t* o1_off;
  const char*    o1_seq;
  const int32_t* h2a[3];           // hap_to_allele per block or NULL
  const uint8_t* uncallable;       // per sample or NULL
  int32_t  min_reads;
  double   min_frac;
  // results
  int32_t* cand_off;               // [n_loci+1] (hs_census_scan_kernel)
  int32_t* cand_req;               // [cap_cand]
  int32_t* n_spanning, *n_span_stutter;   // [n_samp], zeroed before the launch
  uint8_t* called, *spanned;       // [n_opts], zeroed before the launch
  // scratch
  int32_t* cand_count;             // [n_loci], zeroed before the launch
  int32_t* req_rank;               // [n_req] position of a candidate in its locus, -1 otherwise
  uint8_t* has_read;               // [n_samp] a read with seed >= 0, zeroed before the launch
  int32_t* ws;                     // route 2
  // ---- only with the trace fields of a resident traceback result (hipstr_post_census_dev); NULL / 0 otherwise
  int32_t* check;                  // [2] HS_CENSUS_BAD_* found by hs_census_check_kernel, the lowest read of HS_CENSUS_BAD_NO_STR
  int32_t  n_reads;                // un-pooled reads of the batch
  int32_t  check_offsets;          // the handle's offsets are not known to ascend
  int64_t  str_total;              // elements of str_seq
  int32_t* cand_seq_off;           // [cap_cand+1] (hs_census_gather_kernel)
  char*    cand_seq;               // [min(cap_chars, str_total)]
  int64_t* cand_chars;             // [1] bytes of the candidates' strings
  int32_t  cap_chars;
};
// what hs_census_check_kernel can find in the trace fields
#define HS_CENSUS_NO_STR_DATA (-100000)   // == HIPSTR_NO_STR_DATA
#define HS_CENSUS_BAD_NEGATIVE 1       // str_seq_off[0] < 0
#define HS_CENSUS_BAD_DECREASE 2       // str_seq_off decreases, or ends beyond str_seq
#define HS_CENSUS_BAD_NO_STR 4         // a spanning request without STR data used by a read with a seed
