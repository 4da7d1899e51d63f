// record_alleles_layout.h — what record_alleles.hip's kernel and the host share: the cap, the argument blocks, and the per-option steps of
// a wavefront — the stop tests of the two trims, the order of two options, an allele's bytes.  Plain C++ (tests/cpp/record_alleles_host_test.cpp
// runs them on the host against record_alleles_host.cpp).  Every loop has its bound in its head.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define HS_RA_FN static __host__ __device__ __attribute__((unused)) inline
#else
#define HS_RA_FN static __attribute__((unused)) inline
#endif

#define HS_RA_WAVE 64                 // one wavefront per locus
#define HS_RA_MAX_OPTIONS 256         // == HIPSTR_ALLELES_DEVICE_OPTIONS: a locus of more options is the host twin's (the ranks cost V^2 compares)
#define HS_RA_WIN_PAD 40              // window[i] = chrom_seq[region_start - 40 + i]
#define HS_RA_DUPLICATE 1
#define HS_RA_OUTSIDE 2

struct hs_ra_locus_t {
  int32_t opt0, n_opts;               // block 1's options: opt_off[opt0 .. opt0 + n_opts]
  int32_t start, end, region_start, region_stop;
  int32_t win_base, win_len;          // the locus' window
  int32_t var_off;                    // into the per-variant outputs
  int32_t on_host;                    // beyond the cap: the kernel passes by
  int64_t pool_base;                  // the locus' piece of the string pool: option i at pool_base + i*stride
  int32_t stride, pad_;
};
struct hs_ra_dev_t {
  const hs_ra_locus_t* loci;
  const int32_t* opt_off; const char* seq; const char* window;
  int32_t* scal;                      // [4*n_loci] status, pos, left_trim, right_trim
  int32_t *out_len, *bp_diff, *old_to_new, *new_to_old;      // [sum V]
  char* pool;
  int32_t n_loci;
};

HS_RA_FN char hs_ra_upper(char c){ return (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }
// does option (o, n) stop the left trim at left_trim = t?  (o0, n0): option 0   (:706)
HS_RA_FN bool hs_ra_left_stop(const char* seq, int o, int n, int o0, int n0, int t){
  if (t + 1 >= n0 || t + 1 >= n) return true;
  return seq[o + t] != seq[o0 + t];
}
// the same for the right trim at right_trim = t, on options already cut by lt on the left   (:726)
HS_RA_FN bool hs_ra_right_stop(const char* seq, int o, int n, int o0, int n0, int lt, int t){
  if (t + 1 >= n0 - lt || t + 1 >= n - lt) return true;
  return seq[o + n - t - 1] != seq[o0 + n0 - t - 1];
}
// (length, bytes as unsigned char) order of two strings: -1, 0, 1   (stringops.cpp:35-39)
HS_RA_FN int hs_ra_order(const char* a, int na, const char* b, int nb){
  if (na != nb) return na < nb ? -1 : 1;
  for (int i = 0; i < na; i++){
    const unsigned char x = (unsigned char)a[i], y = (unsigned char)b[i];
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}
