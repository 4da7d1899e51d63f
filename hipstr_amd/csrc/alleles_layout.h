// alleles_layout.h — device-side description of the allele-set update between two genotype() rounds (alleles.hip: hipstr_alleles_apply;
// host form: alleles_host.cpp), and the arithmetic both forms share word for word: the options' polynomial hash, a haplotype's key from
// its three options, the table slot, the Gray code's digits and the byte comparison of two haplotypes through their options.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pool_layout.h"      // HS_POOL_HD, hs_pool_mix, hs_pool_chunk_end

#define HS_ALLELES_HD HS_POOL_HD

// ---- size decisions: the one place each is taken.  alleles.hip's kernel and hipstr_alleles_apply use them; the tests read them through
// hipstr_debug_alleles_limits.
#define HS_ALLELES_THREADS 256         // threads of the locus' workgroup (four wavefronts)
#define HS_ALLELES_MAX_HAPS 1024       // most haplotypes of a locus, before and after the update, the workgroup takes (max_total_haplotypes is 1000)
#define HS_ALLELES_MAX_OPTS 1024       // most options of a locus' three blocks together, before and after ([1,1000,1] has 1002)
#define HS_ALLELES_SLOTS 2048          // slots of the LDS table: a power of two, at least twice MAX_HAPS, so a probe always ends at a free slot
#define HS_ALLELES_WS_MIB 256          // workspace budget of a chunk of whole loci (HIPSTR_ALLELES_WS_MIB overrides it)
#define HS_ALLELES_LOCUS_FIXED 256     // bytes of per-locus tables
#define HS_ALLELES_OPT_FIXED 24        // bytes of tables per option, old or new
#define HS_ALLELES_HAP_FIXED 24        // bytes of results per haplotype, old or new
#define HS_ALLELES_MAX_CHUNK_BYTES 1073741824      // device offsets are 32-bit: a locus that takes more goes to the host code

// LDS of the workgroup: per option (old and new) hash, B^length and length; the table's two dwords per slot; the mapping
#define HS_ALLELES_LDS_BYTES (2*HS_ALLELES_MAX_OPTS*20 + HS_ALLELES_SLOTS*8 + HS_ALLELES_MAX_HAPS*4 + 64)

#define HS_ALLELES_BASE 0x9E3779B97F4A7C15ull      // odd: multiplication by it is a bijection of 64-bit words

HS_ALLELES_HD inline int hs_alleles_on_device(int64_t old_haps, int64_t new_haps, int64_t old_opts, int64_t new_opts, int64_t bytes){
  return old_haps <= HS_ALLELES_MAX_HAPS && new_haps <= HS_ALLELES_MAX_HAPS && old_opts <= HS_ALLELES_MAX_OPTS && new_opts <= HS_ALLELES_MAX_OPTS &&
         bytes <= HS_ALLELES_MAX_CHUNK_BYTES;
}
// workspace a locus takes of a chunk: the old strings, the adds, the new strings, and the tables
HS_ALLELES_HD inline int64_t hs_alleles_locus_bytes(int64_t old_haps, int64_t new_haps, int64_t old_opts, int64_t new_opts, int64_t old_seq, int64_t add_seq, int64_t new_seq){
  return HS_ALLELES_LOCUS_FIXED + (old_opts + new_opts)*HS_ALLELES_OPT_FIXED + (old_haps + new_haps)*HS_ALLELES_HAP_FIXED + old_seq + add_seq + new_seq;
}

// The hash of a string s of length n: sum (s[i] + 1) * B^(n-1-i) mod 2^64 — so hash(xy) = hash(x) * B^|y| + hash(y): a wavefront folds the
// pieces of its lanes in order, and a haplotype's hash follows from its options' (hash, B^length) without touching a byte.
HS_ALLELES_HD inline uint64_t hs_alleles_hash_step(uint64_t h, char c){ return h*HS_ALLELES_BASE + (uint64_t)(uint8_t)c + 1; }
HS_ALLELES_HD inline uint64_t hs_alleles_hap_hash(uint64_t h0, uint64_t h1, uint64_t pw1, uint64_t h2, uint64_t pw2, int bits){
  const uint64_t h = (h0*pw1 + h1)*pw2 + h2;
  return (bits > 0 && bits < 64) ? (h & (((uint64_t)1 << bits) - 1)) : h;      // hipstr_debug_alleles_hash_bits: collisions at test sizes
}
HS_ALLELES_HD inline uint32_t hs_alleles_slot(uint64_t hap_hash, int64_t total_len, uint32_t slots){
  return (uint32_t)hs_pool_mix(hap_hash ^ ((uint64_t)total_len*0xC2B2AE3D27D4EB4Full)) & (slots - 1);
}
// the option of every block in haplotype k: Haplotype::next's visit order (Haplotype.cpp:157-196) — a reflected mixed-radix Gray code,
// block 0 the fastest digit; prep.cpp's allele_options
HS_ALLELES_HD inline void hs_alleles_digits(int n0, int n1, int n2, int k, int* o0, int* o1, int* o2){
  const int d0 = k % n0, q0 = k / n0;
  *o0 = (q0 & 1) ? n0 - 1 - d0 : d0;
  const int d1 = q0 % n1, q1 = q0 / n1;
  *o1 = (q1 & 1) ? n1 - 1 - d1 : d1;
  const int d2 = q1 % n2, q2 = q1 / n2;
  *o2 = (q2 & 1) ? n2 - 1 - d2 : d2;
}
// Two haplotypes of equal total length, each the concatenation of three runs of bytes: equal iff every byte is.  *bytes counts the bytes looked at.
HS_ALLELES_HD inline bool hs_alleles_equal(const char* a0, int la0, const char* a1, int la1, const char* a2, int la2,
                                           const char* b0, int lb0, const char* b1, int lb1, const char* b2, int lb2){
  int n = la0 + la1 + la2, sa = 0, sb = 0, ia = 0, ib = 0;
  const char* pa = a0; int ea = la0;
  const char* pb = b0; int eb = lb0;
  while (n > 0){
    while (ia == ea){ sa++; ia = 0; pa = sa == 1 ? a1 : a2; ea = sa == 1 ? la1 : la2; }
    while (ib == eb){ sb++; ib = 0; pb = sb == 1 ? b1 : b2; eb = sb == 1 ? lb1 : lb2; }
    const int run = (ea - ia) < (eb - ib) ? (ea - ia) : (eb - ib);
    for (int k = 0; k < run; k++) if (pa[ia + k] != pb[ib + k]) return false;
    ia += run; ib += run; n -= run;
  }
  return true;
}

// What the kernel takes (by value).  Loci, options, haplotypes and byte offsets are chunk-local; every array is a piece of the chunk's one
// device block.
struct hs_alleles_dev_t {
  // uploaded, per locus
  const int32_t* nopts;        // [6*nl] the three old counts, then the three new ones
  const int32_t* l_oopt;       // [nl+1] first old option
  const int32_t* l_nopt;       // [nl+1] first new option
  const int32_t* l_ohap;       // [nl+1] first old haplotype
  const int32_t* l_nhap;       // [nl+1] first new haplotype
  // uploaded, per option
  const int32_t* o_off;        // [old options + 1] into old_seq
  const int32_t* n_off;        // [new options + 1] into new_seq
  const int32_t* n_src;        // [new options] where its bytes come from: >= 0 an offset into old_seq, < 0: -1 - offset into add_seq
  const char*    old_seq;
  const char*    add_seq;
  // results (one copy back): in this order in the block
  int32_t* mapping;            // [old haplotypes]
  int32_t* h2a;                // [3 * new haplotypes] a locus' three rows back to back from 3*l_nhap on
  int32_t* counts;             // [2*nl] table probes, byte comparisons
  uint8_t* realign;            // [new haplotypes]
  char*    new_seq;
  int32_t  nl, hash_bits;
};
