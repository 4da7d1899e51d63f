// pool_layout.h — device-side description of the read pooler (pool.hip: hipstr_pool_reads; host twin: pool_host.cpp): ReadPooler's pools
// (read_pooler.cpp:3-20) and the per-position median base qualities of their members (base_quality.cpp:11-28).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HS_POOL_HD __host__ __device__
#else
#define HS_POOL_HD
#endif

// ---- size decisions: the one place each is taken.  pool.hip's kernels and hipstr_pool_reads call them, hipstr_debug_pool_plan reports them.
#define HS_POOL_THREADS 256            // threads of a workgroup (four wavefronts)
#define HS_POOL_LDS_READS 4096         // a locus of up to this many reads is grouped in LDS; a larger one is pooled by the host twin
#define HS_POOL_NET 8                  // a pool of up to this many members takes its medians from a sorting network in registers
#define HS_POOL_HASH_STEP 16           // bytes a lane of the hash wavefront loads per step (a wavefront: 1024 bytes per step)
#define HS_POOL_ALIGN 16               // reads start at multiples of this in the device's copy (pad bytes are zero)
#define HS_POOL_MIN_SLOTS 64           // fewest slots of a locus' hash table
#define HS_POOL_WS_MIB 512             // workspace budget of a chunk of whole loci (HIPSTR_POOL_WS_MIB overrides it)
#define HS_POOL_READ_FIXED 64          // bytes of per-read tables a read takes of the workspace, whatever its length
#define HS_POOL_LOCUS_FIXED 32         // bytes of per-locus tables
#define HS_POOL_MAX_LOCUS_BYTES 1073741824      // a locus whose padded reads take more goes to the host twin (device offsets are 32-bit)

#define HS_POOL_ROUTE_COPY 0           // median routes by pool size: 1 member
#define HS_POOL_ROUTE_NET 1            // 2 .. HS_POOL_NET
#define HS_POOL_ROUTE_RADIX 2          // beyond: bitwise radix select, eight counting passes over the members
#define HS_POOL_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull      // a free slot of the hash table (no hash takes this value: hs_pool_hash_finish)

HS_POOL_HD inline int hs_pool_median_route(int n){ return n <= 1 ? HS_POOL_ROUTE_COPY : n <= HS_POOL_NET ? HS_POOL_ROUTE_NET : HS_POOL_ROUTE_RADIX; }
HS_POOL_HD inline int64_t hs_pool_pad(int64_t len){ return (len + HS_POOL_ALIGN - 1) & ~(int64_t)(HS_POOL_ALIGN - 1); }
HS_POOL_HD inline int hs_pool_hash_steps(int64_t len){ return (int)((len + 64*HS_POOL_HASH_STEP - 1) / (64*HS_POOL_HASH_STEP)); }
// slots of a locus' table: the power of two that leaves it at most half full
HS_POOL_HD inline int hs_pool_table_slots(int n_reads){
  int s = HS_POOL_MIN_SLOTS; while (s < 2*n_reads) s <<= 1;
  return s;
}
// LDS of the grouping workgroup for a launch whose largest locus has n_reads reads: the table's keys (8 bytes a slot; once the table is
// built the same bytes hold four dwords per read: pool size, first member, fill cursor, pool number), its leaders (4 bytes a slot), the slot
// of every read, and the scan's partial sums
HS_POOL_HD inline size_t hs_pool_lds_bytes(int n_reads){ return (size_t)hs_pool_table_slots(n_reads)*12 + (size_t)n_reads*4 + 64; }
HS_POOL_HD inline int hs_pool_on_device(int64_t n_reads, int64_t padded_bytes){ return n_reads <= HS_POOL_LDS_READS && padded_bytes <= HS_POOL_MAX_LOCUS_BYTES; }
HS_POOL_HD inline int64_t hs_pool_read_bytes(int64_t len){ return 3*hs_pool_pad(len) + HS_POOL_READ_FIXED; }      // bases, qualities, median qualities + tables

// The hash of a read: a sum over its 16-byte pieces (any order: the lanes of a wavefront add theirs up) of two mixed 64-bit words salted
// with the piece's number, closed with the length; `bits` < 64 keeps the low bits only (HIPSTR_DEBUG_POOL_HASH_BITS: collisions at test sizes).
HS_POOL_HD inline uint64_t hs_pool_mix(uint64_t x){       // the finaliser of MurmurHash3 (public domain): a bijection of 64-bit words
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
HS_POOL_HD inline uint64_t hs_pool_hash_piece(uint64_t lo, uint64_t hi, uint64_t piece){
  return hs_pool_mix(lo + (2*piece + 1)*0x9E3779B97F4A7C15ull) + hs_pool_mix(hi + (2*piece + 2)*0xC2B2AE3D27D4EB4Full);
}
HS_POOL_HD inline uint64_t hs_pool_hash_finish(uint64_t sum, int64_t len, int bits){
  uint64_t h = hs_pool_mix(sum ^ hs_pool_mix((uint64_t)len + 0x165667B19E3779F9ull));
  if (bits > 0 && bits < 64) h &= (((uint64_t)1 << bits) - 1);
  return h == HS_POOL_EMPTY_KEY ? h - 1 : h;
}

// chunk [l0, end) of whole loci under a budget: per-locus workspace bytes in `cost` (0 for a locus the host pools); at least one locus
inline int hs_pool_chunk_end(const int64_t* cost, int l0, int n_loci, int64_t budget){
  int64_t sum = 0; int l = l0;
  while (l < n_loci && (l == l0 || sum + cost[l] <= budget)){ sum += cost[l]; l++; }
  return l;
}

// What the kernels take (by value).  Read indices are chunk-local; every array is a piece of the chunk's one device block.
struct hs_pool_dev_t {
  // uploaded
  const int32_t* len;          // [n] bases of a read
  const int32_t* doff;         // [n] where its bases / qualities start (multiples of HS_POOL_ALIGN)
  const int32_t* lread_off;    // [nl+1] reads of a locus (a locus the host pools has none here)
  const char*    bases;        // padded, pad bytes zero
  const char*    quals;
  // workspace
  uint64_t* hash;              // [n]
  int32_t*  members;           // [n] the loci's pools' members, pool after pool
  int32_t*  p_rep;             // [n] per slot (a locus' slot p = its pool p, at lread_off + p): first read
  int32_t*  p_size;            // [n] members; 0 = the slot holds no pool
  int32_t*  p_qoff;            // [n] start of the pool's qualities within its locus
  int32_t*  p_moff;            // [n] start of its members in members[]
  int32_t*  slot_locus;        // [n]
  int32_t*  qbytes;            // [nl] quality bytes of the locus' pools
  // results (one copy back): in this order in the block
  int32_t*  pool_index;        // [n]
  int32_t*  n_pools;           // [nl]
  int32_t*  collision;         // [nl] 1 = two reads with one hash differ: the host redoes the locus
  int32_t*  pool_off;          // [nl+1]
  int32_t*  qual_base;         // [nl+1] start of the locus' pool qualities in out_quals
  int32_t*  out_rep;           // [n] per pool, pool_off order
  int32_t*  out_size;          // [n]
  int32_t*  out_qoff;          // [n]
  char*     out_quals;
  int32_t   n, nl, hash_bits, pad;
};
