// flank_layout.h — every size and every decision of size of the flank reassembly stage (flank.hip, flank_task.h): the De Bruijn assembly of
// SeqStutterGenotyper::assemble_flanks (seq_stutter_genotyper.cpp:40-217), one wavefront per (locus, flank, sample) task.  Host and device
// read the same functions; hipstr_debug_flank_plan reports them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HS_FLK_HD __host__ __device__
#else
#define HS_FLK_HD
#endif

#define HS_FLK_WAVE         64        // lanes of a task's wavefront (the workgroup is one wavefront)
#define HS_FLK_MAX_K        15        // largest k the device packs: a (k+1)-mer of 3-bit codes is 48 bits
#define HS_FLK_K_STEPS      6         // values of k one task may try (the reference's 10 .. 15)
#define HS_FLK_EDGE_SLOTS   1024      // LDS hash table of distinct (k+1)-mers (power of two)
#define HS_FLK_NODE_SLOTS   1024      // LDS hash table of distinct k-mers (power of two)
#define HS_FLK_MAX_EDGES    512       // distinct edges of one graph: half the slots
#define HS_FLK_MAX_NODES    512       // distinct nodes of one graph: half the slots
#define HS_FLK_MAX_RECS     1024      // path records of one enumeration (every push makes one; the heap holds indices of them)
#define HS_FLK_MAX_READS    4096      // reads of one (locus, sample) run; the first-occurrence key holds read+1 in 16 bits
#define HS_FLK_MAX_LEN      4096      // bases of one string (reference flank or read flank); the key holds the position in 16 bits
#define HS_FLK_MAX_PATHS    16        // max_paths the device serves
#define HS_FLK_MAX_PATH_LEN 1024      // bases of one emitted path
#define HS_FLK_PEEL_SLACK   2         // peeling rounds allowed beyond the node cap (the last round finds nothing)
#define HS_FLK_EMPTY        (~0ull)   // an empty slot of either table
#define HS_FLK_NO_REC       0xFFFFu   // a path record without parent

// Largest sizes seen, all on the device under these caps (hipstr_debug_flank_plan; tests/test_flank_gpu.py and
// tests/test_flow_chain_flanks_gpu.py assert that no task of theirs takes the host twin):
//                                         edges  nodes  records  reads  string  path
//   unit cases (tests/flank_cases.py)       114    111      387    101      80    80
//   200 random tasks                         99     99       92     16      77    61
//   six flow cases (148 tasks)               68     66       52     19      35    35

// why a task left the device (bits of task_flag); 0 = assembled on the device
#define HS_FLK_F_EDGES  0x01    // more distinct edges than the cap (or a probe sequence that ran out)
#define HS_FLK_F_NODES  0x02
#define HS_FLK_F_RECS   0x04    // more path records than the cap
#define HS_FLK_F_READS  0x08    // more reads in the run than the cap
#define HS_FLK_F_LEN    0x10    // a string, or an emitted path, longer than the cap
#define HS_FLK_F_BYTE   0x20    // a byte other than A, C, G, T, N
#define HS_FLK_F_K      0x40    // k outside what the device packs, or more values of k than HS_FLK_K_STEPS
#define HS_FLK_F_POOL   0x80    // the path pool of the call ran out
#define HS_FLK_F_PEEL   0x100   // the peeling rounds ran out (cannot happen below the node cap; the loop is bounded all the same)
#define HS_FLK_F_PARAM  0x200   // max_paths above HS_FLK_MAX_PATHS: the whole call's tasks
#define HS_FLK_F_RANGE  0x400   // a flank offset that leaves the handle's pool: the call is refused once the host has seen the offsets

// the caps of one call: the compiled limits, or smaller ones from HIPSTR_DEBUG_FLANK_CAPS (tests reach the fallback at test sizes)
struct hs_flk_caps_t { int32_t max_edges, max_nodes, max_recs, max_reads, max_len, max_path_len; };

HS_FLK_HD inline hs_flk_caps_t hs_flk_default_caps(){
  hs_flk_caps_t c = { HS_FLK_MAX_EDGES, HS_FLK_MAX_NODES, HS_FLK_MAX_RECS, HS_FLK_MAX_READS, HS_FLK_MAX_LEN, HS_FLK_MAX_PATH_LEN };
  return c;
}
// a requested cap is clamped into [1, compiled limit]
HS_FLK_HD inline int32_t hs_flk_clamp_cap(int64_t want, int32_t limit){ return want < 1 ? 1 : (want > limit ? limit : (int32_t)want); }

// 3-bit code of a base, -1 for a byte the device does not pack
HS_FLK_HD inline int hs_flk_code(char c){ return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : c == 'N' ? 4 : -1; }
HS_FLK_HD inline char hs_flk_base(int code){ return code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : code == 3 ? 'T' : 'N'; }

// decisions the host takes before the launch
HS_FLK_HD inline bool hs_flk_k_fits(int k0, int max_k){ return k0 >= 1 && max_k <= HS_FLK_MAX_K && max_k - k0 + 1 <= HS_FLK_K_STEPS; }
HS_FLK_HD inline bool hs_flk_reads_fit(int64_t n_reads, const hs_flk_caps_t& c){ return n_reads <= c.max_reads; }
HS_FLK_HD inline bool hs_flk_len_fits(int64_t len, const hs_flk_caps_t& c){ return len <= c.max_len; }
HS_FLK_HD inline bool hs_flk_paths_fit(int max_paths){ return max_paths >= 0 && max_paths <= HS_FLK_MAX_PATHS; }
// the flags a task of these needs gets (what the kernel decides step by step, decided at once: hipstr_debug_flank_plan)
HS_FLK_HD inline int hs_flk_task_flags(int k0, int max_k, int max_paths, int edges, int nodes, int recs, int reads, int len, int path_len, int bad_byte,
                                       const hs_flk_caps_t& c){
  int f = 0;
  if (!hs_flk_k_fits(k0, max_k)) f |= HS_FLK_F_K;
  if (!hs_flk_paths_fit(max_paths)) f |= HS_FLK_F_PARAM;
  if (!hs_flk_reads_fit(reads, c)) f |= HS_FLK_F_READS;
  if (!hs_flk_len_fits(len, c) || path_len > c.max_path_len) f |= HS_FLK_F_LEN;
  if (edges > c.max_edges) f |= HS_FLK_F_EDGES;
  if (nodes > c.max_nodes) f |= HS_FLK_F_NODES;
  if (recs > c.max_recs) f |= HS_FLK_F_RECS;
  if (bad_byte) f |= HS_FLK_F_BYTE;
  return f;
}
// the peeling rounds of one graph: every round but the last removes a node
HS_FLK_HD inline int hs_flk_peel_rounds(const hs_flk_caps_t& c){ return c.max_nodes + HS_FLK_PEEL_SLACK; }
// bytes one path takes in the call's pool: weight, length, the bases padded to 4 bytes
HS_FLK_HD inline int hs_flk_path_bytes(int len){ return 8 + ((len + 3) & ~3); }
// bytes of the call's path pool: four reference flanks' worth per task and a floor; a task that finds it full goes to the host
HS_FLK_HD inline int64_t hs_flk_pool_bytes(int64_t n_tasks, int64_t sum_ref_len){ return 4*sum_ref_len + 64*n_tasks + 4096; }
HS_FLK_HD inline uint32_t hs_flk_hash(uint64_t key, int slots){ return (uint32_t)((key*0x9E3779B97F4A7C15ull) >> 40) & (uint32_t)(slots - 1); }

// LDS of one task (one workgroup)
struct hs_flk_lds_t {
  unsigned long long ekey[HS_FLK_EDGE_SLOTS];      // packed (k+1)-mer, first base in the highest code
  int32_t  ew[HS_FLK_EDGE_SLOTS];                  // weight: 2 per occurrence in the reference flank, 1 per occurrence in a read
  uint32_t efirst[HS_FLK_EDGE_SLOTS];              // first occurrence: string << 16 | position (string 0 = the reference flank): the edge-id order
  uint16_t esrc[HS_FLK_EDGE_SLOTS], edst[HS_FLK_EDGE_SLOTS];      // node slots
  uint8_t  ekeep[HS_FLK_EDGE_SLOTS];               // survives prune_edges
  unsigned long long nkey[HS_FLK_NODE_SLOTS];      // packed k-mer
  uint8_t  nin[HS_FLK_NODE_SLOTS], nout[HS_FLK_NODE_SLOTS];       // kept incident / departing edges
  uint8_t  nflag[HS_FLK_NODE_SLOTS];               // HS_FLK_N_*
  int32_t  rw[HS_FLK_MAX_RECS];                    // path records: min_weight,
  uint16_t rnode[HS_FLK_MAX_RECS], rparent[HS_FLK_MAX_RECS];      //   node slot and parent record
  uint16_t heap[HS_FLK_MAX_RECS];
  uint16_t emit[HS_FLK_MAX_PATHS];                 // the records of the sink paths, in pop order,
  int32_t  plen[HS_FLK_MAX_PATHS];                 //   and their lengths
  int32_t  n_edges, n_nodes, n_live, n_removed, changed, flag, ok, result_k, n_paths, path_at;
  int32_t  max_edges_seen, max_nodes_seen, max_recs_seen;
};
#define HS_FLK_N_LIVE    1
#define HS_FLK_N_REMOVED 2
#define HS_FLK_N_SINK    4

static_assert(sizeof(hs_flk_lds_t) <= 65536, "one workgroup's LDS");
static_assert(HS_FLK_MAX_EDGES*2 <= HS_FLK_EDGE_SLOTS && HS_FLK_MAX_NODES*2 <= HS_FLK_NODE_SLOTS, "the tables stay at most half full");
static_assert(HS_FLK_MAX_READS < 65535 && HS_FLK_MAX_LEN <= 65536 && HS_FLK_MAX_RECS < HS_FLK_NO_REC && HS_FLK_NODE_SLOTS <= 65536, "16-bit fields");
static_assert(3*(HS_FLK_MAX_K + 1) <= 48, "a (k+1)-mer fits 48 bits");

// per-task sizes the kernel reports (task_size[4*t ..]): most edges, nodes, records over the k tried; strings that entered
#define HS_FLK_SIZES 4

// what the kernel reads and writes
struct hs_post_unit_t;
struct hs_flk_dev_t {
  const hs_post_unit_t* units;         // the posterior run's (locus, sample) runs of reads; unit index == global sample slot
  const int32_t* task_unit;            // [n_tasks]
  const int32_t* task_lf;              // [n_tasks] 2*locus + flank
  const uint8_t* task_skip;            // [n_tasks] nothing to do (a masked sample, a flank without k)
  const int32_t* ref_off;              // [2*n_loci+1] the reference flanks, back to back
  const char*    ref_seq;
  const int32_t* kmer0;                // [2*n_loci] calc_kmer_length
  const int32_t* max_k;                // [2*n_loci]
  const int32_t* seed;                 // [n_reads]
  const int32_t* read_req;             // [n_reads]
  const int32_t* flank_off;            // the trace handle's flank_seq_off [2*n_req+1]
  const char*    flank_seq;
  int64_t        flank_total;          // bytes of flank_seq
  int32_t* task_k;                     // [n_tasks] accepted k, -1 cyclic at every k, -2 skipped
  int32_t* task_flag;                  // [n_tasks] HS_FLK_F_*
  int32_t* task_np;                    // [n_tasks]
  int32_t* task_size;                  // [HS_FLK_SIZES*n_tasks]
  int32_t* task_at;                    // [n_tasks] where the task's paths lie in the pool: per path [min_weight][length][bases, padded to 4]
  char*    pool;                       // 4-byte aligned
  unsigned long long* pool_used;
  int64_t  pool_cap;
  int32_t  n_tasks, min_path_weight, max_paths;
  hs_flk_caps_t caps;
};
