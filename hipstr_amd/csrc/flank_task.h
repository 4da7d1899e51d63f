// flank_task.h — one assembly task of the flank stage as the device runs it: the body of hs_flank_task_kernel (flank.hip), one wavefront per
// (locus, flank, sample).  It restates DebruijnGraph (debruijn_graph.cpp) over two LDS hash tables:
//   edges   every (k+1)-mer occurrence of the reference flank (weight 2) and of the sample's read flanks (weight 1) goes into a table keyed by
//           the packed (k+1)-mer; an entry sums the weights and keeps the smallest (string << 16 | position): the reference's edge id order
//   nodes   the two k-mers of every distinct edge; a node's id is its slot (no result depends on the reference's node numbering: Kahn's verdict
//           is order-free, the alternative sources and sinks are walked in k-mer order, a path's children in edge order)
//   prune   an edge survives iff the reference flank holds it or its weight reaches max(2, ceil(0.02 * strings))
//   degrees a node asks the edge table for its five possible departing and five possible incident edges; no adjacency lists are stored
//   peel    rounds: a live node all of whose kept predecessors are removed is removed; acyclic iff every live node goes
//   paths   one lane: libstdc++'s push_heap / pop_heap restated on record indices, children in first-occurrence order
// The phases are written as loops over lanes with a barrier between them, so that the same text runs as a plain C++ function where
// HS_FLK_SIMULATE is defined (tests/cpp/flank_host_test.cpp runs it against the host twin).  Every loop is bounded by a constant of
// flank_layout.h or by a cap of the call; a task that would exceed one sets a flag and ends (the host twin assembles it in the same call).
#pragma once
#include <math.h>
#include "flank_layout.h"
#include "post_layout.h"

#ifdef HS_FLK_SIMULATE
#define FLK_FN inline
#define FLK_LANES(lane) for (int lane = 0; lane < HS_FLK_WAVE; lane++)
#define FLK_SYNC() ((void)0)
inline unsigned long long flk_cas64(unsigned long long* p, unsigned long long cmp, unsigned long long v){ const unsigned long long o = *p; if (o == cmp) *p = v; return o; }
inline int flk_add(int32_t* p, int v){ const int o = *p; *p += v; return o; }
inline void flk_min_u32(uint32_t* p, uint32_t v){ if (v < *p) *p = v; }
inline void flk_or(int32_t* p, int v){ *p |= v; }
inline void flk_max(int32_t* p, int v){ if (v > *p) *p = v; }
inline unsigned long long flk_add64(unsigned long long* p, unsigned long long v){ const unsigned long long o = *p; *p += v; return o; }
#else
#define FLK_FN __device__ __forceinline__
#define FLK_LANES(lane) for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define FLK_SYNC() __syncthreads()
FLK_FN unsigned long long flk_cas64(unsigned long long* p, unsigned long long cmp, unsigned long long v){ return atomicCAS(p, cmp, v); }
FLK_FN int flk_add(int32_t* p, int v){ return atomicAdd(p, v); }
FLK_FN void flk_min_u32(uint32_t* p, uint32_t v){ atomicMin(p, v); }
FLK_FN void flk_or(int32_t* p, int v){ atomicOr(p, v); }
FLK_FN void flk_max(int32_t* p, int v){ atomicMax(p, v); }
FLK_FN unsigned long long flk_add64(unsigned long long* p, unsigned long long v){ return atomicAdd(p, v); }
#endif

// slot of `key` in a table, or -1; at most `slots` probes
FLK_FN int flk_find(const unsigned long long* tab, int slots, unsigned long long key){
  uint32_t h = hs_flk_hash(key, slots);
  for (int p = 0; p < slots; p++){
    const unsigned long long v = tab[h];
    if (v == key) return (int)h;
    if (v == HS_FLK_EMPTY) return -1;
    h = (h + 1) & (uint32_t)(slots - 1);
  }
  return -1;
}
// slot of `key`, inserted if absent (*fresh = 1 then); -1 when the probes ran out
FLK_FN int flk_insert(unsigned long long* tab, int slots, unsigned long long key, int* fresh){
  uint32_t h = hs_flk_hash(key, slots);
  *fresh = 0;
  for (int p = 0; p < slots; p++){
    unsigned long long v = tab[h];
    if (v == HS_FLK_EMPTY){ v = flk_cas64(&tab[h], HS_FLK_EMPTY, key); if (v == HS_FLK_EMPTY){ *fresh = 1; return (int)h; } }
    if (v == key) return (int)h;
    h = (h + 1) & (uint32_t)(slots - 1);
  }
  return -1;
}

// std::push_heap's sift (libstdc++ __push_heap) on record indices, ordered by min_weight: heap[0 .. n-1] is a heap, `value` enters at hole n-1
FLK_FN void flk_push_heap(uint16_t* heap, const int32_t* rw, int hole, int top, uint16_t value){
  int parent = (hole - 1)/2;
  while (hole > top && rw[heap[parent]] < rw[value]){          // (at most log2(HS_FLK_MAX_RECS) steps: the hole halves)
    heap[hole] = heap[parent]; hole = parent; parent = (hole - 1)/2;
  }
  heap[hole] = value;
}
// std::pop_heap (libstdc++ __pop_heap + __adjust_heap) on heap[0 .. n-1], n >= 1: the top goes to heap[n-1]
FLK_FN void flk_pop_heap(uint16_t* heap, const int32_t* rw, int n){
  if (n <= 1) return;
  const int len = n - 1;
  const uint16_t value = heap[len];
  heap[len] = heap[0];
  int hole = 0, child = 0;
  while (child < (len - 1)/2){
    child = 2*(child + 1);
    if (rw[heap[child]] < rw[heap[child - 1]]) child--;
    heap[hole] = heap[child]; hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2)/2){
    child = 2*(child + 1);
    heap[hole] = heap[child - 1]; hole = child - 1;
  }
  flk_push_heap(heap, rw, hole, 0, value);
}

// packed k-mer of str[pos .. pos+n), first base in the highest code; *bad is set by a byte outside ACGTN
FLK_FN unsigned long long flk_pack(const char* str, int pos, int n, int* bad){
  unsigned long long key = 0;
  for (int j = 0; j < n; j++){                                  // n <= HS_FLK_MAX_K + 1
    const int c = hs_flk_code(str[pos + j]);
    if (c < 0){ *bad = 1; return 0; }
    key = (key << 3) | (unsigned long long)c;
  }
  return key;
}

// One task.  Every lane of the wavefront calls it with the same t; L is the workgroup's LDS.
FLK_FN void hs_flk_task(const hs_flk_dev_t& d, int t, hs_flk_lds_t& L){
  const hs_flk_caps_t caps = d.caps;
  const hs_post_unit_t u = d.units[d.task_unit[t]];
  const int lf = d.task_lf[t];
  const char* ref = d.ref_seq + d.ref_off[lf];
  const int ref_len = d.ref_off[lf+1] - d.ref_off[lf];
  const int k0 = d.kmer0[lf], max_k = d.max_k[lf];
  FLK_LANES(lane){
    if (lane == 0){ L.flag = 0; L.result_k = -1; L.n_paths = 0; L.path_at = 0; L.max_edges_seen = 0; L.max_nodes_seen = 0; L.max_recs_seen = 0; L.ok = 0; }
  }
  FLK_SYNC();
  int n_entered = 0;
  if (d.task_skip[t]){
    FLK_LANES(lane){ if (lane == 0) L.result_k = -2; }
  } else if (!hs_flk_k_fits(k0, max_k)){
    FLK_LANES(lane){ if (lane == 0) L.flag = HS_FLK_F_K; }
  } else if (!hs_flk_paths_fit(d.max_paths)){
    FLK_LANES(lane){ if (lane == 0) L.flag = HS_FLK_F_PARAM; }
  } else if (!hs_flk_reads_fit(u.n_reads, caps)){
    FLK_LANES(lane){ if (lane == 0) L.flag = HS_FLK_F_READS; }
  } else if (!hs_flk_len_fits(ref_len, caps)){
    FLK_LANES(lane){ if (lane == 0) L.flag = HS_FLK_F_LEN; }
  } else {
    for (int k = k0, step = 0; k <= max_k && step < HS_FLK_K_STEPS; k++, step++){
      // ---- clear
      FLK_LANES(lane){
        for (int i = lane; i < HS_FLK_EDGE_SLOTS; i += HS_FLK_WAVE){ L.ekey[i] = HS_FLK_EMPTY; L.ew[i] = 0; L.efirst[i] = 0xFFFFFFFFu; }
        for (int i = lane; i < HS_FLK_NODE_SLOTS; i += HS_FLK_WAVE){ L.nkey[i] = HS_FLK_EMPTY; L.nflag[i] = 0; }
        if (lane == 0){ L.n_edges = 0; L.n_nodes = 0; L.n_live = 0; L.n_removed = 0; }
      }
      FLK_SYNC();
      // ---- edges: string 0 is the reference flank (weight 2), string r+1 the flank of read r of the run
      int n_strings = 0;
      for (int s = 0; s <= u.n_reads; s++){                      // u.n_reads <= caps.max_reads
        const char* str = ref; int len = ref_len;
        if (s > 0){
          const int g = u.read_begin + s - 1;
          len = 0;
          if (d.seed[g] >= 0){
            const int q = d.read_req[g];
            if (q >= 0){
              const int o = d.flank_off[2*q + (lf & 1)]; str = d.flank_seq + o; len = d.flank_off[2*q + (lf & 1) + 1] - o;
              if (o < 0 || len < 0 || (int64_t)o + len > d.flank_total){      // offsets that leave the pool (a fabricated handle): nothing is read there
                FLK_LANES(lane){ if (lane == 0) flk_or(&L.flag, HS_FLK_F_RANGE); }
                break;
              }
            }
          }
        }
        if (len <= k) continue;                                  // DebruijnGraph::add_string: not counted
        if (!hs_flk_len_fits(len, caps)){ FLK_LANES(lane){ if (lane == 0) flk_or(&L.flag, HS_FLK_F_LEN); } break; }
        n_strings++;
        const int w = s == 0 ? 2 : 1;
        FLK_LANES(lane){
          for (int i = lane; i < len - k; i += HS_FLK_WAVE){     // len <= caps.max_len
            int bad = 0, fresh = 0;
            const unsigned long long key = flk_pack(str, i, k + 1, &bad);
            if (bad){ flk_or(&L.flag, HS_FLK_F_BYTE); continue; }
            const int e = flk_insert(L.ekey, HS_FLK_EDGE_SLOTS, key, &fresh);
            if (e < 0){ flk_or(&L.flag, HS_FLK_F_EDGES); continue; }
            if (fresh && flk_add(&L.n_edges, 1) + 1 > caps.max_edges) flk_or(&L.flag, HS_FLK_F_EDGES);
            flk_add(&L.ew[e], w);
            flk_min_u32(&L.efirst[e], ((uint32_t)s << 16) | (uint32_t)i);
          }
        }
        FLK_SYNC();
        const int fl = L.flag;                                   // (read between two barriers: no lane runs ahead and sets it meanwhile)
        FLK_SYNC();
        if (fl) break;
      }
      FLK_SYNC();
      if (L.flag) break;                                         // (nothing below sets the flag before the next barrier)
      n_entered = n_strings - 1;
      // ---- nodes and pruning
      int thr = (int)ceil(0.02*(double)n_strings);               // prune_edges(0.02, 2): one double product, as written
      if (thr < 2) thr = 2;
      const unsigned long long kmask = (1ull << (3*k)) - 1ull;
      FLK_LANES(lane){
        for (int e = lane; e < HS_FLK_EDGE_SLOTS; e += HS_FLK_WAVE){
          const unsigned long long key = L.ekey[e];
          if (key == HS_FLK_EMPTY) continue;
          int f1 = 0, f2 = 0;
          const int a = flk_insert(L.nkey, HS_FLK_NODE_SLOTS, key >> 3, &f1);
          const int b = flk_insert(L.nkey, HS_FLK_NODE_SLOTS, key & kmask, &f2);
          if (a < 0 || b < 0){ flk_or(&L.flag, HS_FLK_F_NODES); continue; }
          if (f1 + f2 && flk_add(&L.n_nodes, f1 + f2) + f1 + f2 > caps.max_nodes) flk_or(&L.flag, HS_FLK_F_NODES);
          L.esrc[e] = (uint16_t)a; L.edst[e] = (uint16_t)b;
          L.ekeep[e] = ((L.efirst[e] >> 16) == 0 || L.ew[e] >= thr) ? 1 : 0;
        }
      }
      FLK_SYNC();
      FLK_LANES(lane){ if (lane == 0){ flk_max(&L.max_edges_seen, L.n_edges); flk_max(&L.max_nodes_seen, L.n_nodes); } }
      const int fl_nodes = L.flag;
      FLK_SYNC();
      if (fl_nodes) break;
      int bad_ref = 0;
      const unsigned long long src_key = flk_pack(ref, 0, k, &bad_ref), snk_key = flk_pack(ref, ref_len - k, k, &bad_ref);
      // ---- degrees over the kept edges; live nodes (prune_edges keeps the source, the sink and every end of a kept edge)
      FLK_LANES(lane){
        for (int n = lane; n < HS_FLK_NODE_SLOTS; n += HS_FLK_WAVE){
          const unsigned long long nk = L.nkey[n];
          if (nk == HS_FLK_EMPTY) continue;
          int in = 0, out = 0;
          for (int b = 0; b < 5; b++){
            const int eo = flk_find(L.ekey, HS_FLK_EDGE_SLOTS, ((nk << 3) | (unsigned long long)b));
            if (eo >= 0 && L.ekeep[eo]) out++;
            const int ei = flk_find(L.ekey, HS_FLK_EDGE_SLOTS, (((unsigned long long)b << (3*k)) | nk));
            if (ei >= 0 && L.ekeep[ei]) in++;
          }
          L.nin[n] = (uint8_t)in; L.nout[n] = (uint8_t)out;
          if (in + out > 0 || nk == src_key || nk == snk_key){ L.nflag[n] = HS_FLK_N_LIVE; flk_add(&L.n_live, 1); }
        }
      }
      FLK_SYNC();
      // ---- peeling (DirectedGraph::can_sort_topologically's verdict)
      const int rounds = hs_flk_peel_rounds(caps);
      int round = 0;
      for (; round < rounds; round++){
        FLK_LANES(lane){ if (lane == 0) L.changed = 0; }
        FLK_SYNC();
        FLK_LANES(lane){
          for (int n = lane; n < HS_FLK_NODE_SLOTS; n += HS_FLK_WAVE){
            if (L.nflag[n] != HS_FLK_N_LIVE) continue;           // (empty, dead or removed already)
            const unsigned long long nk = L.nkey[n];
            bool pred = false;
            for (int b = 0; b < 5 && !pred; b++){
              const int ei = flk_find(L.ekey, HS_FLK_EDGE_SLOTS, (((unsigned long long)b << (3*k)) | nk));
              if (ei >= 0 && L.ekeep[ei] && !(L.nflag[L.esrc[ei]] & HS_FLK_N_REMOVED)) pred = true;
            }
            if (!pred){ L.nflag[n] = HS_FLK_N_LIVE | HS_FLK_N_REMOVED; flk_add(&L.n_removed, 1); L.changed = 1; }
          }
        }
        FLK_SYNC();
        const int ch = L.changed;
        FLK_SYNC();
        if (!ch) break;
      }
      if (round == rounds){ FLK_LANES(lane){ if (lane == 0) flk_or(&L.flag, HS_FLK_F_PEEL); } FLK_SYNC(); break; }
      const int src = flk_find(L.nkey, HS_FLK_NODE_SLOTS, src_key), snk = flk_find(L.nkey, HS_FLK_NODE_SLOTS, snk_key);
      const bool good = L.n_removed == L.n_live && src >= 0 && snk >= 0 && L.nout[src] > 0 && L.nin[src] == 0 && L.nin[snk] > 0 && L.nout[snk] == 0;
      FLK_SYNC();
      if (!good) continue;                                       // has_cycles(), !is_source_ok() or !is_sink_ok(): the next k
      // ---- enumerate_paths on one lane
      FLK_LANES(lane){
        if (lane == 0){
          int n_rec = 0, n_heap = 0, n_paths = 0, flag = 0;
          L.rnode[0] = (uint16_t)src; L.rparent[0] = HS_FLK_NO_REC; L.rw[0] = 1000000; L.heap[0] = 0; n_rec = 1; n_heap = 1;
          L.nflag[snk] |= HS_FLK_N_SINK;
          for (int pass = 0; pass < 2; pass++){                  // get_alt_kmer_nodes: of the source k-mer, then of the sink k-mer
            const unsigned long long base_key = pass == 0 ? src_key : snk_key;
            for (int i = 0; i < k; i++){
              const int sh = 3*(k - 1 - i);
              const int orig = (int)((base_key >> sh) & 7ull);
              for (int b = 0; b < 4; b++){
                if (b == orig) continue;
                const unsigned long long alt = (base_key & ~(7ull << sh)) | ((unsigned long long)b << sh);
                const int n = flk_find(L.nkey, HS_FLK_NODE_SLOTS, alt);
                if (n < 0 || !(L.nflag[n] & HS_FLK_N_LIVE)) continue;
                if (pass == 0){
                  if (L.nin[n] > 0) continue;
                  if (n_rec >= caps.max_recs){ flag |= HS_FLK_F_RECS; continue; }
                  L.rnode[n_rec] = (uint16_t)n; L.rparent[n_rec] = HS_FLK_NO_REC; L.rw[n_rec] = 1000000;
                  L.heap[n_heap] = (uint16_t)n_rec; n_heap++;
                  flk_push_heap(L.heap, L.rw, n_heap - 1, 0, (uint16_t)n_rec);
                  n_rec++;
                } else if (L.nout[n] == 0) L.nflag[n] |= HS_FLK_N_SINK;
              }
            }
          }
          // every pop consumes a record: at most caps.max_recs pops
          for (int pops = 0; n_heap > 0 && n_paths < d.max_paths && !flag && pops < caps.max_recs; pops++){
            flk_pop_heap(L.heap, L.rw, n_heap);
            const int best = L.heap[n_heap - 1]; n_heap--;
            const int node = L.rnode[best];
            if (L.nflag[node] & HS_FLK_N_SINK){
              int depth = 0;
              for (int p = L.rparent[best]; p != (int)HS_FLK_NO_REC && depth <= caps.max_recs; p = L.rparent[p]) depth++;      // a parent has a smaller index
              const int len = k + depth;
              if (len > caps.max_path_len){ flag |= HS_FLK_F_LEN; break; }
              L.emit[n_paths] = (uint16_t)best; L.plen[n_paths] = len;      // written out below, a lane per path
              n_paths++;
            }
            // the departing edges in edge-id order (first occurrence), those of weight >= min_path_weight
            int ce[5]; uint32_t cf[5]; int nc = 0;
            const unsigned long long nk = L.nkey[node];
            for (int b = 0; b < 5; b++){
              const int e = flk_find(L.ekey, HS_FLK_EDGE_SLOTS, ((nk << 3) | (unsigned long long)b));
              if (e < 0 || !L.ekeep[e]) continue;
              int j = nc;
              while (j > 0 && cf[j-1] > L.efirst[e]){ ce[j] = ce[j-1]; cf[j] = cf[j-1]; j--; }
              ce[j] = e; cf[j] = L.efirst[e]; nc++;
            }
            for (int c = 0; c < nc; c++){
              const int e = ce[c];
              if (L.ew[e] < d.min_path_weight) continue;
              if (n_rec >= caps.max_recs){ flag |= HS_FLK_F_RECS; break; }
              L.rnode[n_rec] = L.edst[e]; L.rparent[n_rec] = (uint16_t)best; L.rw[n_rec] = L.rw[best] < L.ew[e] ? L.rw[best] : L.ew[e];
              L.heap[n_heap] = (uint16_t)n_rec; n_heap++;
              flk_push_heap(L.heap, L.rw, n_heap - 1, 0, (uint16_t)n_rec);
              n_rec++;
            }
          }
          // the pops ran out with work left: the records did (every pop consumes one)
          if (!flag && n_heap > 0 && n_paths < d.max_paths) flag |= HS_FLK_F_RECS;
          flk_max(&L.max_recs_seen, n_rec);
          // the task's piece of the call's pool, taken at once: per path [min_weight][length][bases, padded to 4 bytes]
          if (!flag && n_paths > 0){
            int total = 0;
            for (int p = 0; p < n_paths; p++) total += hs_flk_path_bytes(L.plen[p]);
            const unsigned long long at = flk_add64(d.pool_used, (unsigned long long)total);
            if (at + (unsigned long long)total > (unsigned long long)d.pool_cap) flag |= HS_FLK_F_POOL;
            else L.path_at = (int32_t)at;
          }
          if (flag) flk_or(&L.flag, flag);
          L.n_paths = n_paths; L.result_k = k; L.ok = 1;
        }
      }
      FLK_SYNC();
      // ---- the paths: a lane each (DebruijnPath::get_sequence: the last node's label, then the first base of every ancestor)
      FLK_LANES(lane){
        if (!L.flag && lane < L.n_paths){
          int off = L.path_at;
          for (int p = 0; p < lane; p++) off += hs_flk_path_bytes(L.plen[p]);
          const int best = L.emit[lane], len = L.plen[lane], depth = len - k;
          int32_t* head = (int32_t*)(d.pool + off);
          head[0] = L.rw[best]; head[1] = len;
          char* seq = d.pool + off + 8;
          const unsigned long long nk = L.nkey[L.rnode[best]];
          for (int j = 0; j < k; j++) seq[depth + j] = hs_flk_base((int)((nk >> (3*(k - 1 - j))) & 7ull));
          int at_pos = depth - 1;
          for (int p = L.rparent[best]; p != (int)HS_FLK_NO_REC && at_pos >= 0; p = L.rparent[p], at_pos--)      // at most depth <= caps.max_path_len steps
            seq[at_pos] = hs_flk_base((int)((L.nkey[L.rnode[p]] >> (3*(k - 1))) & 7ull));
        }
      }
      FLK_SYNC();
      break;                                                     // the first acyclic k is the task's
    }
  }
  FLK_SYNC();
  FLK_LANES(lane){
    if (lane == 0){
      d.task_flag[t] = L.flag; d.task_k[t] = L.flag ? -1 : L.result_k; d.task_np[t] = L.flag ? 0 : L.n_paths; d.task_at[t] = L.path_at;
      d.task_size[HS_FLK_SIZES*t + 0] = L.max_edges_seen; d.task_size[HS_FLK_SIZES*t + 1] = L.max_nodes_seen;
      d.task_size[HS_FLK_SIZES*t + 2] = L.max_recs_seen; d.task_size[HS_FLK_SIZES*t + 3] = n_entered;
    }
  }
}
