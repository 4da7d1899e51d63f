// pool.hip — ReadPooler on gfx950: the pools of a batch of un-pooled reads (read_pooler.cpp:3-20) and the median base qualities of their
// members (base_quality.cpp:11-28), in front of hipstr_hmm_upload.  Equality of byte strings and an order statistic of bytes: no arithmetic,
// so device and host twin (pool_host.cpp) agree bit for bit.
//
//   hs_pool_hash_kernel    a wavefront per read: 16 bytes per lane and step, a 64-bit hash of bases and length, summed over the lanes
//   hs_pool_group_kernel   a workgroup per locus: the reads' hashes go into an open-addressing table in LDS (64-bit compare-and-swap claims a
//                          slot, an integer minimum leaves the slot's lowest read index: the pool's first read, whatever order the atomics
//                          arrive in); a workgroup scan over the leader flags in read order numbers the pools; every member is compared with
//                          its leader byte for byte (a wavefront per read, 16 bytes per lane) — a difference raises the locus' collision flag;
//                          then the pools' sizes, the members of every pool (a counting sort; the order inside a pool changes no output) and
//                          the offsets of the pools' qualities within the locus
//   hs_pool_scan_kernel    one workgroup: the loci's pool counts and quality bytes into pool_off / qual_base
//   hs_pool_median_kernel  a wavefront per pool, lanes are positions (a member's bytes are consecutive addresses across the lanes): a copy for
//                          one member, a sorting network in registers up to HS_POOL_NET, a bitwise radix select beyond
// No kernel waits on memory and no workgroup talks to another; every word a kernel reads was written by the same call (the upload, or a
// kernel before it on the stream).  Correctness never rests on the hash: a locus with its collision flag up, and a locus of more than
// HS_POOL_LDS_READS reads, is pooled by the host twin inside the same call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/hipstr_hmm.h"
#include "../../include/hipstr_hmm_debug.h"
#include "api_internal.h"
#include "pool_host.h"
#include "pool_layout.h"
#include "prep.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ int pool_wave_incl_scan(int v, int lane){
  for (int dlt = 1; dlt < 64; dlt <<= 1){ const int o = __shfl_up(v, dlt); if (lane >= dlt) v += o; }
  return v;
}
// exclusive prefix of the workgroup's HS_POOL_THREADS values in thread order; total = their sum.  part: four dwords of LDS.  Every thread
// of the workgroup calls it (two barriers; the first ends the previous use of part).
__device__ __forceinline__ int pool_wg_excl_scan(int v, int32_t* part, int& total){
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = pool_wave_incl_scan(v, lane);
  __syncthreads();
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < HS_POOL_THREADS/64; w++){ const int pw = part[w]; tot += pw; if (w < wave) base += pw; }
  total = tot;
  return base + incl - v;
}

extern "C" __global__ void __launch_bounds__(HS_POOL_THREADS) hs_pool_hash_kernel(const hs_pool_dev_t d){
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x*(HS_POOL_THREADS/64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (r >= d.n) return;
  const int len = d.len[r];
  const uint4* p = (const uint4*)(d.bases + d.doff[r]);       // 16-byte aligned; the read's last piece is padded with zeros
  unsigned long long sum = 0;
  for (int piece = lane; piece*HS_POOL_HASH_STEP < len; piece += 64){
    const uint4 v = p[piece];
    sum += hs_pool_hash_piece(((uint64_t)v.y << 32) | v.x, ((uint64_t)v.w << 32) | v.z, (uint64_t)piece);
  }
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
  if (lane == 0) d.hash[r] = hs_pool_hash_finish(sum, len, d.hash_bits);
}

extern __shared__ uint64_t hs_pool_lds[];

extern "C" __global__ void __launch_bounds__(HS_POOL_THREADS) hs_pool_group_kernel(const hs_pool_dev_t d){
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int l = blockIdx.x;
  const int r0 = d.lread_off[l], n = d.lread_off[l+1] - r0;
  if (n <= 0){                                    // no reads, or a locus the host pools
    if (t == 0){ d.n_pools[l] = 0; d.qbytes[l] = 0; d.collision[l] = 0; }
    return;
  }
  const int slots = hs_pool_table_slots(n);
  uint64_t* keys = hs_pool_lds;                   // [slots]
  int32_t* lead = (int32_t*)(keys + slots);       // [slots] lowest read index of the slot's key
  int32_t* rslot = lead + slots;                  // [n] slot of the read; from phase 6 on its pool
  int32_t* part = rslot + n;                      // [4] scan partials; part[8]: the collision flag
  // once the table is built the keys' bytes (16 n at least) hold four dwords per read
  int32_t* psize = (int32_t*)keys, *pstart = psize + n, *pcur = pstart + n, *pnum = pcur + n;

  // ---- 1: an empty table
  for (int i = t; i < slots; i += HS_POOL_THREADS){ keys[i] = HS_POOL_EMPTY_KEY; lead[i] = INT32_MAX; }
  if (t == 0) part[8] = 0;
  __syncthreads();
  // ---- 2: every read finds or claims the slot of its hash (at most half the slots are ever taken: the probe ends)
  for (int r = t; r < n; r += HS_POOL_THREADS){
    const uint64_t h = d.hash[r0 + r];
    int s = (int)(h & (uint64_t)(slots - 1));
    for (;;){
      const unsigned long long prev = atomicCAS((unsigned long long*)&keys[s], (unsigned long long)HS_POOL_EMPTY_KEY, (unsigned long long)h);
      if (prev == HS_POOL_EMPTY_KEY || prev == h) break;
      s = (s + 1) & (slots - 1);
    }
    atomicMin(&lead[s], r);
    rslot[r] = s;
  }
  __syncthreads();
  // ---- 3: the keys are dead
  for (int i = t; i < n; i += HS_POOL_THREADS) psize[i] = 0;
  __syncthreads();
  // ---- 4: pools are numbered as their first reads appear: a scan over the leader flags in read order
  int P = 0;
  for (int base = 0; base < n; base += HS_POOL_THREADS){
    const int r = base + t;
    const int flag = (r < n && lead[rslot[r]] == r) ? 1 : 0;
    int tot;
    const int ex = pool_wg_excl_scan(flag, part, tot);
    if (flag){ pnum[r] = P + ex; pcur[P + ex] = r; }      // (pcur: the pool's first read until phase 7 has taken it)
    P += tot;
  }
  __syncthreads();
  // ---- 5: a wavefront per read: the member against its leader, byte for byte
  for (int r = wave; r < n; r += HS_POOL_THREADS/64){
    const int L = lead[rslot[r]];
    if (L == r) continue;
    const int len = d.len[r0 + r];
    bool diff = len != d.len[r0 + L];
    if (!diff){
      const uint4* a = (const uint4*)(d.bases + d.doff[r0 + r]);
      const uint4* b = (const uint4*)(d.bases + d.doff[r0 + L]);
      for (int piece = lane; piece*HS_POOL_HASH_STEP < len; piece += 64){
        const uint4 x = a[piece], y = b[piece];
        diff = diff || ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0;
      }
    }
    if (__ballot(diff) != 0 && lane == 0) part[8] = 1;
  }
  __syncthreads();
  // ---- 6: pool of every read, members per pool
  for (int r = t; r < n; r += HS_POOL_THREADS){
    const int p = pnum[lead[rslot[r]]];
    rslot[r] = p;
    d.pool_index[r0 + r] = p;
    atomicAdd(&psize[p], 1);
  }
  __syncthreads();
  // ---- 7: where the pools' members and qualities start
  int m_sum = 0, q_sum = 0;
  for (int base = 0; base < P; base += HS_POOL_THREADS){
    const int p = base + t;
    const int sz = p < P ? psize[p] : 0, rep = p < P ? pcur[p] : 0;
    const int ln = p < P ? d.len[r0 + rep] : 0;
    int tot_m, tot_q;
    const int em = pool_wg_excl_scan(sz, part, tot_m);
    const int eq = pool_wg_excl_scan(ln, part, tot_q);
    if (p < P){
      pstart[p] = m_sum + em; pcur[p] = 0;
      d.p_rep[r0 + p] = r0 + rep; d.p_size[r0 + p] = sz; d.p_qoff[r0 + p] = q_sum + eq; d.p_moff[r0 + p] = r0 + m_sum + em;
    }
    m_sum += tot_m; q_sum += tot_q;
  }
  for (int p = P + t; p < n; p += HS_POOL_THREADS) d.p_size[r0 + p] = 0;
  for (int p = t; p < n; p += HS_POOL_THREADS) d.slot_locus[r0 + p] = l;
  if (t == 0){ d.n_pools[l] = P; d.qbytes[l] = q_sum; d.collision[l] = part[8]; }
  __syncthreads();
  // ---- 8: the members of every pool
  for (int r = t; r < n; r += HS_POOL_THREADS){
    const int p = rslot[r];
    const int k = atomicAdd(&pcur[p], 1);
    d.members[r0 + pstart[p] + k] = r0 + r;
  }
}

extern "C" __global__ void __launch_bounds__(HS_POOL_THREADS) hs_pool_scan_kernel(const hs_pool_dev_t d){
  __shared__ int32_t part[4];
  const int t = threadIdx.x;
  int p_sum = 0, q_sum = 0;
  for (int base = 0; base < d.nl; base += HS_POOL_THREADS){
    const int l = base + t;
    const int np = l < d.nl ? d.n_pools[l] : 0, qb = l < d.nl ? d.qbytes[l] : 0;
    int tot_p, tot_q;
    const int ep = pool_wg_excl_scan(np, part, tot_p);
    const int eq = pool_wg_excl_scan(qb, part, tot_q);
    if (l < d.nl){ d.pool_off[l] = p_sum + ep; d.qual_base[l] = q_sum + eq; }
    p_sum += tot_p; q_sum += tot_q;
  }
  if (t == 0){ d.pool_off[d.nl] = p_sum; d.qual_base[d.nl] = q_sum; }
}

#define HS_POOL_CX(a, b) { const unsigned lo_ = min(v[a], v[b]), hi_ = max(v[a], v[b]); v[a] = lo_; v[b] = hi_; }

extern "C" __global__ void __launch_bounds__(HS_POOL_THREADS) hs_pool_median_kernel(const hs_pool_dev_t d){
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x*(HS_POOL_THREADS/64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // slot
  if (i >= d.n) return;
  const int sz = d.p_size[i];
  if (sz == 0) return;
  const int l = d.slot_locus[i];
  if (d.collision[l]) return;                     // the host redoes the locus (members of a pool may differ in length here)
  const int g = d.pool_off[l] + (i - d.lread_off[l]);
  const int rep = d.p_rep[i], len = d.len[rep];
  const int qo = d.qual_base[l] + d.p_qoff[i];
  if (lane == 0){ d.out_rep[g] = rep; d.out_size[g] = sz; d.out_qoff[g] = qo; }
  const int32_t* mem = d.members + d.p_moff[i];
  const int k = sz/2;
  const int route = hs_pool_median_route(sz);
  for (int pos = lane; pos < len; pos += 64){
    unsigned q;
    if (route == HS_POOL_ROUTE_COPY) q = (uint8_t)d.quals[d.doff[rep] + pos];
    else if (route == HS_POOL_ROUTE_NET){
      // bytes as their rank among signed chars; the slots past the pool hold the largest rank, which sorts behind every member
      unsigned v[HS_POOL_NET];
#pragma unroll
      for (int m = 0; m < HS_POOL_NET; m++) v[m] = m < sz ? ((uint8_t)d.quals[d.doff[mem[m]] + pos] ^ 0x80u) : 0xFFu;
      // Batcher's odd-even merge sort of eight: nineteen compare-exchanges
      HS_POOL_CX(0, 1) HS_POOL_CX(2, 3) HS_POOL_CX(4, 5) HS_POOL_CX(6, 7)
      HS_POOL_CX(0, 2) HS_POOL_CX(1, 3) HS_POOL_CX(4, 6) HS_POOL_CX(5, 7)
      HS_POOL_CX(1, 2) HS_POOL_CX(5, 6)
      HS_POOL_CX(0, 4) HS_POOL_CX(1, 5) HS_POOL_CX(2, 6) HS_POOL_CX(3, 7)
      HS_POOL_CX(2, 4) HS_POOL_CX(3, 5)
      HS_POOL_CX(1, 2) HS_POOL_CX(3, 4) HS_POOL_CX(5, 6)
      unsigned s = v[1];                          // sz >= 2: k = 1 .. 4
      s = k == 2 ? v[2] : s; s = k == 3 ? v[3] : s; s = k == 4 ? v[4] : s;
      q = s ^ 0x80u;
    } else {
      // the k-th smallest rank, bit by bit from the top: members that share the bits found so far and have a 0 next
      unsigned prefix = 0; int kk = k;
      for (int bit = 7; bit >= 0; bit--){
        const unsigned hi_mask = (0xFFu << (bit + 1)) & 0xFFu;
        int zeros = 0;
        for (int m = 0; m < sz; m++){
          const unsigned key = (uint8_t)d.quals[d.doff[mem[m]] + pos] ^ 0x80u;
          zeros += ((key & hi_mask) == prefix && !((key >> bit) & 1u)) ? 1 : 0;
        }
        if (kk >= zeros){ kk -= zeros; prefix |= 1u << bit; }
      }
      q = prefix ^ 0x80u;
    }
    d.out_quals[qo + pos] = (char)(uint8_t)q;
  }
}
static_assert(HS_POOL_NET == 8, "the sorting network of hs_pool_median_kernel is written for eight");

// ------------------------------------------------------------------------------------------------------------------------ host side
using hipstr::api_fail;

thread_local hipstr::ChunkLast t_last;

int64_t pool_ws_bytes(double ws_mib){ return hipstr::chunk_budget(ws_mib, "HIPSTR_POOL_WS_MIB", (double)HS_POOL_WS_MIB, (double)HS_POOL_MAX_LOCUS_BYTES); }

// per locus: the route (1 = device) and the workspace it takes
void pool_costs(const hipstr_batch_t* b, std::vector<uint8_t>& dev, std::vector<int64_t>& cost){
  const int nl = b->n_loci;
  dev.assign((size_t)nl, 0); cost.assign((size_t)nl, 0);
  for (int l = 0; l < nl; l++){
    int64_t padded = 0, bytes = 0;
    for (int r = b->read_off[l]; r < b->read_off[l+1]; r++){
      const int64_t len = b->base_off[r+1] - b->base_off[r];
      padded += hs_pool_pad(len); bytes += hs_pool_read_bytes(len);
    }
    dev[l] = hs_pool_on_device(b->read_off[l+1] - b->read_off[l], padded) ? 1 : 0;
    cost[l] = HS_POOL_LOCUS_FIXED + (dev[l] ? bytes : 0);
  }
}

int pool_check(const hipstr_batch_t* b, const hipstr_pool_out_t* out, const char* who){
  if (!b || !out) return api_fail(std::string(who) + ": null argument");
  { std::string bad; if (hipstr::validate_tables(b, bad)) return api_fail(std::string(who) + ": " + bad); }
  if (!out->pool_index || !out->n_pools || !out->pool_off || !out->pool_rep || !out->pool_size || !out->pool_qual_off || !out->pool_quals)
    return api_fail(std::string(who) + ": null output array");
  return 0;
}

int pool_reads_device(const hipstr_batch_t* b, hipstr_pool_out_t* out){
  const int nl = b->n_loci;
  hipstr::Ctx* ctx = hipstr::api_current_ctx();
  if (!ctx) return 1;
  if (hipstr::api_bind(ctx)) return 1;
  hipStream_t st = hipstr::ctx_stream(ctx);
  hipstr::ChunkLast last;
  t_last = last;                                  // a call that fails on the way reports zeros, not the call before it
  int hash_bits = 64;
  if (const char* e = getenv("HIPSTR_DEBUG_POOL_HASH_BITS")){ const int v = atoi(e); if (v >= 1 && v < 64) hash_bits = v; }
  const bool timing = getenv("HIPSTR_POOL_TIMING") != NULL;
  const int64_t budget = pool_ws_bytes(0.0);
  std::vector<uint8_t> dev; std::vector<int64_t> cost;
  pool_costs(b, dev, cost);
  hipstr_pool::Sink sink{out, 0, 0};
  std::vector<int32_t> lread;
  // (nothing is written before the first chunk has come home; a failure of the device in a later chunk leaves the loci of the chunks
  // before it written, as include/hipstr_hmm.h says)
  for (int l0 = 0; l0 < nl; ){
    const int l1 = hs_pool_chunk_end(cost.data(), l0, nl, budget), nlc = l1 - l0;
    lread.assign((size_t)nlc + 1, 0);
    int64_t n64 = 0, B = 0, Bq = 0; int max_reads = 0;
    for (int l = l0; l < l1; l++){
      if (dev[l]){
        const int nr = b->read_off[l+1] - b->read_off[l];
        for (int r = b->read_off[l]; r < b->read_off[l+1]; r++){ const int64_t len = b->base_off[r+1] - b->base_off[r]; B += hs_pool_pad(len); Bq += len; }
        n64 += nr; max_reads = std::max(max_reads, nr);
      }
      lread[(size_t)(l - l0) + 1] = (int32_t)n64;
    }
    if (B > INT32_MAX || n64 > INT32_MAX) return api_fail("hipstr_pool_reads: a chunk of more than 2^31 bytes (lower HIPSTR_POOL_WS_MIB)");
    const size_t n = (size_t)n64;
    hipstr::ChunkBlocks K(ctx, st);
    const int32_t* r_pi = NULL, *r_np = NULL, *r_coll = NULL, *r_po = NULL, *r_qb = NULL, *r_rep = NULL, *r_size = NULL, *r_qoff = NULL; const char* r_quals = NULL;
    if (n > 0){
      last.v[6]++; last.v[7] += (int64_t)n;
      // uploaded | workspace | results
      const size_t u_len = K.take(n*4), u_doff = K.take(n*4), u_lro = K.take(((size_t)nlc + 1)*4), u_bases = K.take((size_t)B), u_quals = K.take((size_t)B);
      K.end_upload();
      const size_t w_hash = K.take(n*8), w_mem = K.take(n*4), w_rep = K.take(n*4), w_size = K.take(n*4), w_qoff = K.take(n*4), w_moff = K.take(n*4),
                   w_sl = K.take(n*4), w_qbytes = K.take((size_t)nlc*4);
      K.begin_results();
      const size_t o_pi = K.take(n*4), o_np = K.take((size_t)nlc*4), o_coll = K.take((size_t)nlc*4), o_po = K.take(((size_t)nlc + 1)*4),
                   o_qb = K.take(((size_t)nlc + 1)*4), o_rep = K.take(n*4), o_size = K.take(n*4), o_qoff = K.take(n*4), o_quals = K.take((size_t)Bq);
      if (K.reserve()) return 1;
      // the reads, every one on a 16-byte boundary, the last piece of its bases filled up with zeros
      const auto t0 = std::chrono::steady_clock::now();
      {
        int32_t* len_h = K.up<int32_t>(u_len), *doff_h = K.up<int32_t>(u_doff);
        memcpy(K.up<char>(u_lro), lread.data(), ((size_t)nlc + 1)*4);
        char* bases_h = K.up<char>(u_bases), *quals_h = K.up<char>(u_quals);
        size_t i = 0; int64_t off = 0;
        for (int l = l0; l < l1; l++){
          if (!dev[l]) continue;
          for (int r = b->read_off[l]; r < b->read_off[l+1]; r++, i++){
            const int64_t src = b->base_off[r], len = b->base_off[r+1] - src, pad = hs_pool_pad(len);
            len_h[i] = (int32_t)len; doff_h[i] = (int32_t)off;
            if (len){ memcpy(bases_h + off, b->bases + src, (size_t)len); memcpy(quals_h + off, b->quals + src, (size_t)len); }
            if (pad > len) memset(bases_h + off + len, 0, (size_t)(pad - len));
            off += pad;
          }
        }
      }
      last.t[3] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      hs_pool_dev_t d; memset(&d, 0, sizeof d);
      char* D = K.dev;
      d.len = (const int32_t*)(D + u_len); d.doff = (const int32_t*)(D + u_doff); d.lread_off = (const int32_t*)(D + u_lro);
      d.bases = D + u_bases; d.quals = D + u_quals;
      d.hash = (uint64_t*)(D + w_hash); d.members = (int32_t*)(D + w_mem); d.p_rep = (int32_t*)(D + w_rep); d.p_size = (int32_t*)(D + w_size);
      d.p_qoff = (int32_t*)(D + w_qoff); d.p_moff = (int32_t*)(D + w_moff); d.slot_locus = (int32_t*)(D + w_sl); d.qbytes = (int32_t*)(D + w_qbytes);
      d.pool_index = (int32_t*)(D + o_pi); d.n_pools = (int32_t*)(D + o_np); d.collision = (int32_t*)(D + o_coll); d.pool_off = (int32_t*)(D + o_po);
      d.qual_base = (int32_t*)(D + o_qb); d.out_rep = (int32_t*)(D + o_rep); d.out_size = (int32_t*)(D + o_size); d.out_qoff = (int32_t*)(D + o_qoff);
      d.out_quals = D + o_quals;
      d.n = (int32_t)n; d.nl = nlc; d.hash_bits = hash_bits;
      const size_t lds = hs_pool_lds_bytes(max_reads);
      // (the largest size there is, the same in every call: calls of several threads cannot lower it under one another's launch)
      HS_HIP(hipFuncSetAttribute((const void*)hs_pool_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hs_pool_lds_bytes(HS_POOL_LDS_READS)));
      if (K.upload(timing)) return 1;
      const unsigned per_wave = (unsigned)((n + HS_POOL_THREADS/64 - 1)/(HS_POOL_THREADS/64));
      hipLaunchKernelGGL(hs_pool_hash_kernel, dim3(per_wave), dim3(HS_POOL_THREADS), 0, st, d);
      hipLaunchKernelGGL(hs_pool_group_kernel, dim3((unsigned)nlc), dim3(HS_POOL_THREADS), lds, st, d);
      hipLaunchKernelGGL(hs_pool_scan_kernel, dim3(1), dim3(HS_POOL_THREADS), 0, st, d);
      hipLaunchKernelGGL(hs_pool_median_kernel, dim3(per_wave), dim3(HS_POOL_THREADS), 0, st, d);
      HS_HIP(hipGetLastError());
      if (K.fetch(timing, &last.t[0])) return 1;
      last.t[1] += (double)K.up_bytes; last.t[2] += (double)K.res_bytes();
      r_pi = K.host<int32_t>(o_pi); r_np = K.host<int32_t>(o_np); r_coll = K.host<int32_t>(o_coll); r_po = K.host<int32_t>(o_po);
      r_qb = K.host<int32_t>(o_qb); r_rep = K.host<int32_t>(o_rep); r_size = K.host<int32_t>(o_size); r_qoff = K.host<int32_t>(o_qoff);
      r_quals = K.host<char>(o_quals);
    }
    if (l0 == 0){ out->pool_off[0] = 0; out->pool_qual_off[0] = 0; }
    for (int l = l0; l < l1; l++){
      const int lc = l - l0, nr = b->read_off[l+1] - b->read_off[l];
      if (!dev[l]){ last.v[1]++; hipstr_pool::pool_locus_host(b, l, sink); continue; }
      if (nr == 0){ last.v[0]++; hipstr_pool::pool_locus_host(b, l, sink); continue; }
      if (r_coll[lc]){ last.v[2]++; hipstr_pool::pool_locus_host(b, l, sink); continue; }
      last.v[0]++;
      const int P = r_np[lc], g0 = r_po[lc], q0 = r_qb[lc], qn = r_qb[lc+1] - q0, cr0 = lread[lc], rbase = b->read_off[l];
      out->pool_off[l] = (int32_t)sink.pools;
      memcpy(out->pool_index + rbase, r_pi + cr0, (size_t)nr*4);
      for (int p = 0; p < P; p++){
        const int64_t g = sink.pools + p;
        out->pool_rep[g] = r_rep[g0 + p] - cr0 + rbase;
        out->pool_size[g] = r_size[g0 + p];
        out->pool_qual_off[g] = (int32_t)(r_qoff[g0 + p] - q0 + sink.quals);
        last.v[3 + hs_pool_median_route(r_size[g0 + p])]++;
      }
      if (qn) memcpy(out->pool_quals + sink.quals, r_quals + q0, (size_t)qn);
      sink.pools += P; sink.quals += qn;
      out->n_pools[l] = P; out->pool_off[l+1] = (int32_t)sink.pools; out->pool_qual_off[sink.pools] = (int32_t)sink.quals;
    }
    l0 = l1;
  }
  if (nl == 0){ out->pool_off[0] = 0; out->pool_qual_off[0] = 0; }
  t_last = last;
  return 0;
}

// room for every output of a batch's pooling
struct PoolArrays {
  std::vector<int32_t> pool_index, n_pools, pool_off, pool_rep, pool_size, pool_qual_off; std::vector<char> quals;
  hipstr_pool_out_t out;
  explicit PoolArrays(const hipstr_batch_t* b){
    const size_t nl = (size_t)b->n_loci, n = nl ? (size_t)b->read_off[nl] : 0, nb = n ? (size_t)b->base_off[n] : 0;
    pool_index.assign(n + 1, 0); n_pools.assign(nl + 1, 0); pool_off.assign(nl + 1, 0); pool_rep.assign(n + 1, 0); pool_size.assign(n + 1, 0);
    pool_qual_off.assign(n + 1, 0); quals.assign(nb + 1, 0);
    out.pool_index = pool_index.data(); out.n_pools = n_pools.data(); out.pool_off = pool_off.data(); out.pool_rep = pool_rep.data();
    out.pool_size = pool_size.data(); out.pool_qual_off = pool_qual_off.data(); out.pool_quals = quals.data();
  }
};

void json_ints(std::string& s, const char* name, const int64_t* v, int n){
  s += "\""; s += name; s += "\": [";
  for (int i = 0; i < n; i++){ if (i) s += ", "; s += std::to_string(v[i]); }
  s += "]";
}

}  // namespace

extern "C" int hipstr_pool_reads_host(const hipstr_batch_t* b, hipstr_pool_out_t* out){
  if (pool_check(b, out, "hipstr_pool_reads_host")) return 1;
  hipstr_pool::pool_reads_host(b, out);
  return 0;
}

extern "C" int hipstr_pool_reads(const hipstr_batch_t* b, hipstr_pool_out_t* out){
  if (pool_check(b, out, "hipstr_pool_reads")) return 1;
  return pool_reads_device(b, out);
}

extern "C" hipstr_pooled_batch_t* hipstr_pool_batch(const hipstr_batch_t* b, uint32_t flags){
  if (!b){ api_fail("hipstr_pool_batch: null argument"); return NULL; }
  if (flags & ~(uint32_t)HIPSTR_POOL_ON_HOST){ api_fail("hipstr_pool_batch: unknown flag"); return NULL; }
  { std::string bad; if (hipstr::validate_tables(b, bad)){ api_fail("hipstr_pool_batch: " + bad); return NULL; } }
  PoolArrays A(b);
  if (flags & HIPSTR_POOL_ON_HOST) hipstr_pool::pool_reads_host(b, &A.out);
  else if (pool_reads_device(b, &A.out)) return NULL;
  return hipstr_pool::assemble_pooled_batch(b, &A.out);
}
extern "C" const hipstr_batch_t* hipstr_pooled_batch_batch(const hipstr_pooled_batch_t* p){ return p ? &p->batch : NULL; }
extern "C" const int32_t* hipstr_pooled_batch_pool_index(const hipstr_pooled_batch_t* p){ return p ? p->pool_index : NULL; }
extern "C" void hipstr_pooled_batch_free(hipstr_pooled_batch_t* p){ delete p; }

#ifndef HIPSTR_NO_DEBUG_ABI
extern "C" int hipstr_debug_pool_last(int64_t out[8]){
  if (!out) return api_fail("hipstr_debug_pool_last: null argument");
  memcpy(out, t_last.v, sizeof t_last.v);
  return 0;
}
extern "C" int hipstr_debug_pool_last_timing(double out[4]){
  if (!out) return api_fail("hipstr_debug_pool_last_timing: null argument");
  memcpy(out, t_last.t, sizeof t_last.t);
  return 0;
}

extern "C" int hipstr_debug_pool_plan(const hipstr_batch_t* b, double ws_mib, char* json, int cap){
  if (!b){ api_fail("hipstr_debug_pool_plan: null argument"); return -1; }
  { std::string bad; if (hipstr::validate_tables(b, bad)){ api_fail("hipstr_debug_pool_plan: " + bad); return -1; } }
  const int nl = b->n_loci;
  const int64_t budget = pool_ws_bytes(ws_mib);
  std::vector<uint8_t> dev; std::vector<int64_t> cost;
  pool_costs(b, dev, cost);
  PoolArrays A(b);
  hipstr_pool::pool_reads_host(b, &A.out);
  static const char* route_names[5] = { "device", "host", "copy", "net", "radix" };
  std::string s = "{\"thresholds\": {";
  const std::pair<const char*, int64_t> th[] = {
    {"HS_POOL_THREADS", HS_POOL_THREADS}, {"HS_POOL_LDS_READS", HS_POOL_LDS_READS}, {"HS_POOL_NET", HS_POOL_NET}, {"HS_POOL_HASH_STEP", HS_POOL_HASH_STEP},
    {"HS_POOL_ALIGN", HS_POOL_ALIGN}, {"HS_POOL_MIN_SLOTS", HS_POOL_MIN_SLOTS}, {"HS_POOL_WS_MIB", HS_POOL_WS_MIB}, {"HS_POOL_READ_FIXED", HS_POOL_READ_FIXED},
    {"HS_POOL_LOCUS_FIXED", HS_POOL_LOCUS_FIXED}, {"HS_POOL_MAX_LOCUS_BYTES", HS_POOL_MAX_LOCUS_BYTES} };
  for (size_t i = 0; i < sizeof th/sizeof th[0]; i++){ if (i) s += ", "; s += std::string("\"") + th[i].first + "\": " + std::to_string(th[i].second); }
  s += "}, \"budget_bytes\": " + std::to_string(budget) + ", \"routes\": [";
  for (int i = 0; i < 5; i++){ if (i) s += ", "; s += std::string("\"") + route_names[i] + "\""; }
  s += "], \"chunks\": [";
  bool hit[5] = { false, false, false, false, false };
  for (int l0 = 0; l0 < nl; ){
    const int l1 = hs_pool_chunk_end(cost.data(), l0, nl, budget);
    int64_t reads = 0, bytes = 0, nd = 0, nh = 0, steps = 0, pools[3] = { 0, 0, 0 }; int max_reads = 0;
    for (int l = l0; l < l1; l++){
      bytes += cost[l];
      if (!dev[l]){ nh++; hit[1] = true; continue; }
      nd++; hit[0] = true;
      const int nr = b->read_off[l+1] - b->read_off[l];
      reads += nr; max_reads = std::max(max_reads, nr);
      for (int r = b->read_off[l]; r < b->read_off[l+1]; r++) steps = std::max<int64_t>(steps, hs_pool_hash_steps(b->base_off[r+1] - b->base_off[r]));
      for (int p = A.pool_off[l]; p < A.pool_off[l+1]; p++){ const int rt = hs_pool_median_route(A.pool_size[p]); pools[rt]++; hit[2 + rt] = true; }
    }
    if (l0) s += ", ";
    s += "{\"l0\": " + std::to_string(l0) + ", \"l1\": " + std::to_string(l1) + ", \"reads\": " + std::to_string(reads) + ", \"bytes\": " + std::to_string(bytes) +
         ", \"device_loci\": " + std::to_string(nd) + ", \"host_loci\": " + std::to_string(nh) + ", \"lds_bytes\": " + std::to_string(reads ? (int64_t)hs_pool_lds_bytes(max_reads) : 0) +
         ", \"hash_steps\": " + std::to_string(steps) + ", ";
    json_ints(s, "pools", pools, 3);
    s += "}";
    l0 = l1;
  }
  s += "], \"routes_hit\": [";
  { bool first = true; for (int i = 0; i < 5; i++) if (hit[i]){ if (!first) s += ", "; first = false; s += std::string("\"") + route_names[i] + "\""; } }
  s += "]}";
  if (json && cap > 0){ const size_t k = std::min((size_t)cap - 1, s.size()); memcpy(json, s.data(), k); json[k] = 0; }
  return (int)s.size();
}
#endif  // HIPSTR_NO_DEBUG_ABI
