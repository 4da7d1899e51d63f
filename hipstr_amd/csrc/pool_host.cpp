// pool_host.cpp — host twin of the read pooler (pool.hip) and the assembly of the pooled batch.  Plain C++: no HIP, no device; compiles
// next to a stand-alone program (tests/cpp/pool_host_test.cpp).
//
// Grouping is exact: an unordered map keyed by the reads' bytes (length included), pools numbered as their first reads appear
// (read_pooler.cpp:3-20).  The median of a pool's qualities at a position (base_quality.cpp:11-28: sorted[n / 2], char order = signed) is
// found by counting — the members' bytes, mapped to their rank as signed chars, fall into 256 bins of which only the span between the
// smallest and the largest byte seen is walked and cleared — instead of a sort per position; pools of up to eight members (most pools)
// take the larger of two or a sorting network of eight over whole rows.
#include "pool_host.h"

#include <string.h>
#include <string_view>
#include <unordered_map>

namespace hipstr_pool {

void pool_locus_host(const hipstr_batch_t* b, int l, Sink& s){
  hipstr_pool_out_t* o = s.out;
  const int r0 = b->read_off[l], r1 = b->read_off[l+1], n = r1 - r0;
  o->pool_off[l] = (int32_t)s.pools;
  const int64_t p0 = s.pools;
  if (n > 0){
    std::unordered_map<std::string_view, int32_t> pools;
    pools.reserve((size_t)n*2);
    for (int r = r0; r < r1; r++){
      const std::string_view key(b->bases + b->base_off[r], (size_t)(b->base_off[r+1] - b->base_off[r]));
      auto it = pools.find(key);
      int32_t p;
      if (it == pools.end()){
        p = (int32_t)pools.size();
        pools.emplace(key, p);
        o->pool_rep[p0 + p] = r; o->pool_size[p0 + p] = 0;
      } else p = it->second;
      o->pool_index[r] = p;
      o->pool_size[p0 + p]++;
    }
    const int32_t P = (int32_t)pools.size();
    // the members of every pool, pool after pool, in read order
    std::vector<int32_t> start((size_t)P + 1, 0), members((size_t)n);
    for (int32_t p = 0; p < P; p++) start[p+1] = start[p] + o->pool_size[p0 + p];
    {
      std::vector<int32_t> cur(start.begin(), start.end() - 1);
      for (int r = r0; r < r1; r++) members[cur[o->pool_index[r]]++] = r;
    }
    uint32_t cnt[256];
    memset(cnt, 0, sizeof cnt);
    std::vector<const uint8_t*> mq;
    std::vector<uint8_t> rows;
    for (int32_t p = 0; p < P; p++){
      const int rep = o->pool_rep[p0 + p], len = b->base_off[rep+1] - b->base_off[rep], m = o->pool_size[p0 + p];
      o->pool_qual_off[p0 + p] = (int32_t)s.quals;
      char* dst = o->pool_quals + s.quals;
      s.quals += len;
      if (len == 0) continue;                                  // reads of length 0: one pool, no qualities
      if (m == 1){ memcpy(dst, b->quals + b->base_off[rep], (size_t)len); continue; }
      const int32_t* mem = members.data() + start[p];
      mq.resize((size_t)m);
      for (int k = 0; k < m; k++) mq[k] = (const uint8_t*)b->quals + b->base_off[mem[k]];
      if (m == 2){                                             // sorted[1]: the larger of the two
        for (int i = 0; i < len; i++){ const unsigned x = mq[0][i] ^ 0x80u, y = mq[1][i] ^ 0x80u; dst[i] = (char)(uint8_t)((x > y ? x : y) ^ 0x80u); }
        continue;
      }
      if (m <= 8){
        // a handful of members: the device's sorting network of eight, run on whole rows — a compare-exchange is an element-wise minimum and
        // maximum of two rows of ranks (loops the compiler vectorises); rows past the pool hold the largest rank
        rows.resize((size_t)8*(size_t)len);
        uint8_t* R[8];
        for (int k = 0; k < 8; k++){
          R[k] = rows.data() + (size_t)k*(size_t)len;
          if (k < m) for (int i = 0; i < len; i++) R[k][i] = (uint8_t)(mq[k][i] ^ 0x80u);
          else memset(R[k], 0xFF, (size_t)len);
        }
        static const uint8_t net[19][2] = { {0,1},{2,3},{4,5},{6,7}, {0,2},{1,3},{4,6},{5,7}, {1,2},{5,6}, {0,4},{1,5},{2,6},{3,7}, {2,4},{3,5}, {1,2},{3,4},{5,6} };
        for (int c = 0; c < 19; c++){
          uint8_t* x = R[net[c][0]], *y = R[net[c][1]];
          for (int i = 0; i < len; i++){ const uint8_t lo = x[i] < y[i] ? x[i] : y[i], hi = x[i] < y[i] ? y[i] : x[i]; x[i] = lo; y[i] = hi; }
        }
        const uint8_t* med = R[m/2];
        for (int i = 0; i < len; i++) dst[i] = (char)(uint8_t)(med[i] ^ 0x80u);
        continue;
      }
      const uint32_t need = (uint32_t)(m/2) + 1;               // sorted[m / 2]: the first value with more than m / 2 members at or below it
      for (int i = 0; i < len; i++){
        unsigned lo = 255, hi = 0;
        for (int k = 0; k < m; k++){
          const unsigned v = mq[k][i] ^ 0x80u;                 // rank of the byte among signed chars
          cnt[v]++;
          if (v < lo) lo = v;
          if (v > hi) hi = v;
        }
        unsigned med = hi; uint32_t c = 0;
        for (unsigned v = lo; v <= hi; v++){ c += cnt[v]; if (c >= need){ med = v; break; } }
        for (unsigned v = lo; v <= hi; v++) cnt[v] = 0;
        dst[i] = (char)(uint8_t)(med ^ 0x80u);
      }
    }
    s.pools += P;
  }
  o->n_pools[l] = (int32_t)(s.pools - p0);
  o->pool_off[l+1] = (int32_t)s.pools;
  o->pool_qual_off[s.pools] = (int32_t)s.quals;
}

void pool_reads_host(const hipstr_batch_t* b, hipstr_pool_out_t* out){
  Sink s{out, 0, 0};
  out->pool_off[0] = 0; out->pool_qual_off[0] = 0;
  for (int l = 0; l < b->n_loci; l++) pool_locus_host(b, l, s);
}

hipstr_pooled_batch* assemble_pooled_batch(const hipstr_batch_t* b, const hipstr_pool_out_t* o){
  const int64_t nl = b->n_loci;
  int64_t n_opts = 0;
  for (int64_t i = 0; i < 3*nl; i++) n_opts += b->blk_nopts[i];
  const int64_t n_seq = nl ? b->opt_off[n_opts] : 0, n_haps = nl ? b->hap_off[nl] : 0, n_reads = nl ? b->read_off[nl] : 0;
  const int64_t P = nl ? o->pool_off[nl] : 0;
  int64_t n_bases = 0, n_cig = 0;
  for (int64_t p = 0; p < P; p++){
    const int r = o->pool_rep[p];
    n_bases += b->base_off[r+1] - b->base_off[r]; n_cig += b->cigar_off[r+1] - b->cigar_off[r];
  }
  // one allocation, every section on an 8-byte boundary; the byte arrays end with a NUL of their own
  size_t tot = 0;
  auto take = [&](size_t bytes){ const size_t off = tot; tot = (tot + bytes + 7) & ~(size_t)7; return off; };
  const size_t s_bs = take(12*nl), s_be = take(12*nl), s_bn = take(12*nl), s_per = take(4*nl), s_st = take(48*nl), s_oo = take(4*(n_opts + 1)),
               s_seq = take(n_seq + 1), s_ho = take(4*(nl + 1)), s_rh = take(b->realign_hap ? n_haps : 0), s_ro = take(4*(nl + 1)),
               s_bo = take(4*(P + 1)), s_b = take(n_bases + 1), s_q = take(n_bases + 1), s_rs = take(4*P), s_co = take(4*(P + 1)),
               s_cop = take(n_cig + 1), s_cl = take(4*(n_cig + 1)), s_pi = take(4*(n_reads + 1));
  hipstr_pooled_batch* pb = new hipstr_pooled_batch();
  pb->mem.assign(tot + 8, 0);
  uint8_t* m = pb->mem.data();
  auto copy = [&](size_t off, const void* src, size_t bytes){ if (bytes && src) memcpy(m + off, src, bytes); };
  if (nl){
    copy(s_bs, b->blk_start, 12*nl); copy(s_be, b->blk_end, 12*nl); copy(s_bn, b->blk_nopts, 12*nl); copy(s_per, b->period, 4*nl);
    copy(s_st, b->stutter, 48*nl); copy(s_oo, b->opt_off, 4*(n_opts + 1)); copy(s_seq, b->seq, n_seq); copy(s_ho, b->hap_off, 4*(nl + 1));
    copy(s_rh, b->realign_hap, n_haps); copy(s_ro, o->pool_off, 4*(nl + 1)); copy(s_pi, o->pool_index, 4*n_reads);
  }
  int32_t* bo = (int32_t*)(m + s_bo), *co = (int32_t*)(m + s_co), *rs = (int32_t*)(m + s_rs), *cl = (int32_t*)(m + s_cl);
  char* bases = (char*)(m + s_b), *quals = (char*)(m + s_q), *cop = (char*)(m + s_cop);
  int64_t nb = 0, nc = 0;
  for (int64_t p = 0; p < P; p++){
    const int r = o->pool_rep[p];
    const int len = b->base_off[r+1] - b->base_off[r], cig = b->cigar_off[r+1] - b->cigar_off[r];
    bo[p] = (int32_t)nb; co[p] = (int32_t)nc; rs[p] = b->read_start[r];
    if (len){ memcpy(bases + nb, b->bases + b->base_off[r], (size_t)len); memcpy(quals + nb, o->pool_quals + o->pool_qual_off[p], (size_t)len); }
    if (cig){ memcpy(cop + nc, b->cigar_op + b->cigar_off[r], (size_t)cig); memcpy(cl + nc, b->cigar_len + b->cigar_off[r], 4*(size_t)cig); }
    nb += len; nc += cig;
  }
  bo[P] = (int32_t)nb; co[P] = (int32_t)nc;
  hipstr_batch_t& q = pb->batch;
  memset(&q, 0, sizeof q);
  q.n_loci = (int32_t)nl;
  q.blk_start = (const int32_t*)(m + s_bs); q.blk_end = (const int32_t*)(m + s_be); q.blk_nopts = (const int32_t*)(m + s_bn);
  q.period = (const int32_t*)(m + s_per); q.stutter = (const double*)(m + s_st); q.opt_off = (const int32_t*)(m + s_oo);
  q.seq = (const char*)(m + s_seq); q.hap_off = (const int32_t*)(m + s_ho);
  q.realign_hap = b->realign_hap ? (const uint8_t*)(m + s_rh) : NULL;
  q.read_off = (const int32_t*)(m + s_ro); q.base_off = bo; q.bases = bases; q.quals = quals; q.read_start = rs; q.cigar_off = co;
  q.cigar_op = cop; q.cigar_len = cl; q.realign_read = NULL;
  pb->pool_index = (const int32_t*)(m + s_pi);
  return pb;
}

}  // namespace hipstr_pool
