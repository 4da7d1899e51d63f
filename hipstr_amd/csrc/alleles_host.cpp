// alleles_host.cpp — the host form of the allele-set update between two genotype() rounds (include/hipstr_hmm.h: hipstr_alleles_apply_host,
// hipstr_alleles_step): add_and_remove_alleles (seq_stutter_genotyper.cpp:330-369) and the policy of genotype() around it (:570-601,
// :647-663) for a batch of loci.  Plain C++.  The table, the hash and the byte comparison are those of the device form (alleles_layout.h),
// walked by one thread: the same bytes come out.
#include "alleles_host.h"

#include <limits.h>
#include <string.h>

#include <algorithm>

#include "alleles_layout.h"

namespace hipstr_al {

namespace {

int fail(std::string& err, const std::string& what){ err = what; return 1; }
std::string at(const char* what, int l, int blk = -1){ return std::string(what) + " (locus " + std::to_string(l) + (blk >= 0 ? ", block " + std::to_string(blk) : "") + ")"; }

// an option's (hash, B^length) from its bytes
void option_hash(const char* p, int len, uint64_t* h, uint64_t* pw){
  uint64_t x = 0, w = 1;
  for (int i = 0; i < len; i++){ x = hs_alleles_hash_step(x, p[i]); w *= HS_ALLELES_BASE; }
  *h = x; *pw = w;
}

// one side (old or new) of a locus: its option counts, where block b's options start, and per option bytes, length, hash, B^length
struct Side {
  int n[3], first[3];
  std::vector<const char*> p; std::vector<int32_t> len; std::vector<uint64_t> h, pw;
  void init(const int32_t* nopts, const int32_t* opt_off, const char* seq){
    first[0] = 0; for (int k = 0; k < 3; k++){ n[k] = nopts[k]; if (k) first[k] = first[k-1] + n[k-1]; }
    const int no = n[0] + n[1] + n[2];
    p.resize((size_t)no); len.resize((size_t)no); h.resize((size_t)no); pw.resize((size_t)no);
    for (int o = 0; o < no; o++){ p[o] = seq + opt_off[o]; len[o] = opt_off[o+1] - opt_off[o]; option_hash(p[o], len[o], &h[o], &pw[o]); }
  }
  int64_t A() const { return (int64_t)n[0]*n[1]*n[2]; }
  void hap(int k, int o[3]) const { hs_alleles_digits(n[0], n[1], n[2], k, &o[0], &o[1], &o[2]); o[0] += first[0]; o[1] += first[1]; o[2] += first[2]; }
  uint64_t key(const int o[3], int bits, int64_t* total) const {
    *total = (int64_t)len[o[0]] + len[o[1]] + len[o[2]];
    return hs_alleles_hap_hash(h[o[0]], h[o[1]], pw[o[1]], h[o[2]], pw[o[2]], bits);
  }
};
bool equal(const Side& x, const int a[3], const Side& y, const int b[3]){
  return hs_alleles_equal(x.p[a[0]], x.len[a[0]], x.p[a[1]], x.len[a[1]], x.p[a[2]], x.len[a[2]], y.p[b[0]], y.len[b[0]], y.p[b[1]], y.len[b[1]], y.p[b[2]], y.len[b[2]]);
}

}  // namespace

int plan(const hipstr_alleles_request_t* rq, Plan& P, hipstr_alleles& a, std::string& err){
  if (!rq || !rq->pooled) return fail(err, "null argument");
  const hipstr_batch_t* b = rq->pooled;
  const int nl = b->n_loci;
  if (nl < 0) return fail(err, "negative locus count");
  if (nl > 0 && (!b->blk_start || !b->blk_end || !b->blk_nopts || !b->opt_off || !b->seq || !b->hap_off || !b->read_off)) return fail(err, "null table in a batch with loci");
  if (rq->keep_blocks & ~7u) return fail(err, "keep_blocks names a block outside 0..2");
  if (rq->add_off && (!rq->add_seq_off || !rq->add_seq)) return fail(err, "add_off without add_seq_off / add_seq");
  P.rq = rq; P.b = b; P.nl = nl;
  P.o_opt0.assign((size_t)nl + 1, 0); P.n_opt0.assign((size_t)nl + 1, 0); P.on.assign((size_t)nl, 1);
  // ---- the old tables
  int64_t n_old = 0;
  for (int i = 0; i < 3*nl; i++){
    if (b->blk_nopts[i] < 1) return fail(err, at("haplotype block without options", i/3, i%3));
    n_old += b->blk_nopts[i];
    if (n_old > INT32_MAX) return fail(err, "more than INT32_MAX options");
    if (i%3 == 2) P.o_opt0[(size_t)i/3 + 1] = (int32_t)n_old;
  }
  if (nl > 0 && b->opt_off[0] != 0) return fail(err, "opt_off does not start at 0");
  for (int64_t o = 0; o < n_old; o++) if (b->opt_off[o+1] < b->opt_off[o]) return fail(err, "opt_off decreases");
  if (nl > 0 && b->hap_off[0] != 0) return fail(err, "hap_off does not start at 0");
  for (int l = 0; l < nl; l++){
    if (b->hap_off[l+1] < b->hap_off[l]) return fail(err, "hap_off decreases");
    const int64_t combs = (int64_t)b->blk_nopts[3*l]*b->blk_nopts[3*l+1];
    if (combs > INT32_MAX || combs*b->blk_nopts[3*l+2] != (int64_t)b->hap_off[l+1] - b->hap_off[l]) return fail(err, at("hap_off is not the prefix sum of num_combs", l));
  }
  int64_t n_add = 0;
  if (rq->add_off){
    if (rq->add_off[0] != 0) return fail(err, "add_off does not start at 0");
    for (int i = 0; i < 3*nl; i++) if (rq->add_off[i+1] < rq->add_off[i]) return fail(err, "add_off decreases");
    n_add = rq->add_off[3*nl];
    if (rq->add_seq_off[0] != 0) return fail(err, "add_seq_off does not start at 0");
    for (int64_t i = 0; i < n_add; i++) if (rq->add_seq_off[i+1] < rq->add_seq_off[i]) return fail(err, "add_seq_off decreases");
  }
  // ---- the new counts: kept options, then the adds
  a.blk_nopts.assign((size_t)3*nl, 0); a.hap_off.assign((size_t)nl + 1, 0); a.new_n.assign((size_t)nl, 0); a.added.assign((size_t)nl, 0);
  P.n_src.clear(); P.n_src.reserve((size_t)(n_old + n_add));
  std::vector<int32_t> n_len; n_len.reserve((size_t)(n_old + n_add));
  int64_t haps = 0;
  for (int l = 0; l < nl; l++){
    const bool on = !rq->locus_on || rq->locus_on[l];
    P.on[l] = on ? 1 : 0;
    int64_t combs = 1;
    for (int k = 0; k < 3; k++){
      const int o0 = P.o_opt0[l] + (k > 0 ? b->blk_nopts[3*l] : 0) + (k > 1 ? b->blk_nopts[3*l+1] : 0), no = b->blk_nopts[3*l+k];
      const bool filter = on && rq->keep && ((rq->keep_blocks >> k) & 1);
      if (filter && !rq->keep[o0]) return fail(err, at("keep drops option 0: HapBlock::remove_alleles asserts", l, k));
      int64_t cnt = 0;
      for (int o = 0; o < no; o++)
        if (!filter || rq->keep[o0 + o]){ P.n_src.push_back(b->opt_off[o0 + o]); n_len.push_back(b->opt_off[o0 + o + 1] - b->opt_off[o0 + o]); cnt++; }
      if (on && rq->add_off)
        for (int i = rq->add_off[3*l+k]; i < rq->add_off[3*l+k+1]; i++){
          P.n_src.push_back(-1 - rq->add_seq_off[i]); n_len.push_back(rq->add_seq_off[i+1] - rq->add_seq_off[i]); cnt++; a.added[l] = 1;
        }
      if (cnt > INT32_MAX) return fail(err, at("more than INT32_MAX options", l, k));
      a.blk_nopts[(size_t)3*l+k] = (int32_t)cnt;
      combs *= cnt;
      if (combs > INT32_MAX) return fail(err, at("the new num_combs exceeds INT32_MAX", l));
    }
    haps += combs;
    if (haps > INT32_MAX) return fail(err, "the new haplotype counts sum to more than INT32_MAX");
    if (P.n_src.size() > (size_t)INT32_MAX) return fail(err, "more than INT32_MAX options");
    a.new_n[l] = (int32_t)combs; a.hap_off[(size_t)l+1] = (int32_t)haps; P.n_opt0[(size_t)l+1] = (int32_t)P.n_src.size();
  }
  const size_t n_new = P.n_src.size();
  a.opt_off.assign(n_new + 1, 0);
  int64_t bytes = 0;
  for (size_t o = 0; o < n_new; o++){
    bytes += n_len[o];
    if (bytes > INT32_MAX) return fail(err, "more than INT32_MAX new sequence bytes");
    a.opt_off[o+1] = (int32_t)bytes;
  }
  a.seq.assign((size_t)bytes + 1, 0);
  a.mapping.assign((size_t)(nl ? b->hap_off[nl] : 0), -1);
  a.realign.assign((size_t)haps, 0);
  for (int k = 0; k < 3; k++) a.h2a[k].assign((size_t)haps, 0);
  return 0;
}

void gather_locus(const Plan& P, int l, hipstr_alleles& a){
  for (int o = P.n_opt0[l]; o < P.n_opt0[(size_t)l+1]; o++){
    const int len = a.opt_off[(size_t)o+1] - a.opt_off[o], src = P.n_src[o];
    if (len) memcpy(a.seq.data() + a.opt_off[o], src >= 0 ? P.b->seq + src : P.rq->add_seq + (-1 - src), (size_t)len);
  }
}

void identity_locus(const Plan& P, int l, hipstr_alleles& a){
  const int32_t* n = a.blk_nopts.data() + 3*(size_t)l;
  const int h0 = a.hap_off[l], A = a.new_n[l], m0 = P.b->hap_off[l];
  for (int k = 0; k < A; k++){
    int o[3]; hs_alleles_digits(n[0], n[1], n[2], k, &o[0], &o[1], &o[2]);
    a.mapping[(size_t)m0 + k] = k; a.realign[(size_t)h0 + k] = 0;
    for (int blk = 0; blk < 3; blk++) a.h2a[blk][(size_t)h0 + k] = o[blk];
  }
}

void map_locus(const Plan& P, int l, hipstr_alleles& a, int hash_bits, int64_t counts[2]){
  const hipstr_batch_t* b = P.b;
  Side O, N;
  O.init(b->blk_nopts + 3*l, b->opt_off + P.o_opt0[l], b->seq);
  N.init(a.blk_nopts.data() + 3*(size_t)l, a.opt_off.data() + P.n_opt0[l], a.seq.data());
  const int A_old = (int)O.A(), A_new = (int)N.A();
  uint32_t slots = 64; while ((int64_t)slots < 2*(int64_t)A_old) slots <<= 1;
  std::vector<int32_t> lead((size_t)slots, -1), val((size_t)slots, -1);
  int32_t* map = a.mapping.data() + b->hap_off[l];
  // ---- the old haplotypes: the first of a key leads its slot, the highest index is its value (:335)
  for (int i = 0; i < A_old; i++){
    int o[3]; O.hap(i, o);
    int64_t tl; const uint64_t h = O.key(o, hash_bits, &tl);
    for (uint32_t s = hs_alleles_slot(h, tl, slots); ; s = (s + 1) & (slots - 1)){
      counts[0]++;
      if (lead[s] < 0){ lead[s] = i; val[s] = i; break; }
      int q[3]; O.hap(lead[s], q);
      int64_t ql; const uint64_t qh = O.key(q, hash_bits, &ql);
      if (qh != h || ql != tl) continue;
      counts[1]++;
      if (equal(O, o, O, q)){ val[s] = std::max(val[s], i); break; }
    }
    map[i] = -1;
  }
  // ---- the new ones, looked up (:358-367): the last new haplotype of a key takes the mapping
  const int h0 = a.hap_off[l];
  for (int j = 0; j < A_new; j++){
    int o[3]; N.hap(j, o);
    for (int blk = 0; blk < 3; blk++) a.h2a[blk][(size_t)h0 + j] = o[blk] - N.first[blk];
    int64_t tl; const uint64_t h = N.key(o, hash_bits, &tl);
    uint8_t realign = 1;
    for (uint32_t s = hs_alleles_slot(h, tl, slots); ; s = (s + 1) & (slots - 1)){
      counts[0]++;
      if (lead[s] < 0) break;
      int q[3]; O.hap(lead[s], q);
      int64_t ql; const uint64_t qh = O.key(q, hash_bits, &ql);
      if (qh != h || ql != tl) continue;
      counts[1]++;
      if (equal(N, o, O, q)){ realign = 0; map[val[s]] = std::max(map[val[s]], j); break; }
    }
    a.realign[(size_t)h0 + j] = realign;
  }
}

void finish(const Plan& P, hipstr_alleles& a){
  a.batch = *P.b;
  a.batch.blk_nopts = a.blk_nopts.data(); a.batch.opt_off = a.opt_off.data(); a.batch.seq = a.seq.data(); a.batch.hap_off = a.hap_off.data();
  a.batch.realign_hap = a.realign.data();
  a.batch_all = a.batch; a.batch_all.realign_hap = NULL;
}

hipstr_alleles* apply_host(const hipstr_alleles_request_t* rq, int hash_bits, int64_t counts[4], std::string& err){
  Plan P; hipstr_alleles* a = new hipstr_alleles;
  if (plan(rq, P, *a, err)){ delete a; return NULL; }
  int64_t c[2] = {0, 0}, n_host = 0;
  for (int l = 0; l < P.nl; l++){
    gather_locus(P, l, *a);
    if (!P.on[l]){ identity_locus(P, l, *a); continue; }
    map_locus(P, l, *a, hash_bits, c); n_host++;
  }
  finish(P, *a);
  if (counts){ counts[0] = 0; counts[1] = n_host; counts[2] = c[0]; counts[3] = c[1]; }
  return a;
}

int step_plan(const hipstr_batch_t* b, const hipstr_census_out_t* cen, const int32_t* phase, int32_t max_total, Step& S, std::string& err){
  if (!b || !cen || !phase) return fail(err, "null argument");
  const int nl = b->n_loci;
  if (nl < 0) return fail(err, "negative locus count");
  if (nl > 0 && (!b->blk_nopts || !b->opt_off || !b->hap_off)) return fail(err, "null table in a batch with loci");
  if (nl > 0 && (!cen->cand_off || !cen->cand_seq_off || !cen->cand_seq || !cen->new_n_haps || !cen->called || !cen->spanned)) return fail(err, "null census array");
  if (max_total < 0) return fail(err, "negative max_total_haplotypes");
  const int64_t max_haps = max_total ? max_total : 1000;
  int64_t n_opts = 0;
  for (int i = 0; i < 3*nl; i++){
    if (b->blk_nopts[i] < 1) return fail(err, at("haplotype block without options", i/3, i%3));
    n_opts += b->blk_nopts[i];
    if (n_opts > INT32_MAX) return fail(err, "more than INT32_MAX options");
  }
  if (nl > 0 && cen->cand_off[0] != 0) return fail(err, "cand_off does not start at 0");
  for (int l = 0; l < nl; l++){
    if (cen->cand_off[l+1] < cen->cand_off[l]) return fail(err, "cand_off decreases");
    if (phase[l] < HIPSTR_PHASE_ADD || phase[l] > HIPSTR_PHASE_ABORTED) return fail(err, at("phase outside 0..4", l));
  }
  const int n_cand = nl ? cen->cand_off[nl] : 0;
  for (int i = 0; i < n_cand; i++) if (cen->cand_seq_off[i+1] < cen->cand_seq_off[i] || cen->cand_seq_off[0] < 0) return fail(err, "cand_seq_off decreases");
  S.on.assign((size_t)nl, 0); S.keep.assign((size_t)n_opts, 1); S.add_off.assign((size_t)3*nl + 1, 0); S.add_seq_off.assign(1, 0); S.add_seq.clear();
  S.phase.assign(phase, phase + nl); S.status.assign((size_t)nl, 0); S.n_added.assign((size_t)nl, 0); S.n_removed.assign((size_t)nl, 0); S.n_affected.assign((size_t)nl, 0);
  S.any_added = 0;
  int64_t o0 = 0;
  for (int l = 0; l < nl; l++){
    const int32_t* no = b->blk_nopts + 3*l;
    const int64_t first[3] = { o0, o0 + no[0], o0 + no[0] + no[1] };
    o0 += (int64_t)no[0] + no[1] + no[2];
    int32_t& ph = S.phase[l];
    int adds = 0;
    if (ph == HIPSTR_PHASE_ADD){                                        // id_and_align_to_stutter_alleles :573-599
      const int c0 = cen->cand_off[l], c1 = cen->cand_off[l+1];
      if (c1 > c0){
        if (cen->new_n_haps[l] > max_haps){ ph = HIPSTR_PHASE_ABORTED; S.status[l] = 1; }      // :591-595
        else {
          adds = c1 - c0;
          for (int i = c0; i < c1; i++){
            S.add_seq.insert(S.add_seq.end(), cen->cand_seq + cen->cand_seq_off[i], cen->cand_seq + cen->cand_seq_off[i+1]);
            if (S.add_seq.size() > (size_t)INT32_MAX) return fail(err, "more than INT32_MAX candidate bytes");
            S.add_seq_off.push_back((int32_t)S.add_seq.size());
          }
          S.n_added[l] = adds; S.on[l] = 1; S.any_added = 1;
        }
      }
      else ph = HIPSTR_PHASE_UNCALLED;
    }
    bool stop = false;
    if (ph == HIPSTR_PHASE_UNCALLED){                                   // :647-654 takes `called`
      ph = HIPSTR_PHASE_UNSPANNED;
      int removed = 0, blocks = 0;
      for (int k = 0; k < 3; k++){
        if (no[k] <= 1) continue;                                       // :255
        int here = 0;
        for (int o = 1; o < no[k]; o++) if (!cen->called[first[k] + o]){ S.keep[(size_t)(first[k] + o)] = 0; here++; }
        removed += here; blocks += here ? 1 : 0;
      }
      if (removed){ S.n_removed[l] = removed; S.n_affected[l] = blocks; S.on[l] = 1; stop = true; }
    }
    if (ph == HIPSTR_PHASE_UNSPANNED && !stop){                         // :657-663 takes `spanned`
      if (no[0] != 1 || no[2] != 1) return fail(err, at("a locus reaches UNSPANNED with a flank block of more than one option: the census writes spanned for block 1 only", l));
      ph = HIPSTR_PHASE_DONE;
      int here = 0;
      for (int o = 1; o < no[1]; o++) if (!cen->spanned[first[1] + o]){ S.keep[(size_t)(first[1] + o)] = 0; here++; }
      if (here){ S.n_removed[l] = here; S.n_affected[l] = 1; S.on[l] = 1; }
    }
    S.add_off[(size_t)3*l + 1] = S.add_off[(size_t)3*l];
    S.add_off[(size_t)3*l + 2] = S.add_off[(size_t)3*l + 1] + adds;
    S.add_off[(size_t)3*l + 3] = S.add_off[(size_t)3*l + 2];
  }
  S.add_seq.push_back(0);
  memset(&S.rq, 0, sizeof S.rq);
  S.rq.pooled = b; S.rq.locus_on = S.on.data(); S.rq.keep = S.keep.data(); S.rq.keep_blocks = 7u;
  S.rq.add_off = S.add_off.data(); S.rq.add_seq_off = S.add_seq_off.data(); S.rq.add_seq = S.add_seq.data();
  return 0;
}

}  // namespace hipstr_al
