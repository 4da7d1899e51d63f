// hapgen_host.cpp — host twin of the haplotype generator (hapgen.hip) and the assembly of the batch it leaves behind.  Plain C++: no HIP,
// no device; compiles next to a stand-alone program (tests/cpp/hapgen_host_test.cpp).
//
// A locus' counted reads are ordered once by (length, folded bytes, sample): the runs of equal strings are the distinct strings in the
// order the outputs list them, and inside a run the samples ascend, which is the order sample_counts is summed in.  The extracted string
// of a read is a run of its own bases (offset, length): nothing is allocated per read.
#include "hapgen_host.h"
#include "hapgen_layout.h"

#include <limits.h>
#include <string.h>

#include <algorithm>

namespace hipstr_hg {

namespace {

// the walk of extract_sequence (:86-152) over read bases instead of the gapped alignment string: off / len of the collected run
void extract(const char* cop, const int32_t* clen, int nc, int32_t start, int32_t rs, int32_t re, int32_t& off, int32_t& len){
  int ci = 0, ch = 0; int32_t pos = start, ri = 0, kept = 0;
  while (ci < nc){
    const int32_t num = clen[ci]; const char op = cop[ci];
    if (ch == num){ ci++; ch = 0; }
    else if (pos > re) break;
    else if (pos == re){
      if (op != 'I') break;
      kept += num; ri += num; ch = 0; ci++;
    }
    else if (pos >= rs){
      int32_t nb = std::min(re - pos, num - ch);
      if (op == 'I'){ nb = num; kept += nb; ri += nb; }
      else if (op == 'D') pos += nb;
      else { kept += nb; ri += nb; pos += nb; }
      ch += nb;
    }
    else {
      int32_t nb;
      if (op == 'I'){ nb = num - ch; ri += nb; }
      else { nb = std::min(rs - pos, num - ch); pos += nb; if (op != 'D') ri += nb; }
      ch += nb;
    }
  }
  off = ri - kept; len = kept;
}

struct Str { const char* p; int32_t len; };
inline int cmp_fold(const Str& a, const Str& b){      // (length, bytes as unsigned char)
  if (a.len != b.len) return a.len < b.len ? -1 : 1;
  for (int32_t i = 0; i < a.len; i++){
    const unsigned char x = (unsigned char)fold(a.p[i]), y = (unsigned char)fold(b.p[i]);
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

}  // namespace

int locus_status(int64_t region_start, int64_t region_stop, int64_t chrom_len, int64_t min_flagged_start, int64_t max_flagged_stop){
  return hs_hapgen_status(region_start, region_stop, chrom_len, min_flagged_start, max_flagged_stop);
}

void trim_amounts(int min_len, int ideal, int common_prefix, int common_suffix, int& left_trim, int& right_trim){
  hs_hapgen_trim(min_len, ideal, common_prefix, common_suffix, &left_trim, &right_trim);
}

int check(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, const hipstr_hapgen_out_t* out, bool need_stutter, std::vector<int32_t>& stop, std::string& err){
  stop.clear();
  if (!b || !rq || !out){ err = "null argument"; return 1; }
  if (b->n_loci < 0){ err = "null or negative-size batch"; return 1; }
  const int nl = b->n_loci;
  if (!out->status || !out->blk_start || !out->blk_end || !out->blk_nopts || !out->opt_off || !out->seq || !out->n_spanning || !out->n_samples_spanning ||
      !out->n_distinct || !out->left_trim || !out->right_trim || !out->min_aln_start || !out->max_aln_stop){ err = "null output array"; return 1; }
  if (nl == 0) return 0;
  if (!b->read_off || !b->base_off || !b->bases || !b->read_start || !b->cigar_off || !b->cigar_op || !b->cigar_len){ err = "null table in a batch with loci"; return 1; }
  if (!rq->region_start || !rq->region_stop || !rq->period || !rq->chrom_len || !rq->win_off || !rq->window || !rq->n_samples || !rq->sample_label ||
      (need_stutter && !rq->stutter)){ err = "null array in the request"; return 1; }
  if (b->read_off[0] < 0 || rq->win_off[0] < 0){ err = "negative offset"; return 1; }
  for (int l = 0; l < nl; l++){
    if (b->read_off[l+1] < b->read_off[l]){ err = "read_off must not decrease"; return 1; }
    if (rq->win_off[l+1] < rq->win_off[l]){ err = "win_off must not decrease"; return 1; }
  }
  const int n0 = b->read_off[0], nr = b->read_off[nl];
  if (nr > n0 && (b->base_off[n0] < 0 || b->cigar_off[n0] < 0)){ err = "negative offset"; return 1; }
  for (int r = n0; r < nr; r++){
    if (b->base_off[r+1] < b->base_off[r]){ err = "base_off must not decrease"; return 1; }
    if (b->cigar_off[r+1] < b->cigar_off[r]){ err = "cigar_off must not decrease"; return 1; }
  }
  const int64_t nbases = nr > n0 ? (int64_t)b->base_off[nr] - b->base_off[n0] : 0;
  const int c0 = nr > n0 ? b->cigar_off[n0] : 0, nc = nr > n0 ? b->cigar_off[nr] : 0;
  if ((int64_t)nc - c0 > 2*nbases + 2*(int64_t)(nr - n0)){ err = "cigar_off holds more runs than the reads have bases"; return 1; }
  for (int c = c0; c < nc; c++){
    if (b->cigar_len[c] <= 0){ err = "CIGAR run of non-positive length"; return 1; }
    const char op = b->cigar_op[c];
    if (op != '=' && op != 'X' && op != 'I' && op != 'D'){ err = "CIGAR op other than = X I D"; return 1; }
  }
  std::vector<int32_t> st((size_t)(nr - n0) + 1);
  for (int l = 0; l < nl; l++){
    const int64_t rs = rq->region_start[l], rp = rq->region_stop[l];
    if (rq->period[l] < 1){ err = "period below 1"; return 1; }
    if (rp < rs){ err = "region_stop before region_start"; return 1; }
    if (rp > INT32_MAX - WIN_PAD){ err = "region_stop + 40 beyond 2^31"; return 1; }
    if (rq->n_samples[l] < 0){ err = "negative n_samples"; return 1; }
    if (locus_status(rs, rp, rq->chrom_len[l], INT64_MIN/2, INT64_MAX/2) != 1 && (int64_t)rq->win_off[l+1] - rq->win_off[l] < rp - rs + 2*WIN_PAD){
      err = "window shorter than region_stop - region_start + 80"; return 1;
    }
    for (int r = b->read_off[l]; r < b->read_off[l+1]; r++){
      if (rq->sample_label[r] < 0 || rq->sample_label[r] >= rq->n_samples[l]){ err = "sample_label outside [0, n_samples)"; return 1; }
      int64_t ref_len = 0, read_len = 0;
      for (int c = b->cigar_off[r]; c < b->cigar_off[r+1]; c++){
        if (b->cigar_op[c] != 'I') ref_len += b->cigar_len[c];
        if (b->cigar_op[c] != 'D') read_len += b->cigar_len[c];
      }
      if (read_len > (int64_t)b->base_off[r+1] - b->base_off[r]){ err = "CIGAR covers more bases than the read has"; return 1; }
      const int64_t end = (int64_t)b->read_start[r] + ref_len;
      if (end > INT32_MAX){ err = "read ends beyond 2^31"; return 1; }
      if (rq->read_stop && rq->read_stop[r] > end){ err = "read_stop beyond start + the =, X and D runs of the CIGAR"; return 1; }
      st[(size_t)(r - n0)] = rq->read_stop ? rq->read_stop[r] : (int32_t)end;
    }
  }
  stop.swap(st);
  return 0;
}

void locus_host(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, const int32_t* stop_all, int l, Sink& s){
  hipstr_hapgen_out_t* o = s.out;
  const int r0 = b->read_off[l], r1 = b->read_off[l+1], n0 = b->read_off[0];
  const int32_t* stop = stop_all - n0;                                   // indexed by the batch's read number
  const int32_t rs0 = rq->region_start[l], rp0 = rq->region_stop[l];
  int64_t min_all = INT32_MAX, max_all = INT32_MIN, min_f = INT32_MAX, max_f = INT32_MIN;
  for (int r = r0; r < r1; r++){
    min_all = std::min<int64_t>(min_all, b->read_start[r]); max_all = std::max<int64_t>(max_all, stop[r]);
    if (!rq->use_read || rq->use_read[r]){ min_f = std::min<int64_t>(min_f, b->read_start[r]); max_f = std::max<int64_t>(max_f, stop[r]); }
    if (o->ext_off) o->ext_off[r] = -1;
    if (o->ext_len) o->ext_len[r] = -1;
  }
  const int status = locus_status(rs0, rp0, rq->chrom_len[l], min_f, max_f);
  o->status[l] = status; o->min_aln_start[l] = (int32_t)min_all; o->max_aln_stop[l] = (int32_t)max_all;
  o->n_spanning[l] = o->n_samples_spanning[l] = o->n_distinct[l] = o->left_trim[l] = o->right_trim[l] = 0;
  for (int k = 0; k < 3; k++) o->blk_start[3*l+k] = o->blk_end[3*l+k] = o->blk_nopts[3*l+k] = 0;
  if (status != 0) return;

  const int32_t rs = rs0 - LEFT_PAD, re = rp0 + RIGHT_PAD;
  const char* win = rq->window + rq->win_off[l];                        // win[i] = chrom_seq[rs0 - 40 + i]
  const Str ref = { win + (WIN_PAD - LEFT_PAD), re - rs };
  // ---- the counted reads and their runs of bases
  struct Rd { int32_t r, sample; Str s; };
  std::vector<Rd> rd;
  for (int r = r0; r < r1; r++){
    if (rq->use_read && !rq->use_read[r]) continue;
    if (b->read_start[r] >= rs || stop[r] <= re) continue;              // :83-84
    int32_t off, len;
    const int c = b->cigar_off[r];
    extract(b->cigar_op + c, b->cigar_len + c, b->cigar_off[r+1] - c, b->read_start[r], rs, re, off, len);
    if (o->ext_off) o->ext_off[r] = off;
    if (o->ext_len) o->ext_len[r] = len;
    rd.push_back(Rd{ r, rq->sample_label[r], Str{ b->bases + b->base_off[r] + off, len } });
  }
  const int S = rq->n_samples[l];
  std::vector<int32_t> samp_reads((size_t)S, 0);
  for (const Rd& x : rd) samp_reads[(size_t)x.sample]++;
  int tot_samples = 0;
  for (int i = 0; i < S; i++) tot_samples += samp_reads[(size_t)i] > 0;
  const int tot_reads = (int)rd.size();
  std::sort(rd.begin(), rd.end(), [](const Rd& a, const Rd& c){
    const int k = cmp_fold(a.s, c.s);
    if (k) return k < 0;
    return a.sample != c.sample ? a.sample < c.sample : a.r < c.r;
  });
  // ---- per distinct string: reads, strong samples, the sample fraction; what is selected
  struct Opt { Str s; };
  std::vector<Opt> opts;
  opts.push_back(Opt{ ref });
  int n_distinct = 0;
  for (size_t i = 0; i < rd.size(); ){
    size_t j = i; int32_t rep = rd[i].r, strong = 0; double frac = 0.0;
    while (j < rd.size() && cmp_fold(rd[j].s, rd[i].s) == 0){
      size_t k = j;
      while (k < rd.size() && rd[k].sample == rd[j].sample && cmp_fold(rd[k].s, rd[i].s) == 0){ rep = std::min(rep, rd[k].r); k++; }
      const int cnt = (int)(k - j), sr = samp_reads[(size_t)rd[j].sample];
      if ((double)cnt >= 2.0 && (double)cnt >= 0.2*sr) strong++;                              // :181
      frac += cnt*1.0/sr;                                                                      // :183
      j = k;
    }
    const int reads = (int)(j - i);
    const int64_t d = s.dist + n_distinct;
    if (o->dist_len) o->dist_len[d] = rd[i].s.len;
    if (o->dist_rep) o->dist_rep[d] = rep;
    if (o->dist_reads) o->dist_reads[d] = reads;
    if (o->dist_strong) o->dist_strong[d] = strong;
    if (o->dist_frac) o->dist_frac[d] = frac;
    n_distinct++;
    const bool selected = strong >= 1 || frac > 0.05*tot_samples || (double)reads > 0.05*tot_reads;      // :207-226
    if (selected && cmp_fold(rd[i].s, ref) != 0) opts.push_back(Opt{ rd[i].s });
    i = j;
  }
  s.dist += n_distinct;
  // ---- trim: the common prefix / suffix of all options, as far as trim can use it
  int min_len = INT_MAX;
  for (const Opt& x : opts) min_len = std::min(min_len, (int)x.s.len);
  const int ideal = 3*rq->period[l];
  int cp = 0, cs = 0, lt = 0, rt = 0;
  if (min_len > ideal){
    const int lim = std::min((int)LEFT_PAD, min_len - ideal);
    auto same = [&](int i, bool from_end){
      const char c = fold(from_end ? opts[0].s.p[opts[0].s.len - 1 - i] : opts[0].s.p[i]);
      for (const Opt& x : opts) if (fold(from_end ? x.s.p[x.s.len - 1 - i] : x.s.p[i]) != c) return false;
      return true;
    };
    while (cp < lim && same(cp, false)) cp++;
    while (cs < lim && same(cs, true)) cs++;
    trim_amounts(min_len, ideal, cp, cs, lt, rt);
  }
  const int32_t b1s = rs + lt, b1e = re - rt;
  const int32_t min_start = (int32_t)std::min<int64_t>(b1s - 10, std::max<int64_t>(b1s - REF_FLANK_LEN, min_all));      // :349-350
  const int32_t max_stop = (int32_t)std::max<int64_t>(b1e + 10, std::min<int64_t>(b1e + REF_FLANK_LEN, max_all));
  o->n_spanning[l] = tot_reads; o->n_samples_spanning[l] = tot_samples; o->n_distinct[l] = n_distinct; o->left_trim[l] = lt; o->right_trim[l] = rt;
  o->blk_start[3*l] = min_start; o->blk_end[3*l] = b1s; o->blk_nopts[3*l] = 1;
  o->blk_start[3*l+1] = b1s; o->blk_end[3*l+1] = b1e; o->blk_nopts[3*l+1] = (int32_t)opts.size();
  o->blk_start[3*l+2] = b1e; o->blk_end[3*l+2] = max_stop; o->blk_nopts[3*l+2] = 1;
  auto put = [&](const char* p, int32_t len){
    for (int32_t i = 0; i < len; i++) o->seq[s.seq + i] = fold(p[i]);
    s.seq += len; s.opts++;
    o->opt_off[s.opts] = (int32_t)s.seq;
  };
  const int32_t w0 = rs0 - WIN_PAD;
  put(win + (min_start - w0), b1s - min_start);
  for (const Opt& x : opts) put(x.s.p + lt, x.s.len - lt - rt);
  put(win + (b1e - w0), max_stop - b1e);
}

void hapgen_host(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, const int32_t* stop, hipstr_hapgen_out_t* out){
  Sink s{ out, 0, 0, 0 };
  out->opt_off[0] = 0;
  for (int l = 0; l < b->n_loci; l++) locus_host(b, rq, stop, l, s);
}

Arrays::Arrays(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq){
  const size_t nl = (size_t)b->n_loci, n = nl ? (size_t)b->read_off[nl] : 0;
  const size_t nb = n ? (size_t)b->base_off[n] : 0, nw = nl ? (size_t)rq->win_off[nl] : 0;
  // status, 3 x blk, opt_off, 7 per-locus, 2 + 4 per-read
  const size_t per_l = nl + 1, per_r = n + 1, n_opt = 3*nl + n + 2;
  i32.assign(per_l*(1 + 9 + 7) + n_opt + 6*per_r, 0);
  seq.assign(nw + nb + 1, 0); frac.assign(per_r, 0.0);
  int32_t* p = i32.data();
  auto take = [&](size_t cnt){ int32_t* q = p; p += cnt; return q; };
  out.status = take(per_l); out.blk_start = take(3*per_l); out.blk_end = take(3*per_l); out.blk_nopts = take(3*per_l); out.opt_off = take(n_opt);
  out.seq = seq.data();
  out.n_spanning = take(per_l); out.n_samples_spanning = take(per_l); out.n_distinct = take(per_l); out.left_trim = take(per_l); out.right_trim = take(per_l);
  out.min_aln_start = take(per_l); out.max_aln_stop = take(per_l);
  out.ext_off = take(per_r); out.ext_len = take(per_r); out.dist_len = take(per_r); out.dist_rep = take(per_r); out.dist_reads = take(per_r); out.dist_strong = take(per_r);
  out.dist_frac = frac.data();
}

hipstr_hapgen_batch_t* assemble_batch(const hipstr_batch_t* b, const hipstr_hapgen_request_t* rq, const hipstr_hapgen_out_t* o){
  const int64_t nl = b->n_loci;
  std::vector<int32_t> keep;
  int64_t n_opts_all = 0, n_reads = 0, n_bases = 0, n_cig = 0, n_opts = 0, n_seq = 0;
  for (int64_t l = 0; l < nl; l++){
    const int64_t no = (int64_t)o->blk_nopts[3*l] + o->blk_nopts[3*l+1] + o->blk_nopts[3*l+2];
    if (o->status[l] == 0){
      keep.push_back((int32_t)l);
      n_opts += no; n_seq += o->opt_off[n_opts_all + no] - o->opt_off[n_opts_all];
      const int r0 = b->read_off[l], r1 = b->read_off[l+1];
      n_reads += r1 - r0;
      if (r1 > r0){ n_bases += b->base_off[r1] - b->base_off[r0]; n_cig += b->cigar_off[r1] - b->cigar_off[r0]; }
    }
    n_opts_all += no;
  }
  const int64_t nk = (int64_t)keep.size();
  size_t tot = 0;
  auto take = [&](size_t bytes){ const size_t off = tot; tot = (tot + bytes + 7) & ~(size_t)7; return off; };
  const size_t s_bs = take(12*nk), s_be = take(12*nk), s_bn = take(12*nk), s_per = take(4*nk), s_st = take(48*nk), s_oo = take(4*(n_opts + 1)),
               s_seq = take(n_seq + 1), s_ho = take(4*(nk + 1)), s_ro = take(4*(nk + 1)), s_bo = take(4*(n_reads + 1)), s_b = take(n_bases + 1),
               s_q = take(n_bases + 1), s_rs = take(4*n_reads), s_co = take(4*(n_reads + 1)), s_cop = take(n_cig + 1), s_cl = take(4*(n_cig + 1)),
               s_loc = take(4*(nk + 1)), s_stat = take(4*(nl + 1));
  hipstr_hapgen_batch_t* hb = new hipstr_hapgen_batch_t();
  hb->mem.assign(tot + 8, 0);
  uint8_t* m = hb->mem.data();
  int32_t* bs = (int32_t*)(m + s_bs), *be = (int32_t*)(m + s_be), *bn = (int32_t*)(m + s_bn), *per = (int32_t*)(m + s_per), *oo = (int32_t*)(m + s_oo),
         * ho = (int32_t*)(m + s_ho), *ro = (int32_t*)(m + s_ro), *bo = (int32_t*)(m + s_bo), *rst = (int32_t*)(m + s_rs), *co = (int32_t*)(m + s_co),
         * cl = (int32_t*)(m + s_cl), *loc = (int32_t*)(m + s_loc), *stat = (int32_t*)(m + s_stat);
  double* stt = (double*)(m + s_st);
  char* seq = (char*)(m + s_seq), *bases = (char*)(m + s_b), *quals = (char*)(m + s_q), *cop = (char*)(m + s_cop);
  for (int64_t l = 0; l < nl; l++) stat[l] = o->status[l];
  int64_t g_opt = 0, k_opt = 0, k_seq = 0, k_read = 0, k_base = 0, k_cig = 0, k = 0;
  oo[0] = 0; ho[0] = 0; ro[0] = 0; bo[0] = 0; co[0] = 0;
  for (int64_t l = 0; l < nl; l++){
    const int64_t no = (int64_t)o->blk_nopts[3*l] + o->blk_nopts[3*l+1] + o->blk_nopts[3*l+2];
    if (o->status[l] == 0){
      loc[k] = (int32_t)l; per[k] = rq->period[l];
      for (int i = 0; i < 6; i++) stt[6*k + i] = rq->stutter[6*l + i];
      int64_t A = 1;
      for (int i = 0; i < 3; i++){ bs[3*k+i] = o->blk_start[3*l+i]; be[3*k+i] = o->blk_end[3*l+i]; bn[3*k+i] = o->blk_nopts[3*l+i]; A *= o->blk_nopts[3*l+i]; }
      ho[k+1] = (int32_t)(ho[k] + A);
      const int32_t src0 = o->opt_off[g_opt];
      for (int64_t i = 0; i < no; i++) oo[k_opt + i + 1] = (int32_t)(k_seq + (o->opt_off[g_opt + i + 1] - src0));
      const int32_t nb = o->opt_off[g_opt + no] - src0;
      if (nb) memcpy(seq + k_seq, o->seq + src0, (size_t)nb);
      k_opt += no; k_seq += nb;
      for (int r = b->read_off[l]; r < b->read_off[l+1]; r++){
        const int len = b->base_off[r+1] - b->base_off[r], cig = b->cigar_off[r+1] - b->cigar_off[r];
        rst[k_read] = b->read_start[r];
        if (len){ memcpy(bases + k_base, b->bases + b->base_off[r], (size_t)len); memcpy(quals + k_base, b->quals + b->base_off[r], (size_t)len); }
        if (cig){ memcpy(cop + k_cig, b->cigar_op + b->cigar_off[r], (size_t)cig); memcpy(cl + k_cig, b->cigar_len + b->cigar_off[r], 4*(size_t)cig); }
        k_base += len; k_cig += cig; k_read++;
        bo[k_read] = (int32_t)k_base; co[k_read] = (int32_t)k_cig;
      }
      ro[k+1] = (int32_t)k_read;
      k++;
    }
    g_opt += no;
  }
  hipstr_batch_t& q = hb->batch;
  memset(&q, 0, sizeof q);
  q.n_loci = (int32_t)nk;
  q.blk_start = bs; q.blk_end = be; q.blk_nopts = bn; q.period = per; q.stutter = stt; q.opt_off = oo; q.seq = seq; q.hap_off = ho; q.realign_hap = NULL;
  q.read_off = ro; q.base_off = bo; q.bases = bases; q.quals = quals; q.read_start = rst; q.cigar_off = co; q.cigar_op = cop; q.cigar_len = cl; q.realign_read = NULL;
  hb->locus = loc; hb->status = stat;
  return hb;
}

}  // namespace hipstr_hg
