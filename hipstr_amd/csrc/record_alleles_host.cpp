// record_alleles_host.cpp — see record_alleles_host.h.
#include "record_alleles_host.h"

#include <algorithm>
#include <string.h>

namespace hipstr_rec_alleles {

namespace {
const int WIN_PAD = 40;
// upper(chrom_seq.substr(from, n)) out of the window; false when a byte is not there
bool chrom(const char* win, int32_t win_len, int32_t region_start, int64_t from, int64_t n, std::string* s){
  const int64_t w0 = (int64_t)region_start - WIN_PAD;
  s->clear();
  if (n <= 0) return true;
  if (from < 0 || from < w0 || from + n > w0 + win_len) return false;
  for (int64_t i = 0; i < n; i++){ const char c = win[from - w0 + i]; s->push_back((c >= 'a' && c <= 'z') ? (char)(c - 32) : c); }
  return true;
}
void fail(Locus* out, int status){
  out->status = status; out->pos = out->left_trim = out->right_trim = 0;
  out->alleles.clear(); out->bp_diff.clear(); out->old_to_new.clear(); out->new_to_old.clear();
}
}  // namespace

bool reorder(const std::vector<std::string>& alleles, std::vector<int32_t>* old_to_new, std::vector<int32_t>* new_to_old){
  const size_t V = alleles.size();
  std::vector<int32_t> idx(V);
  for (size_t i = 0; i < V; i++) idx[i] = (int32_t)i;
  auto before = [&](int32_t a, int32_t b){
    const std::string &x = alleles[a], &y = alleles[b];
    return x.size() != y.size() ? x.size() < y.size() : x.compare(y) < 0;
  };
  if (V > 1) std::sort(idx.begin() + 1, idx.end(), before);
  for (size_t i = 1; i < V; i++) if (alleles[idx[i]] == alleles[idx[i - 1]] || alleles[idx[i]] == alleles[0]) return false;
  new_to_old->assign(idx.begin(), idx.end());
  old_to_new->assign(V, -1);
  for (size_t i = 0; i < V; i++) (*old_to_new)[idx[i]] = (int32_t)i;
  return true;
}

void alleles_of(const std::vector<std::string>& options, int32_t start0, int32_t end0, int32_t region_start, int32_t region_stop,
                const char* win, int32_t win_len, Locus* out){
  std::vector<std::string> al = options;
  const size_t V = al.size();
  // :700-716
  int64_t left_trim = 0, start = start0;
  while (start + left_trim < region_start){
    bool trim = true;
    for (size_t i = 0; i < V && trim; i++)
      if ((size_t)left_trim + 1 >= al[i].size() || al[i][(size_t)left_trim] != al[0][(size_t)left_trim]) trim = false;
    if (!trim) break;
    left_trim++;
  }
  start += left_trim;
  for (size_t i = 0; i < V; i++) al[i] = al[i].substr((size_t)left_trim);
  // :718-736
  int64_t right_trim = 0, end = end0;
  while (end - right_trim > region_stop){
    bool trim = true;
    const size_t ref_size = al[0].size();
    for (size_t i = 0; i < V && trim; i++){
      const size_t alt_size = al[i].size();
      if ((size_t)right_trim + 1 >= alt_size || al[i][alt_size - (size_t)right_trim - 1] != al[0][ref_size - (size_t)right_trim - 1]) trim = false;
    }
    if (!trim) break;
    right_trim++;
  }
  end -= right_trim;
  for (size_t i = 0; i < V; i++) al[i] = al[i].substr(0, al[i].size() - (size_t)right_trim);
  // :738-742
  std::string left_flank, right_flank;
  if (start >= region_start && !chrom(win, win_len, region_start, region_start, start - region_start, &left_flank)) return fail(out, HIPSTR_ALLELES_OUTSIDE_WINDOW);
  if (end <= region_stop && !chrom(win, win_len, region_start, end, (int64_t)region_stop - end, &right_flank)) return fail(out, HIPSTR_ALLELES_OUTSIDE_WINDOW);
  int64_t pos = std::min<int64_t>(region_start, start);
  left_trim -= (int64_t)left_flank.size();
  right_trim -= (int64_t)right_flank.size();
  // :744-758
  if (left_flank.empty()){
    bool pad_left = false;
    const char first = al[0].empty() ? '\0' : al[0][0];
    for (size_t i = 1; i < V && !pad_left; i++) if (al[i].empty() || al[i][0] != first) pad_left = true;
    if (pad_left){
      pos -= 1; left_trim -= 1;
      if (!chrom(win, win_len, region_start, pos, 1, &left_flank)) return fail(out, HIPSTR_ALLELES_OUTSIDE_WINDOW);
    }
  }
  for (size_t i = 0; i < V; i++) al[i] = left_flank + al[i] + right_flank;
  pos += 1;                                                          // :766
  if (pos < INT32_MIN || pos > INT32_MAX) return fail(out, HIPSTR_ALLELES_OUTSIDE_WINDOW);
  if (!reorder(al, &out->old_to_new, &out->new_to_old)) return fail(out, HIPSTR_ALLELES_DUPLICATE);
  out->status = 0; out->pos = (int32_t)pos; out->left_trim = (int32_t)left_trim; out->right_trim = (int32_t)right_trim;
  out->bp_diff.resize(V);
  for (size_t i = 0; i < V; i++) out->bp_diff[i] = (int32_t)al[i].size() - (int32_t)al[0].size();       // :1047-1050
  out->alleles.swap(al);
}

bool flank_options(const std::vector<std::string>& lopts, const std::vector<std::string>& ropts, const std::string& ref_str, int left_trim, int right_trim,
                   std::vector<std::string>* lflanks, std::vector<std::string>* rflanks){
  lflanks->clear(); rflanks->clear();
  const int ref_len = (int)ref_str.size();
  bool ok = left_trim < ref_len && right_trim < ref_len && (int64_t)left_trim + right_trim < ref_len && right_trim >= 0;       // :1015-1016; substr(trim) of :1037
  for (size_t i = 0; ok && i < lopts.size(); i++){
    const std::string& seq = lopts[i];
    if ((int64_t)seq.size() + left_trim <= 0){ ok = false; break; }                                     // :1023
    lflanks->push_back(left_trim < 0 ? seq.substr(0, seq.size() - (size_t)(-(int64_t)left_trim)) : seq + ref_str.substr(0, (size_t)left_trim));
  }
  for (size_t i = 0; ok && i < ropts.size(); i++){
    const std::string& seq = ropts[i];
    if ((int64_t)seq.size() + right_trim <= 0){ ok = false; break; }                                    // :1035
    rflanks->push_back(ref_str.substr((size_t)(ref_len - right_trim), (size_t)right_trim) + seq);
  }
  if (!ok){ lflanks->clear(); rflanks->clear(); }
  return ok;
}

std::string check(const hipstr_batch_t* b, const hipstr_record_alleles_request_t* rq, const hipstr_record_alleles_out_t* out, int64_t* n_var){
  const int nl = b->n_loci;
  if (rq->win_off[0] < 0) return "negative offset";
  if (b->opt_off[0] != 0) return "opt_off must begin at 0";
  int64_t o = 0, nv = 0;
  for (int l = 0; l < nl; l++){
    if (rq->region_stop[l] < rq->region_start[l]) return "region_stop < region_start";
    if (rq->win_off[l + 1] < rq->win_off[l]) return "win_off must not decrease";
    for (int k = 0; k < 3; k++){
      const int n = b->blk_nopts[3*l + k];
      if (n < 0) return "a negative option count";
      if (k == 1 && n < 1) return "a block 1 without options";
      for (int i = 0; i < n; i++, o++) if (b->opt_off[o + 1] < b->opt_off[o]) return "opt_off must ascend";
      if (o > INT32_MAX - 1) return "too many options for one call";
    }
    nv += b->blk_nopts[3*l + 1];
  }
  (void)out;
  *n_var = nv;
  return "";
}

std::vector<std::string> block_options(const hipstr_batch_t* b, int64_t opt_base, int l, int blk){
  int64_t o = opt_base;
  for (int k = 0; k < blk; k++) o += b->blk_nopts[3*l + k];
  std::vector<std::string> v;
  for (int i = 0; i < b->blk_nopts[3*l + blk]; i++, o++) v.emplace_back(b->seq + b->opt_off[o], (size_t)(b->opt_off[o + 1] - b->opt_off[o]));
  return v;
}

std::string emit(const hipstr_batch_t* b, std::vector<Locus>& loci, hipstr_record_alleles_out_t* out){
  const int nl = b->n_loci;
  // the flank strings first (they may flag a locus), then the sizes, then the writes
  std::vector<std::vector<std::string>> lf((size_t)nl), rf((size_t)nl);
  const bool want_flanks = out->lflank_off || out->rflank_off;
  int64_t ob = 0, need_a = 0, need_l = 0, need_r = 0;
  for (int l = 0; l < nl; l++){
    Locus& L = loci[(size_t)l];
    if (want_flanks && L.status == 0){
      const std::vector<std::string> ref = block_options(b, ob, l, 1);
      if (!flank_options(block_options(b, ob, l, 0), block_options(b, ob, l, 2), ref[0], L.left_trim, L.right_trim, &lf[(size_t)l], &rf[(size_t)l]))
        L.status |= HIPSTR_ALLELES_FLANK_ASSERT;
    }
    for (const std::string& s : L.alleles) need_a += (int64_t)s.size();
    for (const std::string& s : lf[(size_t)l]) need_l += (int64_t)s.size();
    for (const std::string& s : rf[(size_t)l]) need_r += (int64_t)s.size();
    ob += b->blk_nopts[3*l] + b->blk_nopts[3*l + 1] + b->blk_nopts[3*l + 2];
  }
  if (need_a > out->cap_alleles || need_a > INT32_MAX) return "cap_alleles is too small";
  if (out->lflank_off && (need_l > out->cap_lflanks || need_l > INT32_MAX)) return "cap_lflanks is too small";
  if (out->rflank_off && (need_r > out->cap_rflanks || need_r > INT32_MAX)) return "cap_rflanks is too small";
  int64_t v = 0, at = 0, lo = 0, la = 0, ro = 0, ra = 0;
  for (int l = 0; l < nl; l++){
    const Locus& L = loci[(size_t)l];
    const int V = b->blk_nopts[3*l + 1];
    const bool ok = !L.alleles.empty();
    out->status[l] = L.status; out->pos[l] = L.pos; out->left_trim[l] = L.left_trim; out->right_trim[l] = L.right_trim;
    for (int i = 0; i < V; i++, v++){
      out->allele_off[v] = (int32_t)at;
      if (ok){ memcpy(out->alleles + at, L.alleles[(size_t)i].data(), L.alleles[(size_t)i].size()); at += (int64_t)L.alleles[(size_t)i].size(); }
      out->allele_bp_diff[v] = ok ? L.bp_diff[(size_t)i] : 0;
      out->old_to_new[v] = ok ? L.old_to_new[(size_t)i] : -1; out->new_to_old[v] = ok ? L.new_to_old[(size_t)i] : -1;
    }
    if (out->lflank_off) for (int i = 0; i < b->blk_nopts[3*l]; i++, lo++){
      out->lflank_off[lo] = (int32_t)la;
      if (!lf[(size_t)l].empty()){ const std::string& s = lf[(size_t)l][(size_t)i]; memcpy(out->lflanks + la, s.data(), s.size()); la += (int64_t)s.size(); }
    }
    if (out->rflank_off) for (int i = 0; i < b->blk_nopts[3*l + 2]; i++, ro++){
      out->rflank_off[ro] = (int32_t)ra;
      if (!rf[(size_t)l].empty()){ const std::string& s = rf[(size_t)l][(size_t)i]; memcpy(out->rflanks + ra, s.data(), s.size()); ra += (int64_t)s.size(); }
    }
  }
  out->allele_off[v] = (int32_t)at;
  if (out->lflank_off) out->lflank_off[lo] = (int32_t)la;
  if (out->rflank_off) out->rflank_off[ro] = (int32_t)ra;
  return "";
}

}  // namespace hipstr_rec_alleles
