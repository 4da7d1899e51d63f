// alleles_host_main.cpp — hipstr_amd/csrc/alleles_host.cpp as a stand-alone program, for a build with -fsanitize=address,undefined
// (tests/test_alleles_host.py): reads cases in the text format of tests/alleles_cases.py, runs them as one batch through
// hipstr_al::apply_host with the whole hash and with 4 bits of it, requires the same bytes from both, and prints per case
//   case NAME nopts N0 N1 N2 map M... realign R...
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hipstr_amd/csrc/alleles_host.h"

static std::string seq_of(const std::string& s){ return s == "-" ? std::string() : s; }

int main(int argc, char** argv){
  if (argc != 2){ fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in){ perror(argv[1]); return 2; }
  std::vector<std::string> names;
  std::vector<int32_t> blk_start, blk_end, blk_nopts, period, opt_off(1, 0), hap_off(1, 0), read_off(1, 0), add_off(1, 0), add_seq_off(1, 0);
  std::vector<double> stutter;
  std::vector<uint8_t> keep;
  std::string seq, add_seq, line, word;
  while (std::getline(in, line)){
    if (line.empty()) continue;
    std::istringstream hd(line);
    std::string name; int per = 0;
    hd >> word >> name >> per;
    if (word != "case" || !hd){ fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
    names.push_back(name); period.push_back(per);
    const double sm[6] = { 0.9, 0.05, 0.05, 0.7, 0.005, 0.005 };
    stutter.insert(stutter.end(), sm, sm + 6);
    int combs = 1; size_t first[3];
    for (int b = 0; b < 3; b++){
      std::getline(in, line);
      std::istringstream ls(line);
      int idx = 0, start = 0, end = 0, n = 0; std::string s;
      ls >> word >> idx >> start >> end >> n;
      if (word != "block" || idx != b || !ls || n < 1){ fprintf(stderr, "bad block line: %s\n", line.c_str()); return 2; }
      blk_start.push_back(start); blk_end.push_back(end); blk_nopts.push_back(n); combs *= n;
      first[b] = keep.size();
      for (int o = 0; o < n; o++){ ls >> s; seq += seq_of(s); opt_off.push_back((int32_t)seq.size()); keep.push_back(1); }
    }
    hap_off.push_back(hap_off.back() + combs); read_off.push_back(0);
    for (int b = 0; b < 3; b++){
      std::getline(in, line);
      std::istringstream ls(line);
      int idx = 0, n = 0;
      ls >> word >> idx >> n;
      if (word != "remove" || idx != b || !ls){ fprintf(stderr, "bad remove line: %s\n", line.c_str()); return 2; }
      for (int i = 0; i < n; i++){ int o = 0; ls >> o; keep[first[b] + (size_t)o] = 0; }
    }
    for (int b = 0; b < 3; b++){
      std::getline(in, line);
      std::istringstream ls(line);
      int idx = 0, n = 0; std::string s;
      ls >> word >> idx >> n;
      if (word != "add" || idx != b || !ls){ fprintf(stderr, "bad add line: %s\n", line.c_str()); return 2; }
      for (int i = 0; i < n; i++){ ls >> s; add_seq += seq_of(s); add_seq_off.push_back((int32_t)add_seq.size()); }
      add_off.push_back((int32_t)add_seq_off.size() - 1);
    }
  }
  hipstr_batch_t b; memset(&b, 0, sizeof b);
  b.n_loci = (int32_t)names.size();
  b.blk_start = blk_start.data(); b.blk_end = blk_end.data(); b.blk_nopts = blk_nopts.data(); b.period = period.data(); b.stutter = stutter.data();
  b.opt_off = opt_off.data(); b.seq = seq.c_str(); b.hap_off = hap_off.data(); b.read_off = read_off.data();
  hipstr_alleles_request_t rq; memset(&rq, 0, sizeof rq);
  rq.pooled = &b; rq.keep = keep.data(); rq.keep_blocks = 7u; rq.add_off = add_off.data(); rq.add_seq_off = add_seq_off.data(); rq.add_seq = add_seq.c_str();
  std::string err; int64_t c64[4], c4[4];
  hipstr_alleles* full = hipstr_al::apply_host(&rq, 64, c64, err);
  if (!full){ fprintf(stderr, "refused: %s\n", err.c_str()); return 1; }
  hipstr_alleles* cut = hipstr_al::apply_host(&rq, 4, c4, err);
  if (!cut){ fprintf(stderr, "refused: %s\n", err.c_str()); return 1; }
  if (full->mapping != cut->mapping || full->realign != cut->realign || full->seq != cut->seq || full->opt_off != cut->opt_off || full->blk_nopts != cut->blk_nopts ||
      full->h2a[0] != cut->h2a[0] || full->h2a[1] != cut->h2a[1] || full->h2a[2] != cut->h2a[2] || c4[3] <= c64[3]){
    fprintf(stderr, "the 4-bit hash changes the result, or compares no more bytes (%lld against %lld)\n", (long long)c4[3], (long long)c64[3]);
    return 1;
  }
  // a refusal leaves through the same door: keep drops option 0
  keep[0] = 0;
  if (hipstr_al::apply_host(&rq, 64, c64, err) || err.find("keep drops option 0") == std::string::npos){ fprintf(stderr, "not refused\n"); return 1; }
  for (size_t l = 0; l < names.size(); l++){
    printf("case %s nopts %d %d %d map", names[l].c_str(), full->blk_nopts[3*l], full->blk_nopts[3*l+1], full->blk_nopts[3*l+2]);
    for (int k = hap_off[l]; k < hap_off[l+1]; k++) printf(" %d", full->mapping[(size_t)k]);
    printf(" realign");
    for (int k = full->hap_off[l]; k < full->hap_off[l+1]; k++) printf(" %d", (int)full->realign[(size_t)k]);
    printf("\n");
  }
  delete full; delete cut;
  return 0;
}
