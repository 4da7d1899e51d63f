// flank_fused_test.cpp — the flank sweeps' fused column pass (hipstr_amd/csrc/flank_sweep_step.h, the text band_sweep_coop runs on the
// device) as a host program: random flank blocks of 1-40 rows x 1-20 read columns, cut into bands of 1-15 rows, swept band by band with
// the kernel's pass structure — column 0 initialised, then one top-down pass per column, two values per row, the last pass without its
// rows — and compared with a plain full-matrix evaluation of the recurrence in the reference's order (HapAligner.cpp:33-42, :123-153):
// every last-column M, every last-row M, and every (M, D) pair a band hands to the band below (columns 0 .. n-2: what the band below
// reads; the pair of the last column feeds nothing).  memcmp, 0 mismatches.
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined tests/cpp/flank_fused_test.cpp -I hipstr_amd/csrc
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "flank_sweep_step.h"

static const double IMP = -1000000000.0;      // HS_IMPOSSIBLE (layout.h), HapAligner.cpp:20

struct Problem {
  int R, n;                                   // rows after the block's first row, read columns
  bool lead;                                  // first row: matrix row 0 (running sum of log P(correct)) or the row behind an STR block (mr)
  std::vector<double> blc, blw, mr;           // per column: log P(correct), log P(error); STR-row values
  std::vector<int> rd;                        // per column: read base
  std::vector<int> hap;                       // per row 0..R: haplotype base
  std::vector<double> m2m, m2i;               // per row 1..R (index r): transition logs of the row's class
};

static double emit(const Problem& p, int r, int j){ return p.rd[j] == p.hap[r] ? p.blc[j] : p.blw[j]; }

// The whole matrix, every cell from the reference's own expression.
struct Full { std::vector<double> M, I, D; double side_prob; };
static Full full_matrix(const Problem& p){
  const int n = p.n, R = p.R;
  Full f; f.M.assign((size_t)(R + 1)*n, 0.0); f.I = f.M; f.D = f.M;
  double left = 0.0;
  for (int j = 0; j < n; j++){
    if (p.lead){ f.M[j] = emit(p, 0, j) + left; left += p.blc[j]; }
    else f.M[j] = (j == 0) ? emit(p, 0, j) : emit(p, 0, j) + p.mr[j - 1];
    f.I[j] = IMP; f.D[j] = IMP;
  }
  f.side_prob = left;
  for (int r = 1; r <= R; r++){
    double* M = &f.M[(size_t)r*n]; double* I = &f.I[(size_t)r*n]; double* D = &f.D[(size_t)r*n];
    const double* Mu = M - n; const double* Du = D - n;
    M[0] = emit(p, r, 0);
    I[0] = p.blc[0];
    D[0] = std::max(Du[0] + T_D2D, Mu[0] + T_D2M);
    for (int j = 1; j < n; j++){
      const double p0 = I[j - 1] + p.m2i[r], p1 = Mu[j - 1] + p.m2m[r], p2 = Du[j - 1] + p.m2i[r];      // (match-to-del and match-to-ins: one table)
      M[j] = emit(p, r, j) + std::max(p0, std::max(p1, p2));
      I[j] = p.blc[j] + std::max(Mu[j - 1] + T_I2M, I[j - 1] + T_I2I);
      D[j] = std::max(Mu[j] + T_D2M, Du[j] + T_D2D);
    }
  }
  return f;
}

// One band (rows row0 .. row0+nr-1) with the kernel's pass structure.  top: the (M, D) pairs handed in per column (bands after the
// first); bot: those handed out.  lt[r]: M of the last column; rowp[j]: M of the band's last row.
struct Pair { double M, D; };
static void sweep_band(const Problem& p, int row0, int nr, bool first, const std::vector<Pair>& top, std::vector<Pair>& bot,
                       std::vector<double>& lt, std::vector<double>& rowp, double* side_prob){
  const int n = p.n, nmax = p.n;
  std::vector<double> Mp(nr), Ip(nr);
  for (int r = 0; r < nr; r++){ Mp[r] = emit(p, row0 + r, 0); Ip[r] = p.blc[0]; }
  double pre = 0.0, topM = 0.0;
  if (first){
    const double e0 = emit(p, 0, 0);
    if (p.lead){ topM = e0 + pre; pre += p.blc[0]; if (n == 1) *side_prob = pre; }
    else topM = e0;
    if (n == 1) lt[0] = topM;
  }
  if (n == 1){
    for (int r = 0; r < nr; r++) lt[row0 + r] = Mp[r];
    rowp[0] = Mp[nr - 1];
  }
  bot.assign(nmax, Pair{0.0, 0.0});
  for (int j = 0; j < nmax; j++){
    const bool rows_pass = j + 1 < nmax;
    double upM, upD;
    if (first){
      upM = topM; upD = IMP;
      if (rows_pass){
        const double e0 = emit(p, 0, j + 1);
        if (p.lead){ topM = e0 + pre; pre += p.blc[j + 1]; if (j + 2 == n) *side_prob = pre; }
        else topM = e0 + p.mr[j];
        if (j + 2 == n) lt[0] = topM;
      }
    } else { upM = top[j].M; upD = top[j].D; }
    if (rows_pass){
      const double lastM = Mp[nr - 1];
      double X = upM + T_D2M, A = upM + p.m2m[row0];
      for (int r = 0; r < nr; r++)
        hs_fused_row_step(X, A, upD, Mp[r], Ip[r], emit(p, row0 + r, j + 1), p.blc[j + 1], p.m2i[row0 + r], r + 1 < nr, r + 1 < nr ? p.m2m[row0 + r + 1] : 0.0);
      upM = lastM;
    }
    bot[j] = Pair{upM, upD};
    if (j + 1 < n) rowp[j] = upM;
    if (j + 2 == n){
      for (int r = 0; r < nr; r++) lt[row0 + r] = Mp[r];
      rowp[n - 1] = Mp[nr - 1];
    }
  }
}

static long g_cells = 0, g_bad = 0;
static void same(const double& a, const double& b, const char* what, const Problem& p, int r, int j){
  g_cells++;
  if (memcmp(&a, &b, sizeof(double)) != 0){
    if (g_bad++ < 10) printf("MISMATCH %s: rows %d cols %d %s at row %d col %d: %.17g != %.17g\n", what, p.R, p.n, p.lead ? "lead" : "trail", r, j, a, b);
  }
}

static void run_case(std::mt19937_64& rng, int R, int n, bool lead){
  std::uniform_real_distribution<double> lp(-9.0, -1e-4);
  Problem p; p.R = R; p.n = n; p.lead = lead;
  p.blc.resize(n); p.blw.resize(n); p.mr.resize(n); p.rd.resize(n); p.hap.resize(R + 1); p.m2m.assign(R + 1, 0.0); p.m2i.assign(R + 1, 0.0);
  for (int j = 0; j < n; j++){ p.blc[j] = lp(rng) * 0.01; p.blw[j] = lp(rng); p.mr[j] = lp(rng) * 7.0; p.rd[j] = (int)(rng() % 4); }
  double cm[10], ci[10];
  for (int c = 0; c < 10; c++){ cm[c] = lp(rng) * 0.01; ci[c] = lp(rng); }      // transition classes (homopolymer lengths)
  for (int r = 0; r <= R; r++){ p.hap[r] = (int)(rng() % 4); const int c = (int)(rng() % 10); p.m2m[r] = cm[c]; p.m2i[r] = ci[c]; }
  const Full f = full_matrix(p);
  // bands of 1-15 rows, three cuts per problem: random, as tall as possible, one row each
  for (int cut = 0; cut < 3; cut++){
    std::vector<double> lt(R + 1, 0.0), rowp(n, 0.0); double side_prob = 0.0;
    std::vector<Pair> top, bot;
    int row0 = 1;
    while (row0 <= R){
      const int left = R - row0 + 1;
      const int nr = cut == 0 ? 1 + (int)(rng() % std::min(15, left)) : cut == 1 ? std::min(15, left) : 1;
      sweep_band(p, row0, nr, row0 == 1, top, bot, lt, rowp, &side_prob);
      const int last = row0 + nr - 1;
      for (int j = 0; j + 1 < n; j++){
        same(bot[j].M, f.M[(size_t)last*n + j], "handed M", p, last, j);
        same(bot[j].D, f.D[(size_t)last*n + j], "handed D", p, last, j);
      }
      top = bot; row0 += nr;
    }
    for (int r = 0; r <= R; r++) same(lt[r], f.M[(size_t)r*n + n - 1], "last-column M", p, r, n - 1);
    for (int j = 0; j < n; j++) same(rowp[j], f.M[(size_t)R*n + j], "last-row M", p, R, j);
    if (lead) same(side_prob, f.side_prob, "side_prob", p, 0, n - 1);
  }
}

int main(){
  std::mt19937_64 rng(20240607);
  for (int rep = 0; rep < 3; rep++)
    for (int R = 1; R <= 40; R++)
      for (int n = 1; n <= 20; n++){ run_case(rng, R, n, false); run_case(rng, R, n, true); }
  printf("%ld values compared, %ld mismatches\n%s\n", g_cells, g_bad, g_bad ? "FAILED" : "ok");
  return g_bad ? 1 : 0;
}
