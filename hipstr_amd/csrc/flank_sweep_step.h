// flank_sweep_step.h — the row step of the flank blocks' fused column pass (band_sweep_coop, hmm_kernels.hip), as text that a host
// program can run too (tests/cpp/flank_fused_test.cpp).
//
// The flank recurrence (HapAligner.cpp:144-153), row r = haplotype position, column j = read index:
//   M[r][j] = e[r][j] + max(I[r][j-1] + m2i[r], max(M[r-1][j-1] + m2m[r], D[r-1][j-1] + m2d[r]))       m2d == m2i
//   I[r][j] = blc[j]  + max(M[r-1][j-1] + T_I2M, I[r][j-1] + T_I2I)
//   D[r][j] = max(M[r-1][j] + T_D2M, D[r-1][j] + T_D2D)
// Pass j over a band of rows walks top-down once and turns column j's (M, I) of every row into column j + 1's.  Going into row r it
// holds, of the row above in column j (from the band above, or from the block's first row, for the band's first row), D[r-1][j] and
// the two sums the row takes from M[r-1][j] — X = M[r-1][j] + T_D2M and A = M[r-1][j] + m2m[r] — and the row's own M[r][j] and
// I[r][j]; it forms D[r][j], I[r][j+1] and M[r][j+1] — every sum and maximum the reference forms, on the same operands, two of them
// shared: M[r-1][j] + T_D2M is also M[r-1][j] + T_I2M (one constant, AlignmentModel.h:7-10), and adding m2i after the maximum of I and D
// is adding it to each before (rounding is monotone, m2d and m2i are one number) — and leaves D[r][j] and the row below's two sums of
// M[r][j] behind.  The sums of M[r][j] are formed BEFORE M[r][j+1] is written: the old value has no use after them, so the new one takes
// its register (formed by the row below instead, M[r][j] would have to outlive M[r][j+1]: two register moves per cell).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define HS_STEP_FN __host__ __device__ __forceinline__
#else
#define HS_STEP_FN inline
#endif

namespace {

constexpr double T_I2I = -1.0, T_I2M = -0.4586751453870818910216436;   // AlignmentModel.h:7-10
constexpr double T_D2D = -1.0, T_D2M = -0.4586751453870818910216436;
static_assert(T_I2M == T_D2M, "the row step forms M[r-1][j] + T once for I and D");

// M, I: in M[r][j], I[r][j]; out M[r][j+1], I[r][j+1].  e_next = e[r][j+1], blc_next = blc[j+1].  more: a row of the band follows,
// m2m_below is its m2m (not read otherwise).
HS_STEP_FN void hs_fused_row_step(double& X, double& A, double& upD, double& M, double& I, double e_next, double blc_next, double m2i,
                                  bool more, double m2m_below){
  const double nD = fmax(X, upD + T_D2D);                      // D[r][j]
  const double Q = fmax(I, upD);
  const double newI = blc_next + fmax(X, I + T_I2I);           // I[r][j+1]
  const double best = fmax(A, Q + m2i);
  if (more){ X = M + T_D2M; A = M + m2m_below; }
  M = e_next + best;                                           // M[r][j+1]
  I = newI; upD = nD;
}

}  // namespace
