// device_common.h — wave primitives shared by the HIP kernels (and, through float_lse.h, the bit-exact float log-sum-exp helpers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layout.h"
#include "float_lse.h"
#include "flank_sweep_step.h"      // T_I2I, T_I2M, T_D2D, T_D2M and the flank sweeps' row step

namespace {

constexpr double IMP = HS_IMPOSSIBLE;

// ------------------------------------------------------------------ wave primitives
__device__ __forceinline__ int shr1(int old, int src){
  return __builtin_amdgcn_update_dpp(old, src, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ double shr1(double old, double src){
  const int lo = shr1(__double2loint(old), __double2loint(src));
  const int hi = shr1(__double2hiint(old), __double2hiint(src));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int rdlane(int v, int l){ return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double rdlane(double v, int l){
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ uint64_t rdlane(uint64_t v, int l){
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}
__device__ __forceinline__ int uni(int v){ return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni(int64_t v){
  return ((int64_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
__device__ __forceinline__ double uni(double v){
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ void wave_lds_sync(){
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Integer minimum / maximum over the wavefront with DPP row shifts and row broadcasts (six VALU operations and a v_readlane) instead of
// six ds_bpermute round trips: these sit on the critical path of the STR kernels' read-end sums.  A lane without a source keeps its own
// value (old = v), which min and max do not mind.
#define HS_DPP_RED(OP) \
  v = OP(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false)); /* row_shr:1 */ \
  v = OP(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false)); /* row_shr:2 */ \
  v = OP(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false)); /* row_shr:4 */ \
  v = OP(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false)); /* row_shr:8: lane 15 of every row holds the row */ \
  v = OP(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false)); /* row_bcast:15 into rows 1 and 3 */ \
  v = OP(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false)); /* row_bcast:31 into rows 2 and 3: lane 63 holds the wavefront */ \
  return __builtin_amdgcn_readlane(v, 63);
__device__ __forceinline__ int wave_min_i(int v){ HS_DPP_RED(min) }
__device__ __forceinline__ int wave_max_i(int v){ HS_DPP_RED(max) }
#undef HS_DPP_RED
// The same for doubles: two DPP moves and one FP64 operation per step.  The sum is used for log-sum-exp totals only: every term is a
// float (2^-10 <= term <= 1, LOG_THRESH = ln 0.001) converted to double, so any order of additions is exact and gives the same bits.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_d(double v, double old){
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_max_d(double v){
  v = fmax(v, dpp_d<0x111, 0xf>(v, v)); v = fmax(v, dpp_d<0x112, 0xf>(v, v)); v = fmax(v, dpp_d<0x114, 0xf>(v, v)); v = fmax(v, dpp_d<0x118, 0xf>(v, v));
  v = fmax(v, dpp_d<0x142, 0xa>(v, v)); v = fmax(v, dpp_d<0x143, 0xc>(v, v));
  return rdlane(v, 63);
}
__device__ __forceinline__ double wave_sum_d(double v){
  v += dpp_d<0x111, 0xf>(v, 0.0); v += dpp_d<0x112, 0xf>(v, 0.0); v += dpp_d<0x114, 0xf>(v, 0.0); v += dpp_d<0x118, 0xf>(v, 0.0);   // lane 15 of a row: the row
  v += dpp_d<0x142, 0xa>(v, 0.0);                    // rows 1 and 3 take lane 15 of the row before
  v += dpp_d<0x143, 0xc>(v, 0.0);                    // rows 2 and 3 take lane 31: lane 63 holds the wavefront
  return rdlane(v, 63);
}

// (the bit-exact float approximations f_fasterexp / f_fasterlog and the streaming Lse: float_lse.h)

__device__ __forceinline__ double emit(uint8_t r, uint8_t c, double2 q){ return r == c ? q.x : q.y; }

}  // namespace
