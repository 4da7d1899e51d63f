// float_lse.h — the reference's float log-sum-exp primitives, one copy for host and gfx950 device code.
//
// Why: every number the library produces passes through four bit-trick float functions of the reference (fastonebigheader.h):
//   fasterexp / fasterlog  serve fast_log_sum_exp(vector) (mathops.cpp:97-106): forward kernels, combine, traceback, expanded tables;
//   fastexp (through fastpow2) / fastlog  serve fast_log_sum_exp(a, b) (mathops.cpp:86-95): posteriors, GL / PL / GLDIFF, stutter EM.
// Bit-for-bit parity of every later stage rests on them, so they live here once and the suite runs exactly this code: on the device
// through hipstr_debug_float_fn / _fast_lse2 / _fast_lse_vec, on the host through their _host forms (include/hipstr_hmm_debug.h).
// tests/test_float_lse.py pins the host side to the oracle and the oracle to the compiled reference over every float argument the
// functions can receive; tests/test_float_lse_gpu.py pins the device side to the oracle over the same ranges.
//
// Device side: every operation is a round-to-nearest intrinsic (__fmul_rn ...: nothing can be contracted or reassociated) and the two
// float divisions are f_div_tab's reciprocal sequence.  Host side: plain float operations and `/`.  Compile with -ffp-contract=off (the
// library's flag): the host expressions must be rounded operation by operation, as the reference's are.
// Stand-alone: no dependency on layout.h; plain C++ when no HIP compiler reads it.
#ifndef HIPSTR_FLOAT_LSE_H_
#define HIPSTR_FLOAT_LSE_H_
#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define FL_FN static __host__ __device__ __forceinline__ __attribute__((unused))
#define FL_MEMBER __host__ __device__ __forceinline__
#else
#define FL_FN static inline __attribute__((unused))
#define FL_MEMBER inline
#endif

namespace {

FL_FN float f_from_bits(uint32_t u){ float f; memcpy(&f, &u, 4); return f; }
FL_FN uint32_t f_to_bits(float f){ uint32_t u; memcpy(&u, &f, 4); return u; }

#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
// ------------------------------------------------------------------ device
// The two float divisions of the reference's bit-trick exp2 / log (fastonebigheader.h:188-198: 27.7280233f / (4.84252568f - z), z in [0, 1];
// :320-338: 1.72587999f / (0.3520887068f + mx), mx in [0.5, 1)) as v_rcp_f32 + one Newton step + a residual correction: six instructions
// instead of the compiler's IEEE sequence (scale, reciprocal, three refinements, fmas, fixup: twice that), and the IEEE quotient for EVERY
// float denominator of both ranges — tests/test_float_lse_gpu.py::test_div_tab checks all of them on the device against the host's
// quotient.  Operands outside those ranges: never here.
FL_FN float f_div_tab(float n, float d){
  float r = __builtin_amdgcn_rcpf(d);
  r = __fmaf_rn(__fmaf_rn(-d, r, 1.0f), r, r);
  const float q = __fmul_rn(n, r);
  return __fmaf_rn(__fmaf_rn(-d, q, n), r, q);
}
FL_FN float f_fasterexp(float p){           // fastonebigheader.h:206-218
  const float y = __fmul_rn(1.442695040f, p);
  const float c = (y < -126.0f) ? -126.0f : y;
  return __uint_as_float((uint32_t)__fmul_rn(8388608.0f, __fadd_rn(c, 126.94269504f)));
}
FL_FN float f_fasterlog(float x){           // fastonebigheader.h:348-358
  float y = (float)__float_as_uint(x);
  y = __fmul_rn(y, 8.2629582881927490e-8f);
  return __fsub_rn(y, 87.989971088f);
}
FL_FN float f_fastpow2(float p){            // fastonebigheader.h:188-198
  const float offset = (p < 0.0f) ? 1.0f : 0.0f;
  const float clipp = (p < -126.0f) ? -126.0f : p;
  const int w = (int)clipp;
  const float z = __fadd_rn(__fsub_rn(clipp, (float)w), offset);
  const float t = __fsub_rn(__fadd_rn(__fadd_rn(clipp, 121.2740575f), f_div_tab(27.7280233f, __fsub_rn(4.84252568f, z))), __fmul_rn(1.49012907f, z));
  return __uint_as_float((uint32_t)__fmul_rn(8388608.0f, t));
}
FL_FN float f_fastexp(float p){ return f_fastpow2(__fmul_rn(1.442695040f, p)); }   // fastonebigheader.h:200-204
FL_FN float f_fastlog(float x){             // fastonebigheader.h:320-338
  const uint32_t vi = __float_as_uint(x);
  const float mx = __uint_as_float((vi & 0x007FFFFFu) | 0x3f000000u);
  float y = (float)vi;
  y = __fmul_rn(y, 1.1920928955078125e-7f);
  const float l2 = __fsub_rn(__fsub_rn(__fsub_rn(y, 124.22551499f), __fmul_rn(1.498030302f, mx)),
                             f_div_tab(1.72587999f, __fadd_rn(0.3520887068f, mx)));
  return __fmul_rn(0.69314718f, l2);
}
// the pair term of fast_log_sum_exp(a, b): fastlog(1 + fastexp(p)), p = the float cast of lo - hi
FL_FN float f_lse2_term(float p){ return f_fastlog(__fadd_rn(1.0f, f_fastexp(p))); }
#else
// ------------------------------------------------------------------ host: the reference's expressions, operation by operation
FL_FN float f_div_tab(float n, float d){ return n / d; }
FL_FN float f_fasterexp(float p){           // fastonebigheader.h:206-218
  const float y = 1.442695040f * p;
  const float c = (y < -126.0f) ? -126.0f : y;
  const float z = c + 126.94269504f;
  return f_from_bits((uint32_t)(8388608.0f * z));
}
FL_FN float f_fasterlog(float x){           // fastonebigheader.h:348-358
  float y = (float)f_to_bits(x);
  y = y * 8.2629582881927490e-8f;
  return y - 87.989971088f;
}
FL_FN float f_fastpow2(float p){            // fastonebigheader.h:188-198
  const float offset = (p < 0) ? 1.0f : 0.0f;
  const float clipp = (p < -126) ? -126.0f : p;
  const int w = (int)clipp;
  const float z = clipp - w + offset;
  return f_from_bits((uint32_t)((1 << 23) * (clipp + 121.2740575f + f_div_tab(27.7280233f, 4.84252568f - z) - 1.49012907f * z)));
}
FL_FN float f_fastexp(float p){ return f_fastpow2(1.442695040f * p); }             // fastonebigheader.h:200-204
FL_FN float f_fastlog(float x){             // fastonebigheader.h:320-338
  const uint32_t vi = f_to_bits(x);
  const float mx = f_from_bits((vi & 0x007FFFFF) | 0x3f000000);
  float y = (float)vi;
  y *= 1.1920928955078125e-7f;
  return 0.69314718f * (y - 124.22551499f - 1.498030302f * mx - f_div_tab(1.72587999f, 0.3520887068f + mx));
}
FL_FN float f_lse2_term(float p){ return f_fastlog(1 + f_fastexp(p)); }
#endif

// fast_log_sum_exp(a, b) (mathops.cpp:86-95); thr = LOG_THRESH = ln 0.001.  The test is strict: diff == thr takes the float path.
FL_FN double fast_lse2(double a, double b, double thr){
  const double hi = a > b ? a : b, lo = a > b ? b : a;
  const double diff = lo - hi;
  return diff < thr ? hi : hi + (double)f_lse2_term((float)diff);
}

// streaming form of fast_log_sum_exp(vector) (mathops.cpp:97-106): pass 0 finds the max,
// pass 1 accumulates.  The float terms are summed in double, which is exact for any order.
struct Lse {
  double mx, tot;
  FL_MEMBER void start(int pass, double first){ if (pass == 0) mx = first; else tot = 0.0; }
  FL_MEMBER void push(int pass, double v, double thr){
    if (pass == 0) mx = fmax(mx, v);
    else { const double d = v - mx; if (d > thr) tot += (double)f_fasterexp((float)d); }
  }
  FL_MEMBER double finish() const { return mx + (double)f_fasterlog((float)tot); }
};

}  // namespace

#endif
