// valu_microbench.hip — issue cost of the instruction classes the HMM kernels are made of, measured on the device (gfx950):
// a wavefront runs long straight-line runs of ONE instruction over 8 independent register chains (no dependent-issue stalls) and
// times them with s_memtime; 1, 2, 3 and 4 wavefronts per SIMD show whether the cost is issue (scales) or latency (hides) — 3 and 4 are
// what a kernel of 168 or of 128 registers runs at: the ratio is what the flank sweeps' fourth wavefront can win.
//   hipcc --offload-arch=gfx950 -O2 tools/valu_microbench.hip -o tools/valu_microbench && tools/valu_microbench > profiles/rNN_valu_microbench.json
// The numbers feed tools/sq_counters.py (pipe occupancy from the ISA mix) instead of an assumed 4 cycles for everything.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#include <string>

#define REP8(x) x x x x x x x x
#define BODY_F64(op) \
  asm volatile(REP8(op " %0, %0, %8\n\t" op " %1, %1, %8\n\t" op " %2, %2, %8\n\t" op " %3, %3, %8\n\t" op " %4, %4, %8\n\t" op " %5, %5, %8\n\t" op " %6, %6, %8\n\t" op " %7, %7, %8\n\t") \
    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(c));
#define BODY_B32(op) \
  asm volatile(REP8(op " %0, %0, %8\n\t" op " %1, %1, %8\n\t" op " %2, %2, %8\n\t" op " %3, %3, %8\n\t" op " %4, %4, %8\n\t" op " %5, %5, %8\n\t" op " %6, %6, %8\n\t" op " %7, %7, %8\n\t") \
    : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci));

enum { OP_ADD_F64, OP_MAX_F64, OP_FMA_F64, OP_ADD_F32, OP_ADD_U32, OP_MOV_B32, OP_CNDMASK, OP_CMP_F64, OP_CMP_U32, OP_READLANE, OP_DPP_MOV, OP_MIX_F64_B32, OP_DS_READ_B64, OP_CVT_F32_F64, OP_AND_B32, OP_LSHL_ADD, OP_CMP_CND_VCC, OP_CND_E64, OP_ADD_F64_SGPR, OP_CMP_CND_E64, N_OPS };
static const char* kNames[N_OPS] = { "v_add_f64", "v_max_f64", "v_fma_f64", "v_add_f32", "v_add_u32", "v_mov_b32", "v_cndmask_b32", "v_cmp_gt_f64", "v_cmp_eq_u32",
  "v_readlane_b32", "v_mov_b32_dpp", "v_add_f64+v_mov_b32 (pair)", "ds_read_b64", "v_cvt_f32_f64", "v_and_b32", "v_lshl_add_u32", "v_cmp_eq_u32 vcc + 2 x v_cndmask_b32_e32 (per instruction)", "v_cndmask_b32_e64 (sgpr-pair mask)", "v_add_f64 with an SGPR-pair operand", "v_cmp_eq_u32_e64 s[..] + 2 x v_cndmask_b32_e64 (per instruction)" };

template <int OP>
__global__ void bench(uint64_t* out, int iters, double seed){
  __shared__ double lds[1024];
  lds[threadIdx.x & 1023] = seed;
  double a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5, a6 = seed + 6, a7 = seed + 7, c = 1.0000001;
  uint32_t b0 = threadIdx.x, b1 = b0 + 1, b2 = b0 + 2, b3 = b0 + 3, b4 = b0 + 4, b5 = b0 + 5, b6 = b0 + 6, b7 = b0 + 7, ci = 3;
  __syncthreads();
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  for (int i = 0; i < iters; i++){
    if (OP == OP_ADD_F64) BODY_F64("v_add_f64")
    if (OP == OP_MAX_F64) BODY_F64("v_max_f64")
    if (OP == OP_FMA_F64)
      asm volatile(REP8("v_fma_f64 %0, %0, %8, %8\n\tv_fma_f64 %1, %1, %8, %8\n\tv_fma_f64 %2, %2, %8, %8\n\tv_fma_f64 %3, %3, %8, %8\n\tv_fma_f64 %4, %4, %8, %8\n\tv_fma_f64 %5, %5, %8, %8\n\tv_fma_f64 %6, %6, %8, %8\n\tv_fma_f64 %7, %7, %8, %8\n\t")
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(c));
    if (OP == OP_ADD_F32) BODY_B32("v_add_f32")
    if (OP == OP_ADD_U32) BODY_B32("v_add_u32")
    if (OP == OP_AND_B32) BODY_B32("v_and_b32")
    if (OP == OP_MOV_B32)
      asm volatile(REP8("v_mov_b32 %0, %8\n\tv_mov_b32 %1, %8\n\tv_mov_b32 %2, %8\n\tv_mov_b32 %3, %8\n\tv_mov_b32 %4, %8\n\tv_mov_b32 %5, %8\n\tv_mov_b32 %6, %8\n\tv_mov_b32 %7, %8\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci));
    if (OP == OP_CNDMASK)
      asm volatile(REP8("v_cndmask_b32 %0, %0, %8, vcc\n\tv_cndmask_b32 %1, %1, %8, vcc\n\tv_cndmask_b32 %2, %2, %8, vcc\n\tv_cndmask_b32 %3, %3, %8, vcc\n\tv_cndmask_b32 %4, %4, %8, vcc\n\tv_cndmask_b32 %5, %5, %8, vcc\n\tv_cndmask_b32 %6, %6, %8, vcc\n\tv_cndmask_b32 %7, %7, %8, vcc\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci) : "vcc");
    if (OP == OP_CMP_F64)
      asm volatile(REP8("v_cmp_gt_f64 vcc, %0, %8\n\tv_cmp_gt_f64 vcc, %1, %8\n\tv_cmp_gt_f64 vcc, %2, %8\n\tv_cmp_gt_f64 vcc, %3, %8\n\tv_cmp_gt_f64 vcc, %4, %8\n\tv_cmp_gt_f64 vcc, %5, %8\n\tv_cmp_gt_f64 vcc, %6, %8\n\tv_cmp_gt_f64 vcc, %7, %8\n\t")
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(c) : "vcc");
    if (OP == OP_CMP_U32)
      asm volatile(REP8("v_cmp_eq_u32 vcc, %0, %8\n\tv_cmp_eq_u32 vcc, %1, %8\n\tv_cmp_eq_u32 vcc, %2, %8\n\tv_cmp_eq_u32 vcc, %3, %8\n\tv_cmp_eq_u32 vcc, %4, %8\n\tv_cmp_eq_u32 vcc, %5, %8\n\tv_cmp_eq_u32 vcc, %6, %8\n\tv_cmp_eq_u32 vcc, %7, %8\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci) : "vcc");
    if (OP == OP_READLANE)
      asm volatile(REP8("v_readlane_b32 s20, %0, 3\n\tv_readlane_b32 s21, %1, 3\n\tv_readlane_b32 s22, %2, 3\n\tv_readlane_b32 s23, %3, 3\n\tv_readlane_b32 s24, %4, 3\n\tv_readlane_b32 s25, %5, 3\n\tv_readlane_b32 s26, %6, 3\n\tv_readlane_b32 s27, %7, 3\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci) : "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27");
    if (OP == OP_DPP_MOV)
      asm volatile(REP8("v_mov_b32_dpp %0, %8 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %1, %8 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %2, %8 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %3, %8 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %4, %8 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %5, %8 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %6, %8 wave_shr:1 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %7, %8 wave_shr:1 row_mask:0xf bank_mask:0xf\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci));
    if (OP == OP_MIX_F64_B32)
      asm volatile(REP8("v_add_f64 %0, %0, %8\n\tv_mov_b32 %4, %9\n\tv_add_f64 %1, %1, %8\n\tv_mov_b32 %5, %9\n\tv_add_f64 %2, %2, %8\n\tv_mov_b32 %6, %9\n\tv_add_f64 %3, %3, %8\n\tv_mov_b32 %7, %9\n\t")
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(c), "v"(ci));
    if (OP == OP_DS_READ_B64){
      const uint32_t addr = (threadIdx.x & 63) * 8;
      asm volatile(REP8("ds_read_b64 %0, %8\n\tds_read_b64 %1, %8 offset:512\n\tds_read_b64 %2, %8 offset:1024\n\tds_read_b64 %3, %8 offset:1536\n\tds_read_b64 %4, %8 offset:2048\n\tds_read_b64 %5, %8 offset:2560\n\tds_read_b64 %6, %8 offset:3072\n\tds_read_b64 %7, %8 offset:3584\n\t") "s_waitcnt lgkmcnt(0)\n\t"
        : "=v"(a0), "=v"(a1), "=v"(a2), "=v"(a3), "=v"(a4), "=v"(a5), "=v"(a6), "=v"(a7) : "v"(addr) : "memory");
    }
    if (OP == OP_CVT_F32_F64)
      asm volatile(REP8("v_cvt_f32_f64 %0, %8\n\tv_cvt_f32_f64 %1, %8\n\tv_cvt_f32_f64 %2, %8\n\tv_cvt_f32_f64 %3, %8\n\tv_cvt_f32_f64 %4, %8\n\tv_cvt_f32_f64 %5, %8\n\tv_cvt_f32_f64 %6, %8\n\tv_cvt_f32_f64 %7, %8\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(c));
    if (OP == OP_CMP_CND_VCC)      // 8 x (1 cmp + 2 cndmask) = 24 instructions per asm line, x8 below: counted as 64 by run(): corrected in main
      asm volatile(REP8("v_cmp_eq_u32 vcc, %0, %8\n\tv_cndmask_b32 %1, %1, %2, vcc\n\tv_cndmask_b32 %3, %3, %4, vcc\n\tv_cmp_eq_u32 vcc, %5, %8\n\tv_cndmask_b32 %6, %6, %7, vcc\n\tv_cndmask_b32 %2, %2, %4, vcc\n\tv_cmp_eq_u32 vcc, %7, %8\n\tv_cndmask_b32 %4, %4, %1, vcc\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci) : "vcc");
    if (OP == OP_CND_E64)
      asm volatile(REP8("v_cndmask_b32_e64 %0, %0, %8, s[20:21]\n\tv_cndmask_b32_e64 %1, %1, %8, s[20:21]\n\tv_cndmask_b32_e64 %2, %2, %8, s[22:23]\n\tv_cndmask_b32_e64 %3, %3, %8, s[22:23]\n\tv_cndmask_b32_e64 %4, %4, %8, s[20:21]\n\tv_cndmask_b32_e64 %5, %5, %8, s[20:21]\n\tv_cndmask_b32_e64 %6, %6, %8, s[22:23]\n\tv_cndmask_b32_e64 %7, %7, %8, s[22:23]\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci) : "s20", "s21", "s22", "s23");
    if (OP == OP_ADD_F64_SGPR)
      asm volatile(REP8("v_add_f64 %0, %0, s[20:21]\n\tv_add_f64 %1, %1, s[20:21]\n\tv_add_f64 %2, %2, s[22:23]\n\tv_add_f64 %3, %3, s[22:23]\n\tv_add_f64 %4, %4, s[20:21]\n\tv_add_f64 %5, %5, s[20:21]\n\tv_add_f64 %6, %6, s[22:23]\n\tv_add_f64 %7, %7, s[22:23]\n\t")
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(c) : "s20", "s21", "s22", "s23");
    if (OP == OP_CMP_CND_E64)
      asm volatile(REP8("v_cmp_eq_u32_e64 s[20:21], %0, %8\n\tv_cndmask_b32_e64 %1, %1, %2, s[20:21]\n\tv_cndmask_b32_e64 %3, %3, %4, s[20:21]\n\tv_cmp_eq_u32_e64 s[22:23], %5, %8\n\tv_cndmask_b32_e64 %6, %6, %7, s[22:23]\n\tv_cndmask_b32_e64 %2, %2, %4, s[22:23]\n\tv_cmp_eq_u32_e64 s[24:25], %7, %8\n\tv_cndmask_b32_e64 %4, %4, %1, s[24:25]\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci) : "s20", "s21", "s22", "s23", "s24", "s25");
    if (OP == OP_LSHL_ADD)
      asm volatile(REP8("v_lshl_add_u32 %0, %0, 1, %8\n\tv_lshl_add_u32 %1, %1, 1, %8\n\tv_lshl_add_u32 %2, %2, 1, %8\n\tv_lshl_add_u32 %3, %3, 1, %8\n\tv_lshl_add_u32 %4, %4, 1, %8\n\tv_lshl_add_u32 %5, %5, 1, %8\n\tv_lshl_add_u32 %6, %6, 1, %8\n\tv_lshl_add_u32 %7, %7, 1, %8\n\t")
        : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5), "+v"(b6), "+v"(b7) : "v"(ci));
  }
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  double s = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + (double)(b0 ^ b1 ^ b2 ^ b3 ^ b4 ^ b5 ^ b6 ^ b7);
  if (s == 12345.678) out[1023] = 1;                       // keep the chains alive
  if ((threadIdx.x & 63) == 0) out[(blockIdx.x * blockDim.x + threadIdx.x) >> 6] = t1 - t0;
}

template <int OP> double run(int waves_per_simd, uint64_t* d_out, double clock_ratio){
  const int iters = 2000, threads = 256 * waves_per_simd;       // one workgroup on one CU: waves_per_simd wavefronts on each of its 4 SIMDs
  bench<OP><<<1, threads>>>(d_out, 10, 1.5);
  bench<OP><<<1, threads>>>(d_out, iters, 1.5);
  hipDeviceSynchronize();
  std::vector<uint64_t> h(threads / 64);
  hipMemcpy(h.data(), d_out, h.size() * 8, hipMemcpyDeviceToHost);
  double worst = 0;
  for (uint64_t v : h) worst = v > worst ? (double)v : worst;
  const double n_inst = (double)iters * 64.0 * waves_per_simd;   // instructions issued on ONE SIMD during the slowest wavefront's window
  return worst * clock_ratio / n_inst;
}

int main(){
  uint64_t* d_out; hipMalloc(&d_out, 1024 * 8);
  // s_memtime counts at a constant 100 MHz on gfx9 — calibrate against the shader clock with a known 4-cycle-dependent chain? No:
  // report both raw ticks and cycles using the device's reported clock rates.
  int sclk_khz = 0, wall_khz = 0;
  hipDeviceGetAttribute(&sclk_khz, hipDeviceAttributeClockRate, 0);
  hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, 0);
  // what does an s_memtime tick measure here?  time a long run with HIP events and compare
  double memtime_hz = 0;
  {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    bench<OP_ADD_F64><<<1, 256>>>(d_out, 10, 1.5);
    hipEventRecord(e0, 0);
    bench<OP_ADD_F64><<<1, 256>>>(d_out, 200000, 1.5);
    hipEventRecord(e1, 0); hipEventSynchronize(e1);
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    uint64_t ticks = 0; hipMemcpy(&ticks, d_out, 8, hipMemcpyDeviceToHost);
    memtime_hz = (double)ticks / (ms * 1e-3);
  }
  const double ratio = (double)sclk_khz * 1e3 / memtime_hz;     // shader cycles (at the nominal clock) per s_memtime tick
  printf("{\n \"device_clock_khz\": %d, \"wall_clock_attr_khz\": %d, \"memtime_hz_measured\": %.4g, \"cycles_per_tick\": %.4f, \"note\": \"cycles of ONE SIMD per wave64 instruction = slowest wavefront's s_memtime window x (shader clock / memtime clock) / instructions issued on that SIMD in the window; 8 independent register chains, 2000 x 64 instructions per wavefront\",\n \"cycles_per_wave64_instruction\": {\n", sclk_khz, wall_khz, memtime_hz, ratio);
  double r[N_OPS][4];
  static const int kWaves[4] = {1, 2, 3, 4};
#define RUN(OP) for (int w = 0; w < 4; w++) r[OP][w] = run<OP>(kWaves[w], d_out, ratio);
  RUN(OP_ADD_F64) RUN(OP_MAX_F64) RUN(OP_FMA_F64) RUN(OP_ADD_F32) RUN(OP_ADD_U32) RUN(OP_MOV_B32) RUN(OP_CNDMASK) RUN(OP_CMP_F64) RUN(OP_CMP_U32)
  RUN(OP_READLANE) RUN(OP_DPP_MOV) RUN(OP_MIX_F64_B32) RUN(OP_DS_READ_B64) RUN(OP_CVT_F32_F64) RUN(OP_AND_B32) RUN(OP_LSHL_ADD) RUN(OP_CMP_CND_VCC) RUN(OP_CND_E64) RUN(OP_ADD_F64_SGPR) RUN(OP_CMP_CND_E64)
  for (int o = 0; o < N_OPS; o++)
    printf("  \"%s\": {\"1_wave_per_simd\": %.3f, \"2_waves_per_simd\": %.3f, \"3_waves_per_simd\": %.3f, \"4_waves_per_simd\": %.3f}%s\n", kNames[o], r[o][0], r[o][1], r[o][2], r[o][3], o + 1 < N_OPS ? "," : "");
  printf(" }\n}\n");
  return 0;
}
