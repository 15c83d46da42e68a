// Issue cost of single VALU instructions at the occupancy of the
// register-resident flooding kernel: every CU holds W waves
// per SIMD (default 2; workgroups of 256 threads sized by their LDS request so
// that exactly W fit a CU), each wave issues eight independent chains of one
// instruction from registers, no memory in the timed region. Per instruction,
// in shader cycles (s_memtime) per wave64 instruction and SIMD:
//   side_by_side          window pass: every wave issues until 4 M cycles have
//                         passed, so the W waves of a SIMD issue side by side
//                         throughout, as in a persistent kernel; 1 / (sum of
//                         the SIMD's waves' instructions per cycle), median of
//                         three launches. The figure to price a kernel with.
//   slowest_wave          fixed-work pass (trips x 256 steps per wave, median of
//                         five launches after a warm-up): (longest wave's
//                         time) / (instructions of the W waves of a SIMD). The
//                         waves do not share the issue evenly: the older one
//                         finishes first and the younger one runs its rest
//                         alone, so this includes a single-wave tail
//   cycles_per_inst_simd  the same from the mean over waves
//   kernel_ms             the fixed-work launch by HIP events
// With W = 1 the figures are one wave's own issue interval.
//
// build: hipcc --offload-arch=gfx950 -O2 -o valu_rates valu_rates.hip
// run:   ./valu_rates [waves per SIMD = 2] [loop trips = 1024, of 256 steps]   (JSON lines)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#define CHECK(x)                                                              \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

enum Op {
  ADD_F64, MUL_F64, MIN_F64, MAX_F64, CMP_EQ_F64_CNDMASK, CVT_F64_F32, CVT_F32_F64, MUL_ABS_F64_CVT_F32,
  ADD_F32, MIN_F32, MAX_F32, MIN3_F32, MED3_F32, AND_B32, MIN_U32, MAX_U32, MIN3_U32, MED3_U32, BITOP3_B32, CNDMASK_VCC, MOV_B32, MOV_ROW_ROR, VALU_THEN_DPP,
  VALU_NOP_PAIR,
  OR_B32_ROW_ROR, AND_B32_ROW_ROR, ADD_F32_ROW_ROR, MOV_B64, LSHLREV_B32, LSHRREV_B32, CNDMASK_ALONE, CMP_EQ_F64_VCC,
  CMP_EQ_F64_SGPR, BFI_B32, XOR_B32, CMP_CLASS_F64_VCC, CMP_CLASS_F64_SGPR, MUL_F64_CVT_F32_BITOP3,
  CMP_CLASS_F32_VCC, CMP_CLASS_F32_SGPR, CVT_F32_F64_MIN3_U32, MUL_ABS_F64_CVT_F32_INDEP, NUM_OPS
};
struct OpInfo { const char* name; int inst_per_step; };   // instructions per chain step
static const OpInfo kOps[NUM_OPS] = {
    {"v_add_f64", 1}, {"v_mul_f64", 1}, {"v_min_f64", 1}, {"v_max_f64", 1},
    {"v_cmp_eq_f64 + v_cndmask_b32 (compiler's pair, via SGPRs)", 2},
    {"v_cvt_f64_f32", 1}, {"v_cvt_f32_f64", 1}, {"v_mul_f64 |x| + v_cvt_f32_f64 (dependent pair)", 2},
    {"v_add_f32", 1}, {"v_min_f32", 1}, {"v_max_f32", 1}, {"v_min3_f32", 1}, {"v_med3_f32", 1},
    {"v_and_b32", 1}, {"v_min_u32", 1}, {"v_max_u32", 1}, {"v_min3_u32", 1}, {"v_med3_u32", 1},
    {"v_bitop3_b32", 1}, {"v_cmp_eq_u32 + v_cndmask_b32 (vcc)", 2}, {"v_mov_b32", 1},
    {"v_mov_b32 row_ror (source not written in the loop)", 1},
    {"v_add_u32 ; s_nop 1 ; v_mov_b32 row_ror of its result (pair)", 2},
    {"v_add_u32 ; s_nop 1 ; v_mov_b32 of another register (pair)", 2},
    {"v_or_b32 row_ror (DPP source not written in the loop, other operand zero)", 1},
    {"v_and_b32 row_ror (DPP source not written in the loop, other operand all ones)", 1},
    {"v_add_f32 row_ror (DPP source not written in the loop, added to the chain)", 1},
    {"v_mov_b64", 1}, {"v_lshlrev_b32 (by a constant)", 1}, {"v_lshrrev_b32 (by a constant)", 1},
    {"v_cndmask_b32 alone (mask in an SGPR pair set before the loop)", 1},
    {"v_cmp_eq_f64 alone, into vcc", 1}, {"v_cmp_eq_f64 alone, into an SGPR pair", 1},
    {"v_bfi_b32", 1}, {"v_xor_b32", 1},
    {"v_cmp_class_f64 alone, into vcc", 1}, {"v_cmp_class_f64 alone, into an SGPR pair", 1},
    {"v_mul_f64 + v_cvt_f32_f64 + v_bitop3_b32 (dependent triple)", 3},
    {"v_cmp_class_f32 alone, into vcc", 1}, {"v_cmp_class_f32 alone, into an SGPR pair", 1},
    {"v_cvt_f32_f64 + v_min3_u32 of its result (dependent pair)", 2},
    {"8 x v_mul_f64 |x|, then 8 x v_cvt_f32_f64 of them (independent pairs)", 2},
};

constexpr int kChains = 8, kUnroll = 32;  // 256 steps per loop trip
constexpr int kChunk = 8;                 // trips between two looks at the loop's end condition

template <int OP>
__global__ void __launch_bounds__(256) rate_kernel(uint64_t* cyc, uint32_t* done, uint32_t* sink, int trips, uint64_t window,
                                                   float seed) {
  extern __shared__ unsigned char lds[];
  double d[kChains], e[kChains];
  float f[kChains], g[kChains];
  uint32_t u[kChains], w[kChains];
#pragma unroll
  for (int i = 0; i < kChains; ++i) {
    d[i] = (double)seed * (i + 1) + threadIdx.x;
    e[i] = (double)seed + i;
    f[i] = seed * (i + 2) + threadIdx.x;
    g[i] = seed + i;
    u[i] = threadIdx.x * 2654435761u + i;
    w[i] = threadIdx.x + 7 * i;
    asm volatile("" : "+v"(d[i]), "+v"(e[i]), "+v"(f[i]), "+v"(g[i]), "+v"(u[i]), "+v"(w[i]));
  }
  double one = 1.0;
  asm volatile("" : "+v"(one));
  uint32_t zero = 0, ones = 0xffffffffu;
  asm volatile("" : "+v"(zero), "+v"(ones));
  uint32_t cls = 0x264;                                       // v_cmp_class's mask: +-0, +-inf
  asm volatile("" : "+v"(cls));
  uint64_t sel = 0x5555aaaa3333ccccull, cm[kChains] = {};   // cndmask's mask; the compares' SGPR results
  asm volatile("" : "+s"(sel));
  const uint64_t t0 = __builtin_readcyclecounter();
  // chunks of kChunk trips; fixed-work mode runs `trips` of them, window mode
  // goes on until the window has passed (the clock is read once per chunk)
  int ran = 0;
  do {
  for (int t = 0; t < kChunk; ++t) {
#pragma unroll
    for (int r = 0; r < kUnroll; ++r) {
#pragma unroll
      for (int i = 0; i < kChains; ++i) {
        if constexpr (OP == ADD_F64) asm volatile("v_add_f64 %0, %0, %1" : "+v"(d[i]) : "v"(e[i]));
        if constexpr (OP == MUL_F64) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(d[i]) : "v"(one));
        if constexpr (OP == MIN_F64) asm volatile("v_min_f64 %0, %0, %1" : "+v"(d[i]) : "v"(e[i]));
        if constexpr (OP == MAX_F64) asm volatile("v_max_f64 %0, %0, %1" : "+v"(d[i]) : "v"(e[i]));
        if constexpr (OP == CMP_EQ_F64_CNDMASK) {
          // as the flood kernel's select compiles: compare into an SGPR pair, hazard wait, select
          asm volatile("" : "+v"(d[i]));               // (not loop-invariant)
          u[i] = (d[i] == e[i]) ? u[i] : w[i];
          asm volatile("" : "+v"(u[i]));
        }
        if constexpr (OP == CVT_F64_F32) asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[i]) : "v"(f[i]));
        if constexpr (OP == CVT_F32_F64) asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(f[i]) : "v"(d[i]));
        if constexpr (OP == MUL_ABS_F64_CVT_F32) {
          asm volatile("v_mul_f64 %0, |%1|, %2" : "=v"(e[i]) : "v"(d[i]), "v"(one));
          asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(f[i]) : "v"(e[i]));
        }
        if constexpr (OP == ADD_F32) asm volatile("v_add_f32 %0, %0, %1" : "+v"(f[i]) : "v"(g[i]));
        if constexpr (OP == MIN_F32) asm volatile("v_min_f32 %0, %0, %1" : "+v"(f[i]) : "v"(g[i]));
        if constexpr (OP == MAX_F32) asm volatile("v_max_f32 %0, %0, %1" : "+v"(f[i]) : "v"(g[i]));
        if constexpr (OP == MIN3_F32)
          asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(f[i]) : "v"(g[i]), "v"(g[(i + 1) % kChains]));
        if constexpr (OP == MED3_F32)
          asm volatile("v_med3_f32 %0, %0, %1, %2" : "+v"(f[i]) : "v"(g[i]), "v"(g[(i + 1) % kChains]));
        if constexpr (OP == AND_B32) asm volatile("v_and_b32 %0, %0, %1" : "+v"(u[i]) : "v"(w[i]));
        if constexpr (OP == MIN_U32) asm volatile("v_min_u32 %0, %0, %1" : "+v"(u[i]) : "v"(w[i]));
        if constexpr (OP == MAX_U32) asm volatile("v_max_u32 %0, %0, %1" : "+v"(u[i]) : "v"(w[i]));
        if constexpr (OP == MIN3_U32)
          asm volatile("v_min3_u32 %0, %0, %1, %2" : "+v"(u[i]) : "v"(w[i]), "v"(w[(i + 1) % kChains]));
        if constexpr (OP == MED3_U32)
          asm volatile("v_med3_u32 %0, %0, %1, %2" : "+v"(u[i]) : "v"(w[i]), "v"(w[(i + 1) % kChains]));
        if constexpr (OP == BITOP3_B32)
          asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(u[i]) : "v"(w[i]), "v"(w[(i + 1) % kChains]));
        if constexpr (OP == CNDMASK_VCC)
          asm volatile("v_cmp_eq_u32 vcc, %0, %1\n\tv_cndmask_b32 %0, %0, %2, vcc"
                       : "+v"(u[i]) : "v"(w[i]), "v"(w[(i + 1) % kChains]) : "vcc");
        if constexpr (OP == MOV_B32) asm volatile("v_mov_b32 %0, %1" : "=v"(u[i]) : "v"(w[i]));
        if constexpr (OP == MOV_ROW_ROR)
          asm volatile("v_mov_b32_dpp %0, %1 row_ror:3 row_mask:0xf bank_mask:0xf" : "+v"(u[i]) : "v"(w[i]));
        if constexpr (OP == VALU_THEN_DPP)   // (VALU write -> DPP read of it: 2 wait states)
          asm volatile("v_add_u32 %0, %0, %2\n\ts_nop 1\n\tv_mov_b32_dpp %1, %0 row_ror:3 row_mask:0xf bank_mask:0xf"
                       : "+v"(u[i]), "+v"(w[i]) : "v"(threadIdx.x));
        if constexpr (OP == VALU_NOP_PAIR)   // (the same three issue slots without DPP)
          asm volatile("v_add_u32 %0, %0, %2\n\ts_nop 1\n\tv_mov_b32 %1, %2" : "+v"(u[i]), "+v"(w[i]) : "v"(threadIdx.x));
        if constexpr (OP == OR_B32_ROW_ROR)
          asm volatile("v_or_b32_dpp %0, %1, %2 row_ror:3 row_mask:0xf bank_mask:0xf" : "+v"(u[i]) : "v"(w[i]), "v"(zero));
        if constexpr (OP == AND_B32_ROW_ROR)
          asm volatile("v_and_b32_dpp %0, %1, %2 row_ror:3 row_mask:0xf bank_mask:0xf" : "+v"(u[i]) : "v"(w[i]), "v"(ones));
        if constexpr (OP == ADD_F32_ROW_ROR)
          asm volatile("v_add_f32_dpp %0, %1, %0 row_ror:3 row_mask:0xf bank_mask:0xf" : "+v"(f[i]) : "v"(g[i]));
        if constexpr (OP == MOV_B64) asm volatile("v_mov_b64 %0, %1" : "=v"(d[i]) : "v"(e[i]));
        if constexpr (OP == LSHLREV_B32) asm volatile("v_lshlrev_b32 %0, 3, %1" : "=v"(u[i]) : "v"(w[i]));
        if constexpr (OP == LSHRREV_B32) asm volatile("v_lshrrev_b32 %0, 31, %1" : "=v"(u[i]) : "v"(w[i]));
        if constexpr (OP == CNDMASK_ALONE) asm volatile("v_cndmask_b32 %0, %0, %1, %2" : "+v"(u[i]) : "v"(w[i]), "s"(sel));
        if constexpr (OP == CMP_EQ_F64_VCC) asm volatile("v_cmp_eq_f64 vcc, %0, %1" : : "v"(d[i]), "v"(e[i]) : "vcc");
        if constexpr (OP == CMP_EQ_F64_SGPR) asm volatile("v_cmp_eq_f64 %0, %1, %2" : "=s"(cm[i]) : "v"(d[i]), "v"(e[i]));
        if constexpr (OP == BFI_B32)
          asm volatile("v_bfi_b32 %0, %1, %2, %0" : "+v"(u[i]) : "v"(w[i]), "v"(w[(i + 1) % kChains]));
        if constexpr (OP == XOR_B32) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(u[i]) : "v"(w[i]));
        if constexpr (OP == CMP_CLASS_F64_VCC) asm volatile("v_cmp_class_f64 vcc, %0, %1" : : "v"(d[i]), "v"(cls) : "vcc");
        if constexpr (OP == CMP_CLASS_F64_SGPR) asm volatile("v_cmp_class_f64 %0, %1, %2" : "=s"(cm[i]) : "v"(d[i]), "v"(cls));
        if constexpr (OP == MUL_F64_CVT_F32_BITOP3) {   // the leave-one-out check node's per-edge part
          asm volatile("v_mul_f64 %0, %1, %2" : "=v"(e[i]) : "v"(d[i]), "v"(one));
          asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(f[i]) : "v"(e[i]));
          asm volatile("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x6c" : "=v"(u[i]) : "v"(w[i]), "v"(f[i]), "s"(0x80000000u));
        }
        if constexpr (OP == CMP_CLASS_F32_VCC) asm volatile("v_cmp_class_f32 vcc, %0, %1" : : "v"(f[i]), "v"(cls) : "vcc");
        if constexpr (OP == CMP_CLASS_F32_SGPR) asm volatile("v_cmp_class_f32 %0, %1, %2" : "=s"(cm[i]) : "v"(f[i]), "v"(cls));
        if constexpr (OP == CVT_F32_F64_MIN3_U32) {     // the 32-bit leave-one-out tree's first level
          asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(f[i]) : "v"(d[i]));
          asm volatile("v_min3_u32 %0, %0, %1, %2" : "+v"(u[i]) : "v"(f[i]), "v"(w[i]));
        }
        if constexpr (OP == MUL_ABS_F64_CVT_F32_INDEP) {   // its roundings: every conversion eight instructions behind its product
          if (i == 0) {
#pragma unroll
            for (int j = 0; j < kChains; ++j) asm volatile("v_mul_f64 %0, |%1|, %2" : "=v"(e[j]) : "v"(d[j]), "v"(one));
#pragma unroll
            for (int j = 0; j < kChains; ++j) asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(f[j]) : "v"(e[j]));
          }
        }
      }
    }
  }
  ran += kChunk;
  } while (window != 0 ? __builtin_readcyclecounter() - t0 < window : ran < trips);
  const uint64_t t1 = __builtin_readcyclecounter();
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < kChains; ++i) {
    acc ^= u[i] ^ w[i] ^ __float_as_uint(f[i]) ^ __float_as_uint(g[i]) ^ (uint32_t)__double_as_longlong(d[i]) ^
           (uint32_t)__double_as_longlong(e[i]) ^ (uint32_t)cm[i];
  }
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0) cyc[gw] = t1 - t0, done[gw] = (uint32_t)ran;
  sink[blockIdx.x * 256 + threadIdx.x] = acc;
  if (trips < 0) lds[threadIdx.x] = (unsigned char)acc;   // (never: the LDS request only sizes occupancy)
}

using Kern = void (*)(uint64_t*, uint32_t*, uint32_t*, int, uint64_t, float);
template <int... I>
static void fill(Kern* k, std::integer_sequence<int, I...>) { ((k[I] = &rate_kernel<I>), ...); }

int main(int argc, char** argv) {
  const int wps = argc > 1 ? atoi(argv[1]) : 2;
  const int trips = (argc > 2 ? atoi(argv[2]) : 1024) / kChunk * kChunk;
  const int reps = 5;
  if (wps != 1 && wps != 2) { fprintf(stderr, "waves per SIMD: 1 or 2\n"); return 2; }
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const int lds_cu = 160 * 1024;                   // gfx950's LDS per CU (the property may report less)
  // W workgroups of four waves fit a CU, W + 1 do not
  const int lds = wps == 2 ? lds_cu / 2 - 8192 : lds_cu - 16384;
  const int blocks = cus * wps;
  printf("{\"device\": \"%s\", \"arch\": \"%s\", \"cus\": %d, \"lds_per_cu\": %d, \"waves_per_simd\": %d, "
         "\"workgroups\": %d, \"lds_request\": %d, \"trips\": %d, \"steps_per_trip\": %d, \"clock_mhz\": %d}\n",
         prop.name, prop.gcnArchName, cus, lds_cu, wps, blocks, lds, trips, kChains * kUnroll, prop.clockRate / 1000);
  Kern kern[NUM_OPS];
  fill(kern, std::make_integer_sequence<int, NUM_OPS>{});
  uint64_t* cyc;
  uint32_t *sink, *done;
  CHECK(hipMalloc(&done, sizeof(uint32_t) * blocks * 4));
  CHECK(hipMalloc(&cyc, sizeof(uint64_t) * blocks * 4));
  CHECK(hipMalloc(&sink, sizeof(uint32_t) * blocks * 256));
  std::vector<uint64_t> h(blocks * 4);
  std::vector<uint32_t> hd(blocks * 4);
  const uint64_t window = 4000000;                 // cycles of the window pass (about 1.7 ms)
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  for (int op = 0; op < NUM_OPS; ++op) {
    CHECK(hipFuncSetAttribute((const void*)kern[op], hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    std::vector<double> mean, mx, ms;
    for (int r = 0; r < reps + 1; ++r) {           // the first launch warms up
      CHECK(hipEventRecord(e0));
      hipLaunchKernelGGL(kern[op], dim3(blocks), dim3(256), lds, 0, cyc, done, sink, trips, (uint64_t)0, 1.25f);
      CHECK(hipGetLastError());
      CHECK(hipEventRecord(e1));
      CHECK(hipEventSynchronize(e1));
      float t;
      CHECK(hipEventElapsedTime(&t, e0, e1));
      CHECK(hipMemcpy(h.data(), cyc, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost));
      if (r == 0) continue;
      double s = 0, m = 0;
      for (uint64_t c : h) s += (double)c, m = std::max(m, (double)c);
      mean.push_back(s / h.size());
      mx.push_back(m);
      ms.push_back(t);
    }
    std::sort(mean.begin(), mean.end());
    std::sort(mx.begin(), mx.end());
    std::sort(ms.begin(), ms.end());
    // window pass: every wave issues until the window has passed, so the W
    // waves of a SIMD issue side by side throughout; the SIMD's rate is the sum
    // of its waves' rates
    std::vector<double> ov;
    for (int r = 0; r < 3; ++r) {
      hipLaunchKernelGGL(kern[op], dim3(blocks), dim3(256), lds, 0, cyc, done, sink, 0, window, 1.25f);
      CHECK(hipGetLastError());
      CHECK(hipDeviceSynchronize());
      CHECK(hipMemcpy(h.data(), cyc, sizeof(uint64_t) * h.size(), hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(hd.data(), done, sizeof(uint32_t) * hd.size(), hipMemcpyDeviceToHost));
      double thr = 0;
      for (size_t i = 0; i < h.size(); ++i)
        thr += (double)hd[i] * kChains * kUnroll * kOps[op].inst_per_step / (double)h[i];
      ov.push_back(1.0 / (wps * thr / h.size()));
    }
    std::sort(ov.begin(), ov.end());
    const double inst = (double)trips * kChains * kUnroll * kOps[op].inst_per_step;
    printf("{\"op\": \"%s\", \"inst_per_wave\": %.0f, \"cycles_per_inst_simd\": %.3f, \"min\": %.3f, \"max\": %.3f, "
           "\"slowest_wave\": %.3f, \"side_by_side\": %.3f, \"kernel_ms\": %.4f}\n",
           kOps[op].name, inst, mean[reps / 2] / (inst * wps), mean[0] / (inst * wps), mean[reps - 1] / (inst * wps),
           mx[reps / 2] / (inst * wps), ov[1], ms[reps / 2]);
    fflush(stdout);
  }
  return 0;
}
