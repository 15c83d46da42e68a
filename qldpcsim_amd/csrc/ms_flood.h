// ms_flood.h — ms_flood_kernel and its LDS twin (instantiated in
// ms_flood_kernels.hip).
#pragma once
#include "decode_generic.h"
#include "qc_tables.h"

namespace qldpc {

// ---------------------------------------------------------------------------
// Flooding min-sum for uniform row degree DC <= 8 — the headline kernel.
//
// Differences from decode_kernel<MS, false, DC> (same arithmetic, same
// results, bit for bit):
//  * No graph tables in LDS. Each lane's static graph data comes once from
//    HBM ("fblob", capi_schedule.cpp) and lives in VGPRs as ready-made LDS byte
//    addresses: pa[i][k] = &post[var], ca[i][k] = &c2v[csc position] of edge
//    k of check c = lane + 64 i. The check-node step then spends no VALU on
//    addressing. Pad checks (c >= m) read post[0] and write the 8-float pad
//    behind c2v; `livem` masks their flags.
//  * Variable nodes are visited by runs of equal column degree K (variables
//    are relabeled by degree, so the CSC start of variable start + o is
//    p0 + o * K): no per-variable table, no masking, a compile-time K.
// The LDS then holds only wave state: post f64[n] | c2v f32[E + 8].
// ---------------------------------------------------------------------------
// Per-lane edge addresses of the KC checks a lane owns: absolute LDS byte
// addresses, 16 VGPRs per check, no VALU per use.
template <int KC>
struct FloodTab {
  uint32_t pa[KC][8], ca[KC][8];
  __device__ __forceinline__ void init(const uint32_t* ftab, int lane, uint32_t pbase, uint32_t cbase) {
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      uint32_t t[8];
      load_row8(ftab + (size_t)(lane + 64 * i) * 8, t);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        pa[i][k] = pbase + (t[k] & 0xffffu);
        ca[i][k] = cbase + (t[k] >> 16);
        // opaque: otherwise the compiler keeps the packed words and re-forms
        // one of the two addresses with a VALU add at every use
        asm volatile("" : "+v"(pa[i][k]), "+v"(ca[i][k]));
      }
    }
  }
  __device__ __forceinline__ void get(int i, uint32_t (&p)[8], uint32_t (&c)[8]) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      p[k] = pa[i][k];
      c[k] = ca[i][k];
    }
  }
};
struct FloodRuns {  // fblob header: runs of equal column degree (capi_schedule.cpp)
  int n_runs;
  int start[QLDPC_MAX_RUNS], count[QLDPC_MAX_RUNS], deg[QLDPC_MAX_RUNS], p0[QLDPC_MAX_RUNS];
};

// Sequential float32 sum in ascending check order (np.sum axis=0). It starts
// from the first term instead of 0.0f + x0: the two differ only in the sign of
// an all-zero sum, and post = L + S is the same for S = +0 and S = -0 (L is
// never -0), so the posteriors are bit-identical.
template <int K>
__device__ __forceinline__ float vn_sum(const float* c) {
  if constexpr (K == 0) {
    return 0.0f;
  } else {
    float x[K];
#pragma unroll
    for (int t = 0; t < K; ++t) x[t] = c[t];
    float s = x[0];
#pragma unroll
    for (int t = 1; t < K; ++t) s += x[t];               // float32, ascending check
    return s;
  }
}

template <int K>
__device__ __forceinline__ void vn_run(const DecodeArgs& a, double* post, const float* c2v,
                                       int start, int count, int p0, int lane) {
  // post[start + o] = L + (f64) sum_t c2v[p0 + o K + t]   (decoders.py:172-173)
  // Full 64-variable chunks two at a time (two independent add chains in
  // flight), then the masked tail.
  const float* c = c2v + p0 + lane * K;
  double* po = post + start + lane;
  int o0 = 0;
  if constexpr (QLDPC_VN_PAIR != 0) {
    for (; o0 + 128 <= count; o0 += 128) {
      const float s0 = vn_sum<K>(c + o0 * K);
      const float s1 = vn_sum<K>(c + (o0 + 64) * K);
      po[o0] = a.L + (double)s0;
      po[o0 + 64] = a.L + (double)s1;
    }
  }
  for (; o0 + 64 <= count; o0 += 64) po[o0] = a.L + (double)vn_sum<K>(c + o0 * K);
  if (o0 + lane < count) po[o0] = a.L + (double)vn_sum<K>(c + o0 * K);
}

__device__ __forceinline__ void vn_run_any(const DecodeArgs& a, double* post, const float* c2v,
                                           int start, int count, int K, int p0, int lane) {
  for (int o = lane; o < count; o += 64) {
    const float* c = c2v + p0 + o * K;
    float s = 0.0f;
    for (int t = 0; t < K; ++t) s += c[t];
    post[start + o] = a.L + (double)s;
  }
}

template <int KC>
constexpr int ms_flood_max_threads() { return KC >= 8 ? 512 : 256; }
template <int KC>
constexpr int ms_flood_wpe() { return KC >= 8 ? 2 : QLDPC_FLOOD_WPE; }

// The LDS-resident body described above: ms_flood_kernel's for every shape
// without generated protograph tables, ms_flood_lds_kernel's for all.
template <int DC, int KC>
__device__ __forceinline__ void ms_flood_lds_body(const DecodeArgs& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  static_assert(DC >= 2 && DC <= 8, "row degree 2..8");
  const FloodRuns* runs = (const FloodRuns*)a.blob;                     // global, uniform
  const uint32_t* ftab = (const uint32_t*)(a.blob + a.off_cn_tab);      // global
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  unsigned char* ws = lds + QLDPC_FLOOD_HDR + wid * a.wave_bytes;
  double* post = (double*)ws;
  unsigned char* c2v_b = ws + a.off_c2v;
  const float* c2v_f = (const float*)c2v_b;
  const int m = a.m, n = a.n;

  // static per-lane graph data (VGPRs for the kernel)
  FloodTab<KC> tab;
  tab.init(ftab, lane, lds_addr(ws), lds_addr(ws) + (uint32_t)a.off_c2v);
  uint32_t livem = 0;
#pragma unroll
  for (int i = 0; i < KC; ++i)
    if (lane + 64 * i < m) livem |= 1u << i;
  // the runs header lives in LDS (the first QLDPC_FLOOD_HDR bytes): one
  // broadcast read per field per iteration, no global latency in the loop
  const int n_runs = __builtin_amdgcn_readfirstlane(runs->n_runs);
  if (threadIdx.x < 4 * QLDPC_MAX_RUNS) ((int*)lds)[threadIdx.x] = (&runs->start[0])[threadIdx.x];
  __syncthreads();
  const int* hdr = (const int*)lds;

  for (HalfShotQueue Q(a.batch, a.queue, waves, wid); Q.hs < a.batch; Q.advance()) {
    const long long hs = Q.hs;
    Q.prefetch(threadIdx.x & 63);
    int fl = 0;
    int iters = a.max_iter;
    bool conv = false;
    uint32_t synreg = 0;
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      const int c = lane + 64 * i;
      if (c < m) synreg |= syn_bit(a, hs, c) << i;
    }
    for (int it = 0;; ++it) {
      uint32_t unsat = 0;
      if (it == 0) {
        // every v2c = float32(L) (decoders.py:148-149): one value per check
        const double vf = (double)a.L32;
        const double av = __builtin_fabs(vf);
        const uint32_t cb = __builtin_bit_cast(uint32_t, (float)(a.beta * av));
        const uint32_t neg = (uint32_t)(vf < 0.0);
        if (av == 0.0) fl |= FLAG_MIN_ZERO;
#pragma unroll
        for (int i = 0; i < KC; ++i) {
          const uint32_t negprod = ((neg * DC) ^ (synreg >> i)) & 1u;
          const uint32_t val = cb | ((neg ^ negprod) << 31);
          uint32_t pa[8], ca[8];
          tab.get(i, pa, ca);
#pragma unroll
          for (int k = 0; k < DC; ++k) *QLDPC_LDS(uint32_t, ca[k]) = val;
        }
      } else {
#pragma unroll
        for (int i = 0; i < KC; ++i) {
          uint32_t pa[8], ca[8];
          tab.get(i, pa, ca);
          unsat |= cn_ms_abs<DC>(a, pa, ca, (synreg >> i) & 1u, (livem >> i) & 1u, fl);
          __builtin_amdgcn_sched_barrier(0);         // one check's working set at a time
        }
        // stop test of iteration it-1 (decoders.py:175-176)
        if (ballot(unsat != 0) == 0) {
          iters = it;
          conv = true;
          break;
        }
      }
      wave_sync();
      for (int r = 0; r < n_runs; ++r) {
        const int st = __builtin_amdgcn_readfirstlane(hdr[r]);
        const int cnt = __builtin_amdgcn_readfirstlane(hdr[QLDPC_MAX_RUNS + r]);
        const int K = __builtin_amdgcn_readfirstlane(hdr[2 * QLDPC_MAX_RUNS + r]);
        const int p0 = __builtin_amdgcn_readfirstlane(hdr[3 * QLDPC_MAX_RUNS + r]);
        switch (K) {
          case 0: vn_run<0>(a, post, c2v_f, st, cnt, p0, lane); break;
          case 1: vn_run<1>(a, post, c2v_f, st, cnt, p0, lane); break;
          case 2: vn_run<2>(a, post, c2v_f, st, cnt, p0, lane); break;
          case 3: vn_run<3>(a, post, c2v_f, st, cnt, p0, lane); break;
          case 4: vn_run<4>(a, post, c2v_f, st, cnt, p0, lane); break;
          case 5: vn_run<5>(a, post, c2v_f, st, cnt, p0, lane); break;
          case 6: vn_run<6>(a, post, c2v_f, st, cnt, p0, lane); break;
          default: vn_run_any(a, post, c2v_f, st, cnt, K, p0, lane); break;
        }
      }
      wave_sync();
      if (it + 1 == a.max_iter) {
        uint32_t un = 0;
#pragma unroll
        for (int i = 0; i < KC; ++i) {
          uint32_t ph = 0;
          uint32_t pa[8], ca[8];
          tab.get(i, pa, ca);
#pragma unroll
          for (int k = 0; k < DC; ++k) ph ^= hi_word(*QLDPC_LDS(const double, pa[k]));
          un |= (((ph >> 31) ^ (synreg >> i)) & (livem >> i)) & 1u;
        }
        conv = ballot(un != 0) == 0;
        break;
      }
    }
    double* po = a.post ? a.post + hs * (long long)n : nullptr;
    for (int jo = lane; jo < n; jo += 64) {
      const double pv = post[a.vinv[jo]];
      put_ehat(a, hs, jo, pv < 0.0);
      if (po) po[jo] = pv;
    }
    const uint64_t b1 = ballot((fl & FLAG_MIN_ZERO) != 0);
    if (lane == 0) {
      a.iters[hs] = iters;
      if (a.flags) a.flags[hs] = (int32_t)((b1 ? FLAG_MIN_ZERO : 0) | (conv ? FLAG_CONVERGED : 0));
    }
    wave_sync();
  }
}

#include "ms_flood_qc.h"   // flood_qc_body: the register-resident body (lift-16 QC codes)

// A (DC, KC) shape some generated table has: ms_flood_kernel<DC, KC> is then
// the register-resident kernel (256 VGPRs, two waves per SIMD, no LDS) and
// DecodeArgs::qc_table names the table; codes of that shape that match no
// table, and option flood_qc = 0, run the twin ms_flood_lds_kernel<DC, KC>.
template <typename T, int DC, int KC>
constexpr bool qc_table_fits() { return T::DC == DC && (16 * T::MB + 63) / 64 == KC; }
template <int DC, int KC>
constexpr bool ms_flood_is_qc() {
  bool any = false;
#define QLDPC_QC_ANY(ID, T, NAME) any = any || qc_table_fits<T, DC, KC>();
  QLDPC_QC_TABLES(QLDPC_QC_ANY)
#undef QLDPC_QC_ANY
  return any;
}
template <int DC, int KC>
constexpr int ms_flood_wpe2() { return ms_flood_is_qc<DC, KC>() ? 2 : ms_flood_wpe<KC>(); }

template <int DC, int KC>
__global__ void __launch_bounds__(ms_flood_max_threads<KC>())
__attribute__((amdgpu_waves_per_eu(ms_flood_wpe2<DC, KC>()))) ms_flood_kernel(DecodeArgs a) {
  if constexpr (ms_flood_is_qc<DC, KC>()) {
    switch (a.qc_table) {                              // wave-uniform, outside every loop
#define QLDPC_QC_CASE(ID, T, NAME) \
  case ID:                         \
    if constexpr (qc_table_fits<T, DC, KC>()) flood_qc_body<T>(a); \
    break;
      QLDPC_QC_TABLES(QLDPC_QC_CASE)
#undef QLDPC_QC_CASE
      default: break;
    }
  } else {
    ms_flood_lds_body<DC, KC>(a);
  }
}

template <int DC, int KC>
__global__ void __launch_bounds__(ms_flood_max_threads<KC>()) __attribute__((amdgpu_waves_per_eu(ms_flood_wpe<KC>())))
ms_flood_lds_kernel(DecodeArgs a) {
  ms_flood_lds_body<DC, KC>(a);
}

}  // namespace qldpc
