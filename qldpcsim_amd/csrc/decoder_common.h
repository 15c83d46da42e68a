// decoder_common.h — device helpers shared by every MS / BP kernel family
// (the execution model and numerics: decoder_kernels.hip): the libm table
// image, NumPy's summation orders, syndrome input and estimate output, the
// min / xor trees of the uniform-degree check nodes and the DPP lane swaps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "decoder_kernels.h"
#include "tuning.h"
#include "kargs.h"
#include "wave_common.h"
#include "../../include/qldpc_libm.h"

namespace qldpc {

// NumPy's tanh / SVML's atanh tables (include/qldpc_libm.h). BP kernels copy
// this image into LDS (DecodeArgs::off_libm) once per workgroup: the lookups
// are per lane (data-dependent intervals), 10-13 per edge and iteration.
static __constant__ qldpc_libm_tab qldpc_libm_dev = QLDPC_LIBM_TAB_INIT;   // one per translation unit

__device__ __forceinline__ const qldpc_libm_tab* stage_libm(unsigned char* lds, int off) {
  const uint4* src = (const uint4*)&qldpc_libm_dev;
  uint4* dst = (uint4*)(lds + off);
  for (int i = threadIdx.x; i < (int)(sizeof(qldpc_libm_tab) / 16); i += blockDim.x) dst[i] = src[i];
  return (const qldpc_libm_tab*)(lds + off);
}

__device__ __forceinline__ const DecodeArgs& kargs_fresh() { return kargs_fresh<DecodeArgs>(); }

// NumPy DOUBLE_pairwise_sum over a contiguous LDS segment (np.sum of a 1-D
// float64 array = 0.0 + pairwise(all); decoders.py:269, :276). n <= 128.
__device__ __forceinline__ double np_pairwise_sum(const double* a, int n) {
  if (n < 8) {
    double res = -0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return 0.0 + res;
  }
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  const int nb = n - (n % 8);
  for (; i < nb; i += 8) {
    r0 += a[i + 0]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
    r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i];
  return 0.0 + res;
}

// np_pairwise_sum of a BP column (variable node, decoders.py:276): below 8
// terms NumPy adds sequentially from -0.0, so with K >= n terms loaded at
// once (the c2v region is padded by 8 entries) and the terms past n replaced
// by -0.0 — x + -0.0 == x for every x, -0.0 included — the sum is the same
// bit for bit, without a load-wait-add chain per term. K is wave-uniform:
// the smallest of 3 / 5 / 7 covering every active lane's n (ballots); a wave
// holding a column of 8 or more terms takes the general pairwise sum.
template <int K>
__device__ __forceinline__ double np_sum_lt8(const double* a, int n) {
  double x[K];
#pragma unroll
  for (int t = 0; t < K; ++t) x[t] = a[t];
  double res = -0.0;
#pragma unroll
  for (int t = 0; t < K; ++t) res += (t < n) ? x[t] : -0.0;
  return 0.0 + res;
}

// The same when every active lane's n >= 3 (round 6): -0.0 + x0 == x0 for
// every x0, so the sum starts at x0; prefix sums over all K terms, and n
// picks one of the last K - 2 (a compare and a 64-bit select each) instead of
// a compare and select per term — the same float64 additions on the first n
// terms, the same bits
template <int K>
__device__ __forceinline__ double np_sum_lt8_lo3(const double* a, int n) {
  double x[K];
#pragma unroll
  for (int t = 0; t < K; ++t) x[t] = a[t];
  double pre = x[0];
#pragma unroll
  for (int t = 1; t < 3; ++t) pre += x[t];
  double res = pre;                                        // n = 3
#pragma unroll
  for (int t = 3; t < K; ++t) {
    pre += x[t];                                           // (terms past n: discarded below)
    res = n > t ? pre : res;
  }
  return 0.0 + res;
}

// LO3: try the n >= 3 form first (the layered team kernel: -0.7 % per LP118_2
// p = 0.1 launch; the flooding kernel's extra ballot cost +0.7 %, so it keeps
// the plain form, profiles/r06/r06d_ab_msnew_main.json)
template <bool LO3 = false>
__device__ __forceinline__ double np_sum_col(const double* a, int n) {
  if (__builtin_expect(ballot_b(n >= 8) != 0, 0)) return np_pairwise_sum(a, n);
  if (LO3 && ballot_b(n < 3) == 0) {
    if (ballot_b(n > 3) == 0) return np_sum_lt8_lo3<3>(a, n);
    if (ballot_b(n > 5) == 0) return np_sum_lt8_lo3<5>(a, n);
    return np_sum_lt8_lo3<7>(a, n);
  }
  if (ballot_b(n > 3) == 0) return np_sum_lt8<3>(a, n);
  if (ballot_b(n > 5) == 0) return np_sum_lt8<5>(a, n);
  return np_sum_lt8<7>(a, n);
}

// Set bit `c` of a per-wave bit-word array for every lane whose predicate is
// true, for a chunk of 64 consecutive indices starting at c0 (all lanes call).
__device__ __forceinline__ void store_bits64(uint32_t* words, int c0, int pred, int lane) {
  const uint64_t b = ballot(pred);
  if (lane == 0) words[c0 >> 5] = (uint32_t)b;
  if (lane == 1) words[(c0 >> 5) + 1] = (uint32_t)(b >> 32);
}

// Bit-packed I/O (DecodeArgs::syn_bits / eh_bits): syndromes and hard
// decisions as 64-bit words, bit j % 64 of word j / 64 (the error-vector
// layout of the device sampler), instead of one byte per bit.
__device__ __forceinline__ uint32_t syn_bit(const DecodeArgs& a, long long hs, int c) {
  if (a.syn_bits) return (uint32_t)(((const uint64_t*)a.syn)[hs * a.wm + (c >> 6)] >> (c & 63)) & 1u;
  return a.syn[hs * (long long)a.m + c] & 1u;
}
// ê_jo of half-shot hs. Callers visit columns in 64-aligned wave chunks
// (lane l holds column 64 k + l), so with eh_bits the chunk is one ballot and
// lane 0 stores the word.
__device__ __forceinline__ void put_ehat(const DecodeArgs& a, long long hs, int jo, bool bit) {
  if (a.eh_bits) {
    const uint64_t b = ballot(bit);
    if ((jo & 63) == 0) ((uint64_t*)a.ehat)[hs * a.wn + (jo >> 6)] = b;
  } else {
    a.ehat[hs * (long long)a.n + jo] = (uint8_t)bit;
  }
}

// Syndrome bits of checks lane + 64 i (i < KC) of half-shot hs as bit i of
// the result, every load issued before the first use: bit-packed rows are
// KC wave-uniform words (scalar loads), byte rows KC per-lane loads at
// clamped addresses (a guard around each load made the compiler wait after
// each one).
template <int KC>
__device__ __forceinline__ uint32_t syn_lane_bits(const DecodeArgs& a, long long hs, int lane) {
  const int m = a.m;
  uint32_t r = 0;
  if (a.syn_bits) {
    const uint64_t* row = (const uint64_t*)a.syn + hs * a.wm;
    uint64_t w[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) w[i] = ld_const(row, i < a.wm ? i : a.wm - 1);
#pragma unroll
    for (int i = 0; i < KC; ++i) {                  // (32-bit halves: no 64-bit VGPR shifts)
      const uint32_t h = lane < 32 ? (uint32_t)w[i] : (uint32_t)(w[i] >> 32);
      r |= (((h >> (lane & 31)) & 1u) & (uint32_t)(lane + 64 * i < m)) << i;
    }
  } else {
    const uint8_t* row = a.syn + hs * (long long)m;
    // (opaque lane: the clamped offsets are cheap to form here; hoisted out of
    // the half-shot loop as invariants they cost VGPRs the decode loop needs)
    uint32_t ln;
    asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
    uint32_t b[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) b[i] = row[(int)ln + 64 * i < m ? (int)ln + 64 * i : m - 1];
#pragma unroll
    for (int i = 0; i < KC; ++i) r |= ((b[i] & 1u) & (uint32_t)(lane + 64 * i < m)) << i;
  }
  return r;
}

// ê (and posteriors) of one half-shot: original column jo = ST k + t takes
// post_of(vinv[jo]) (the relabeled variable's posterior); ST = 64 with t the
// lane (one wave per half-shot) or the team size with t the thread index (a
// wave's columns stay one aligned 64-column chunk). Chunks of OC trips: the
// OC vinv loads, then the OC posterior reads, then the outputs — one round
// trip per stage instead of one per trip (a guarded load per trip made the
// compiler wait after each one).
template <int OC, int ST, typename Post>
__device__ __forceinline__ void write_outputs_strided(const DecodeArgs& a, long long hs, int t, Post post_of) {
  const int n = a.n;
  const int cb = t & ~63;                            // this wave's chunk offset within a trip
  double* po = a.post ? a.post + hs * (long long)n : nullptr;
  for (int k0 = 0; ST * k0 < n; k0 += OC) {
    int v[OC];
#pragma unroll
    for (int u = 0; u < OC; ++u) {
      const int jo = ST * (k0 + u) + t;
      v[u] = a.vinv[jo < n ? jo : n - 1];
    }
    double pv[OC];
#pragma unroll
    for (int u = 0; u < OC; ++u) pv[u] = post_of(v[u]);
#pragma unroll
    for (int u = 0; u < OC; ++u) {
      const int jo = ST * (k0 + u) + t;
      if (ST * (k0 + u) + cb < n) {                  // (wave-uniform; columns past n ballot 0)
        if (a.eh_bits) {
          put_ehat(a, hs, jo, jo < n && pv[u] < 0.0);
        } else if (jo < n) {
          put_ehat(a, hs, jo, pv[u] < 0.0);
        }
        if (po && jo < n) po[jo] = pv[u];
      }
    }
  }
}
template <int OC, typename Post>
__device__ __forceinline__ void write_outputs_batched(const DecodeArgs& a, long long hs, int lane, Post post_of) {
  write_outputs_strided<OC, 64>(a, hs, lane, post_of);
}

// syndrome bits of one half-shot into a team's word array: thread t covers
// checks ST k + t, NT trips with their loads in flight together
template <int NT, int ST>
__device__ __forceinline__ void team_syndrome_bits(const DecodeArgs& a, long long hs, uint32_t* synw, int t) {
  const int m = a.m, lane = t & 63, cb = t & ~63;
  for (int k0 = 0; ST * k0 < m; k0 += NT) {
    uint32_t b[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int c = ST * (k0 + u) + t;
      b[u] = syn_bit(a, hs, c < m ? c : m - 1);
    }
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int c0 = ST * (k0 + u) + cb;
      if (c0 < m) store_bits64(synw, c0, (c0 + lane < m) ? (int)b[u] : 0, lane);
    }
  }
}

// Half-shot prologue / epilogue with every global load issued up front (a
// loop of dependent load -> use steps paid one HBM latency per 64 elements).
// The relabeling vinv is per code, so it is read once per kernel into
// registers: VinvRegs holds original column 64k + lane's variable for k < NJ
// (two 16-bit entries per VGPR); n > 64 NJ falls back to global reads.
template <int NJ>
struct VinvRegs {
  uint32_t w[(NJ + 1) / 2];
  __device__ __forceinline__ void load(const uint16_t* vinv, int n, int lane) {
#pragma unroll
    for (int k = 0; k < NJ; k += 2) {
      const int j0 = 64 * k + lane, j1 = j0 + 64;
      const uint32_t v0 = j0 < n ? vinv[j0] : 0u, v1 = j1 < n ? vinv[j1] : 0u;
      w[k / 2] = v0 | (v1 << 16);
    }
  }
  __device__ __forceinline__ int get(int k) const { return (int)((w[k / 2] >> (16 * (k & 1))) & 0xffffu); }
};

// ê (and posteriors) of one half-shot in original column order
template <int NJ>
__device__ __forceinline__ void write_outputs(const DecodeArgs& a, const VinvRegs<NJ>& vr, const double* post,
                                              long long hs, int lane) {
  const int n = a.n;
  double* po = a.post ? a.post + hs * (long long)n : nullptr;
  if (n <= 64 * NJ) {
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      const int jo = 64 * k + lane;
      if (64 * k < n && jo < n) {
        const double pv = post[vr.get(k)];
        put_ehat(a, hs, jo, pv < 0.0);
        if (po) po[jo] = pv;
      }
    }
  } else {
    for (int jo = lane; jo < n; jo += 64) {
      const double pv = post[a.vinv[jo]];
      put_ehat(a, hs, jo, pv < 0.0);
      if (po) po[jo] = pv;
    }
  }
}

// syndrome bits of one half-shot into the per-wave word array (m <= 64 NC:
// all byte loads in flight together; larger m loops)
template <int NC>
__device__ __forceinline__ void load_syndrome_bits(const DecodeArgs& a, long long hs, uint32_t* synw, int lane) {
  const int m = a.m;
  if (a.syn_bits) {                                 // already words: copy them
    const uint32_t* src = (const uint32_t*)((const uint64_t*)a.syn + hs * a.wm);
    for (int w = lane; w < 2 * a.wm; w += 64) synw[w] = src[w];
    return;
  }
  const uint8_t* syn = a.syn + hs * (long long)m;
  if (m <= 64 * NC) {
    // every load at a clamped address (a guarded load per chunk made the
    // compiler wait after each one); the opaque lane keeps the offsets from
    // being hoisted out of the half-shot loop into VGPRs
    uint32_t ln;
    asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
    uint32_t b[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const int c = 64 * k + (int)ln;
      b[k] = syn[c < m ? c : m - 1];
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) b[k] = (64 * k + lane < m) ? (b[k] & 1u) : 0u;
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (64 * k < m) store_bits64(synw, 64 * k, (int)b[k], lane);
  } else {
    for (int c0 = 0; c0 < m; c0 += 64) {
      const int c = c0 + lane;
      store_bits64(synw, c0, c < m ? (syn[c] & 1) : 0, lane);
    }
  }
}

// Hide a register value's provenance from the optimizer, so that values
// derived from it are not re-derived (or hoisted) where that costs VALU or VGPRs.
__device__ __forceinline__ uint32_t opaque_always(uint32_t x) {
  asm volatile("" : "+v"(x));
  return x;
}

// v_min_f64 / v_max_f64 without the canonicalizes LLVM adds around
// minnum/maxnum (operands here are never signalling NaNs).
__device__ __forceinline__ double vmin_f64(double x, double y) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ double vmin_abs_f64(double x, double y) {  // min(|x|, y)
  double r;
  asm("v_min_f64 %0, |%1|, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ double vmax_abs_f64(double x, double y) {  // max(|x|, y)
  double r;
  asm("v_max_f64 %0, |%1|, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}

__device__ __forceinline__ double vmin_abs2_f64(double x, double y) {  // min(|x|, |y|)
  double r;
  asm("v_min_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ double vmax_abs2_f64(double x, double y) {  // max(|x|, |y|)
  double r;
  asm("v_max_f64 %0, |%1|, |%2|" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ double vmax_f64(double x, double y) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
  return r;
}

// Smallest and second smallest (with multiplicity) of |v[0..N)| as a
// tournament: pairs, then merges (l1,h1)+(l2,h2) -> (min(l1,l2),
// min(max(l1,l2), min(h1,h2))). Depth ~log2 N instead of a serial chain
// (the check-node step is latency-bound), and fewer ops than the chain.
template <int N>
__device__ __forceinline__ void min12_tree(const double* v, double& lo, double& hi) {
  if constexpr (N == 1) {
    lo = __builtin_fabs(v[0]);
    hi = __builtin_inf();
  } else if constexpr (N == 2) {
    lo = vmin_abs2_f64(v[0], v[1]);
    hi = vmax_abs2_f64(v[0], v[1]);
  } else {
    constexpr int H = (N / 2 + 1) & ~1;   // even split: 3->2+1, 5->2+3, 6->4+2, 7->4+3, 8->4+4
    double l1, h1, l2, h2;
    min12_tree<(H < N ? H : N - 1)>(v, l1, h1);
    min12_tree<N - (H < N ? H : N - 1)>(v + (H < N ? H : N - 1), l2, h2);
    lo = vmin_f64(l1, l2);
    hi = vmin_f64(vmax_f64(l1, l2), vmin_f64(h1, h2));
  }
}

// Leave-one-out minima of |v[0..N)|, N >= 2: loo[e] = min over e' != e of
// |v[e']|. A recursion over halves, split as min12_tree's: going up, each
// subtree's minimum is formed once; going down, a subtree is handed the minimum
// of everything outside it, min(sibling's minimum, parent's outside), and a leaf's
// outside is its loo. Abs modifiers on the leaf reads. The root forms nothing:
// its halves' outsides are each other's minima, top0 (of |v[0..A)|) and top1 (of
// the rest), and min(top0, top1) is the minimum of all. 3 N - 6 instructions:
// N - 2 going up, 2 N - 4 going down (8: 4 + 2 and 4 + 8; min12_tree: 20).
template <int N>
constexpr int loo_split() {
  constexpr int H = (N / 2 + 1) & ~1;     // min12_tree's even split
  return H < N ? H : N - 1;
}
template <int N>
__device__ __forceinline__ double loo_up(const double* v, double* sub) {
  // sub: the minima of this subtree's inner nodes of two leaves or more, in
  // pre-order (N - 1 of them, the node's own first)
  static_assert(N >= 2, "a leaf is read where it is used");
  constexpr int A = loo_split<N>(), B = N - A;
  if constexpr (N == 2) {
    return sub[0] = vmin_abs2_f64(v[0], v[1]);
  } else if constexpr (B == 1) {
    return sub[0] = vmin_abs_f64(v[A], loo_up<A>(v, sub + 1));
  } else {
    const double a = loo_up<A>(v, sub + 1);
    return sub[0] = vmin_f64(a, loo_up<B>(v + A, sub + A));
  }
}
// min(minimum of the K values at v, whose inner nodes' minima are at sub; out)
template <int K>
__device__ __forceinline__ double loo_with(const double* v, const double* sub, double out) {
  if constexpr (K == 1) return vmin_abs_f64(v[0], out);
  else return vmin_f64(sub[0], out);
}
template <int N>
__device__ __forceinline__ void loo_down(const double* v, const double* sub, double out, double* loo) {
  constexpr int A = loo_split<N>(), B = N - A;
  if constexpr (N == 1) {
    loo[0] = out;
  } else {
    // (sub[0] is this node's own minimum; the halves' nodes follow it)
    loo_down<A>(v, sub + 1, loo_with<B>(v + A, sub + A, out), loo);
    loo_down<B>(v + A, sub + A, loo_with<A>(v, sub + 1, out), loo + A);
  }
}
template <int N>
__device__ __forceinline__ void loo_min_tree(const double* v, double* loo, double& top0, double& top1) {
  static_assert(N >= 2, "a single value has no others");
  constexpr int A = loo_split<N>(), B = N - A;
  double sub[N];                          // (slot 0 unused: the root's minimum is not formed)
  if constexpr (A == 1) top0 = __builtin_fabs(v[0]);
  else top0 = loo_up<A>(v, sub + 1);
  if constexpr (B == 1) top1 = __builtin_fabs(v[A]);
  else top1 = loo_up<B>(v + A, sub + A);
  loo_down<A>(v, sub + 1, top1, loo);
  loo_down<B>(v + A, sub + A, top0, loo + A);
}

// Unsigned minimum / median of three (non-negative float32 bit patterns order
// as unsigned integers; no canonicalisation, no denormal mode)
__device__ __forceinline__ uint32_t umin3(uint32_t x, uint32_t y, uint32_t z) {
  uint32_t r;
  asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}
__device__ __forceinline__ uint32_t umed3(uint32_t x, uint32_t y, uint32_t z) {
  uint32_t r;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}

// Smallest and second smallest (with multiplicity) of w[0..N) as unsigned
// integers. A group of three gives its pair as (min3, med3), a group of two as
// (min, max), a single value has no second. Three pairs (l, h) merge as
//   lo = min3(l1, l2, l3),  hi = min(med3(l1, l2, l3), min3(h1, h2, h3)):
// with the smallest value taken out, what remains is the other two l (their
// smaller one is the median of the three) and every h. N = 8 as 3 + 3 + 2 and
// N = 7 as 3 + 2 + 2: 10 instructions each (pairwise merging as min12_tree's: 17).
template <int N>
__device__ __forceinline__ void min12_tree_u32(const uint32_t* w, uint32_t& lo, uint32_t& hi) {
  if constexpr (N == 1) {
    lo = w[0];
    hi = 0xffffffffu;
  } else if constexpr (N == 2) {
    lo = w[0] < w[1] ? w[0] : w[1];
    hi = w[0] < w[1] ? w[1] : w[0];
  } else if constexpr (N == 3) {
    lo = umin3(w[0], w[1], w[2]);
    hi = umed3(w[0], w[1], w[2]);
  } else {
    constexpr int A = (N + 2) / 3, B = (N + 1) / 3, C = N / 3;   // A >= B >= C >= 1, A >= 2
    uint32_t l1, h1, l2, h2, l3, h3;
    min12_tree_u32<A>(w, l1, h1);
    min12_tree_u32<B>(w + A, l2, h2);
    min12_tree_u32<C>(w + A + B, l3, h3);
    lo = umin3(l1, l2, l3);
    const uint32_t m = umed3(l1, l2, l3);
    if constexpr (C >= 2) {
      const uint32_t h = umin3(h1, h2, h3);
      hi = m < h ? m : h;
    } else if constexpr (B >= 2) {
      hi = umin3(m, h1, h2);
    } else {
      hi = m < h1 ? m : h1;
    }
  }
}

// Leave-one-out minima of w[0..N) as unsigned integers, N >= 2: loo[e] = min
// over e' != e of w[e']. Up to four values each take the minimum of the other
// three (or two; of two, the other one). More are cut into N / 3 groups of
// three and N % 3 single values: a group's minimum is one min3, the groups'
// minima and the single values are the items of the same problem one level up,
// whose result is each item's outside (the minimum of everything not in it);
// a single value's outside is its loo, and a group's member takes min3(the
// other two, the group's outside). N = 8 as 3 + 3 + 1 + 1:
//   mA = min3(w0, w1, w2)      mB = min3(w3, w4, w5)
//   oA = min3(mB, w6, w7)      oB = min3(mA, w6, w7)
//   loo6 = min3(mA, mB, w7)    loo7 = min3(mA, mB, w6)
//   loo0 = min3(w1, w2, oA) ... loo5 = min3(w3, w4, oB)
// 12 instructions (loo_min_tree on float64: 18). top0 and top1 are the first two
// items of the top level (mA and mB; w[0] and w[1] for N <= 4) and out0 the
// first one's outside (oA; loo[0]): min(top0, out0) is the minimum of all, and
// where at most one value is below some bound, top0 or top1 is not.
constexpr int loo_min_tree_u32_ops(int n) {               // (tests/test_loo32_identity.py reads this line)
  return n <= 2 ? 0 : n <= 4 ? n : 4 * (n / 3) + loo_min_tree_u32_ops(n / 3 + n % 3);
}
__device__ __forceinline__ uint32_t umin2(uint32_t x, uint32_t y) { return x < y ? x : y; }
template <int N>
__device__ __forceinline__ void loo_min_tree_u32(const uint32_t* w, uint32_t* loo, uint32_t& top0, uint32_t& top1,
                                                 uint32_t& out0) {
  static_assert(N >= 2, "a single value has no others");
  if constexpr (N == 2) {
    loo[0] = w[1], loo[1] = w[0];
  } else if constexpr (N == 3) {
    loo[0] = umin2(w[1], w[2]), loo[1] = umin2(w[0], w[2]), loo[2] = umin2(w[0], w[1]);
  } else if constexpr (N == 4) {
    loo[0] = umin3(w[1], w[2], w[3]), loo[1] = umin3(w[0], w[2], w[3]);
    loo[2] = umin3(w[0], w[1], w[3]), loo[3] = umin3(w[0], w[1], w[2]);
  } else {
    constexpr int G = N / 3, R = N % 3, K = G + R;
    uint32_t t[K], o[K], t0, t1, o0;
#pragma unroll
    for (int g = 0; g < G; ++g) t[g] = umin3(w[3 * g], w[3 * g + 1], w[3 * g + 2]);
#pragma unroll
    for (int r = 0; r < R; ++r) t[G + r] = w[3 * G + r];
    loo_min_tree_u32<K>(t, o, t0, t1, o0);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      loo[3 * g] = umin3(w[3 * g + 1], w[3 * g + 2], o[g]);
      loo[3 * g + 1] = umin3(w[3 * g], w[3 * g + 2], o[g]);
      loo[3 * g + 2] = umin3(w[3 * g], w[3 * g + 1], o[g]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) loo[3 * G + r] = o[G + r];
    top0 = t[0], top1 = t[1], out0 = o[0];
    return;
  }
  top0 = w[0], top1 = w[1], out0 = loo[0];
}

// XOR of N words as a balanced tree (v_xor3_b32-friendly)
__device__ __forceinline__ uint32_t xor3(uint32_t x, uint32_t y, uint32_t z) {
  uint32_t r;
  // gfx950 has no v_xor3_b32; v_bitop3_b32 truth table 0x96 = S0 ^ S1 ^ S2
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(x), "v"(y), "v"(z));
  return r;
}
// (x & m) ^ y in one instruction, m wave-uniform (truth table 0x6c = (S0 & S2) ^ S1)
__device__ __forceinline__ uint32_t and_xor(uint32_t x, uint32_t m, uint32_t y) {
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x6c" : "=v"(r) : "v"(x), "v"(y), "s"(m));
  return r;
}
template <int N>
__device__ __forceinline__ uint32_t xor_tree(const uint32_t* w) {
  if constexpr (N == 1) return w[0];
  else if constexpr (N == 2) return w[0] ^ w[1];
  else if constexpr (N == 3) return xor3(w[0], w[1], w[2]);
  else if constexpr (N == 4) return xor3(w[0], w[1], w[2]) ^ w[3];
  else if constexpr (N == 5) return xor3(xor3(w[0], w[1], w[2]), w[3], w[4]);
  else return xor3(xor_tree<N - 2>(w), w[N - 2], w[N - 1]);
}

__device__ __forceinline__ uint32_t hi_word(double d) { return (uint32_t)(__builtin_bit_cast(uint64_t, d) >> 32); }

// DPP lane swaps (ms_layered.h's lane groups, wave_xor below)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  return __builtin_bit_cast(double, ((uint64_t)dpp_u32<CTRL>((uint32_t)(u >> 32)) << 32) | dpp_u32<CTRL>((uint32_t)u));
}
constexpr int kDppQuadXor1 = 0xB1;     // quad_perm [1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;     // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;  // row_half_mirror: lane i <-> 7-i within 8

// XOR of a 32-bit value over the 64 lanes (all lanes active): DPP within each
// row of 16 lanes, then the four row results.
constexpr int kDppRowMirror = 0x140;   // row_mirror: lane i <-> 15-i within 16
__device__ __forceinline__ uint32_t wave_xor(uint32_t x) {
  x ^= dpp_u32<kDppQuadXor1>(x);
  x ^= dpp_u32<kDppQuadXor2>(x);
  x ^= dpp_u32<kDppHalfMirror>(x);
  x ^= dpp_u32<kDppRowMirror>(x);
  // rows 1 / 3 take lane 15 of rows 0 / 2 (row_bcast:15), then rows 2-3 take
  // lane 31 (row_bcast:31): lane 63 holds the wave's XOR, one readlane instead
  // of four plus three scalar XORs (layered MS -0.7 %, layered BP -0.5 % per
  // launch, profiles/r06/r06w_ab_wave_xor_bcast.json)
  x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);
  x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

}  // namespace qldpc
