// osd_order.h — osd_order_kernel<EPL>; the one OSD kernel that uses qldpc_libm.h (LDS: osd_order_lds, osd_kernels.hip).
#pragma once
#include "osd_kernels.h"
#include "../../include/qldpc_libm.h"

namespace qldpc {

// ---------------------------------------------------------------------------
// Reliability order of one shot per wavefront: NumPy's own (decoders.py:
// 320-325), bit for bit and tie for tie. Keys by qldpc_osd_key_t (SVML exp8_ha
// restated, include/qldpc_libm.h); the order by x86-simd-sort's argsort as
// NumPy 2.2.6 dispatches it on AVX512_SKX (np_order.cpp states the algorithm
// and is its host twin). LDS holds the keys and indices in their current
// arrangement (both move together); segments come off a small stack:
//   * > 256 keys (argpartition_unrolled<4>): the pivot (5th smallest of 8
//     samples, every lane sorts the same 8); the (size % 32) scalar steps as a
//     walk over two 32-lane streams (left end, right end) whose comparisons
//     are one ballot — a scalar loop assigns each touched key its slot; the
//     32-aligned middle as ballots per 64-key row (8 vectors); x86-simd-sort's
//     block schedule (left or right end, by the store counts so far) as a
//     scalar loop over the blocks' counts held in lanes (readlane), giving each
//     8-key vector its store offsets; every key to its slot;
//   * <= 256 keys (argsort_n): the bitonic network in registers, 4 keys per
//     lane, flip + half-cleaner stages over max(8, 2^ceil) slots with +inf
//     pads; comparators swap only when the upper key is strictly smaller.
// tiepos = n for an exact order, -1 where NumPy's order is left to the host:
// a NaN key, or x86-simd-sort's std::sort fallback after 2 floor(log2 n)
// levels (not restated).
// ---------------------------------------------------------------------------
__constant__ double kExpHL[32] = QLDPC_EXP_HL_INIT;

// A key and its index travel as one 64-bit word: w = u << 11 | i, u =
// bits(key) - bits(0.5) (key in [0.5, 1]: u <= 2^52, order-preserving), i < 2048.
// Comparisons look at the key part only — equal keys compare equal whatever
// their indices, exactly as x86-simd-sort compares the float64 keys:
//   key(b) < key(a)  <=>  (b | 0x7ff) < (a & ~0x7ff)
constexpr uint64_t kOrdIdx = 0x7ffull;
__device__ __forceinline__ bool ord_less(uint64_t b, uint64_t a) { return (b | kOrdIdx) < (a & ~kOrdIdx); }

// compare-exchange of two registers of one lane (positions lo < hi)
__device__ __forceinline__ void ord_cx(uint64_t& lo, uint64_t& hi) {
  const bool sw = ord_less(hi, lo);
  const uint64_t t = lo;
  lo = sw ? hi : lo;
  hi = sw ? t : hi;
}

// within-lane stage: partner position x ^ M, M in {1, 2, 3}. Every stage is
// a compile-time instance: with the partner pattern a run-time value, the
// compiler kept the four words in scratch memory and addressed them by it.
template <int M>
__device__ __forceinline__ void ord_within(uint64_t (&w)[4]) {
  if constexpr (M == 1) {
    ord_cx(w[0], w[1]);
    ord_cx(w[2], w[3]);
  } else if constexpr (M == 2) {
    ord_cx(w[0], w[2]);
    ord_cx(w[1], w[3]);
  } else {
    ord_cx(w[0], w[3]);
    ord_cx(w[1], w[2]);
  }
}

// cross-lane stage: partner position x ^ m, m >= 4: lane ^ LM (LM = m >> 2),
// register r ^ M3 (M3 = m & 3); HB = the highest bit of LM decides which side
// is the lower position
template <int LM, int HB, int M3>
__device__ __forceinline__ void ord_cross(uint64_t (&w)[4], int lane) {
  const bool lo = (lane & HB) == 0;
  uint64_t nw[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t pw = __shfl_xor(w[r ^ M3], LM, 64);
    const bool take = lo ? ord_less(pw, w[r]) : ord_less(w[r], pw);
    nw[r] = take ? pw : w[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r] = nw[r];
}

// half-cleaners J, J/2 .. 1
template <int J>
__device__ __forceinline__ void ord_half(uint64_t (&w)[4], int lane) {
  if constexpr (J >= 4) ord_cross<J / 4, J / 4, 0>(w, lane);
  else if constexpr (J >= 1) ord_within<J>(w);
  if constexpr (J > 1) ord_half<J / 2>(w, lane);
}

// bitonic merge of blocks of KK: flip(KK), then half-cleaners KK/4 .. 1
template <int KK>
__device__ __forceinline__ void ord_merge(uint64_t (&w)[4], int lane) {
  if constexpr (KK <= 4) ord_within<KK - 1>(w);              // flip(2) = x ^ 1, flip(4) = x ^ 3
  else ord_cross<(KK - 1) / 4, KK / 8, 3>(w, lane);          // flip(KK) = x ^ (KK - 1)
  if constexpr (KK >= 4) ord_half<KK / 4>(w, lane);
}

// argsort_n on positions [L, L + N), N <= 256, in registers
__device__ __forceinline__ void ord_small(uint64_t* W, int L, int N, int lane) {
  uint64_t w[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int x = 4 * lane + r;
    const uint64_t v = W[L + (x < N ? x : 0)];
    w[r] = x < N ? v : ~0ull;                               // +inf pads
  }
  // stages up to P = max(8, 2^ceil(log2 N)) (uniform branches)
  ord_merge<2>(w, lane);
  ord_merge<4>(w, lane);
  ord_merge<8>(w, lane);
  if (N > 8) ord_merge<16>(w, lane);
  if (N > 16) ord_merge<32>(w, lane);
  if (N > 32) ord_merge<64>(w, lane);
  if (N > 64) ord_merge<128>(w, lane);
  if (N > 128) ord_merge<256>(w, lane);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int x = 4 * lane + r;
    if (x < N) W[L + x] = w[r];
  }
}

__device__ __forceinline__ void ord_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

template <int EPL>                                          // keys per lane capacity: n <= 64 EPL
__global__ void __launch_bounds__(64) osd_order_kernel(OrderArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int n = a.n;
  uint64_t* W = (uint64_t*)lds;                              // [n] (key, index) words, current arrangement
  int* stk = (int*)(W + n);                                  // [32][3] (L, R, iters)
  uint16_t* VL = (uint16_t*)(stk + 96);                      // [256] per vector: lt store base
  uint16_t* VR = VL + 256;                                   // [256] per vector: ge store end
  const int lane = threadIdx.x;
  const long long shot = blockIdx.x;
  const double* post = a.post + shot * (long long)n;
  int32_t* perm = a.perm + shot * (long long)n;

  bool nan = false;
  for (int i = lane; i < n; i += 64) {
    const double k = qldpc_osd_key_t(post[i], kExpHL);
    nan |= k != k;
    W[i] = ((__builtin_bit_cast(uint64_t, k) - 0x3FE0000000000000ull) << 11) | (uint64_t)i;
  }
  bool fallback = __ballot(nan) != 0;                        // std_argsort_withnan: the host's
  int lg = 0;
  while ((2 << lg) <= n) ++lg;                               // floor(log2 n)
  int sp = 0;
  if (n > 1 && !fallback) {
    if (lane == 0) {
      stk[0] = 0;
      stk[1] = n - 1;
      stk[2] = 2 * lg;
    }
    sp = 1;
  }
  ord_fence();
  while (sp > 0 && !fallback) {
    --sp;
    const int L = __builtin_amdgcn_readfirstlane(stk[3 * sp]);
    const int R = __builtin_amdgcn_readfirstlane(stk[3 * sp + 1]);
    const int it = __builtin_amdgcn_readfirstlane(stk[3 * sp + 2]);
    if (it <= 0) {                                           // argsort_64bit_: std_argsort
      fallback = true;
      break;
    }
    if (R + 1 - L <= 256) {
      if constexpr ((QLDPC_ABLATE_ORD & 1) == 0) ord_small(W, L, R + 1 - L, lane);
      ord_fence();
      continue;
    }
    if constexpr ((QLDPC_ABLATE_ORD & 2) != 0) continue;
    // ---- argpartition_unrolled<4> ----
    // pivot: the 5th smallest key of the 8 samples (every lane sorts the same
    // words; equal keys in any order give the same key)
    const int q = (R - L) >> 3;
    uint64_t sm[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sm[i] = W[L + q * (i + 1)];
#pragma unroll
    for (int i = 1; i < 8; ++i)
#pragma unroll
      for (int j = i; j > 0; --j) {
        const uint64_t lo = sm[j - 1], hi = sm[j];
        sm[j - 1] = lo < hi ? lo : hi;
        sm[j] = lo < hi ? hi : lo;
      }
    const uint64_t pf = sm[4] & ~kOrdIdx;                    // key < pivot <=> w < pf
    const uint64_t pc = pf | kOrdIdx;                        // key > pivot <=> w > pc
    bool lt = false, gt = false;
    int left = L, right = R + 1;
    const int rem = (R + 1 - L) & 31;
    if (rem) {
      // the scalar steps: examine the key at `left`; < pivot: it stays, left
      // advances (the next key is the next of the left stream); >= pivot: it
      // swaps with the key at --right (the right stream's next), which is
      // examined next. Lane i < 32 holds left-stream key i (position L + i),
      // lane 32 + i right-stream key i (position R - i).
      const int pos = lane < 32 ? L + lane : R - (lane - 32);
      const uint64_t wv = W[pos];
      const uint64_t ltm = __ballot(wv < pf);
      int cur = 0, dest = -1;
      bool ex = false;
      for (int s = 0; s < rem; ++s) {
        if (lane == cur) ex = true;
        if ((ltm >> cur) & 1ull) {
          if (lane == cur) dest = left;
          ++left;
          cur = left - L;
        } else {
          --right;
          if (lane == cur) dest = right;
          cur = 32 + (R - right);
        }
      }
      if (lane == cur) dest = left;                          // moved to `left`, not examined
      lt |= ex && wv < pf;
      gt |= ex && wv > pc;
      if (dest >= 0) W[dest] = wv;
      ord_fence();
    }
    // the 32-aligned middle [left, right): rows of 64 keys (8 vectors)
    const int M = right - left, nb = M >> 5;
    uint64_t ev[EPL];
    uint32_t byt[(EPL + 3) / 4];                             // row r's vector byte at bits 8 (r % 4)
    uint32_t mym = 0;
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      if (64 * r >= M) break;
      const int o = 64 * r + lane;
      ev[r] = W[left + (o < M ? o : 0)];
    }
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      if (64 * r >= M) break;
      const bool valid = 64 * r + lane < M;
      lt |= valid && ev[r] < pf;
      gt |= valid && ev[r] > pc;
      const uint64_t bm = __ballot(valid && ev[r] >= pf);
      if ((lane >> 1) == r) mym = (lane & 1) ? (uint32_t)(bm >> 32) : (uint32_t)bm;
      const uint32_t by = (uint32_t)(bm >> (lane & 56)) & 0xffu;
      byt[r / 4] = (r % 4 ? byt[r / 4] : 0u) | (by << (8 * (r % 4)));
    }
    // x86-simd-sort's block schedule: blocks 1 .. nb-2 from the left or the
    // right end, then the held-back first and last blocks
    const int g = __builtin_popcount(mym);                   // lane b: >= pivot keys of block b
    int lsto = left, rend = right, lp = left + 32, rp = right - 32;
    int myl = 0, myr = 0;
    for (int step = 0; step < nb; ++step) {
      int b;
      if (step < nb - 2) {
        if (rend - rp < lp - lsto) {
          rp -= 32;
          b = (rp - left) >> 5;
        } else {
          b = (lp - left) >> 5;
          lp += 32;
        }
      } else {
        b = step == nb - 2 ? 0 : nb - 1;
      }
      if (lane == b) {
        myl = lsto;
        myr = rend;
      }
      const int gb = __builtin_amdgcn_readlane(g, b);
      lsto += 32 - gb;
      rend -= gb;
    }
    const int pidx = lsto;
    if (lane < nb) {
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int c = __builtin_popcount((mym >> (8 * ii)) & 0xffu);
        VL[4 * lane + ii] = (uint16_t)myl;
        VR[4 * lane + ii] = (uint16_t)myr;
        myl += 8 - c;
        myr -= c;
      }
    }
    ord_fence();
#pragma unroll
    for (int r = 0; r < EPL; ++r) {
      if (64 * r >= M) break;
      const int o = 64 * r + lane;
      const int v = o < M ? o >> 3 : 0;
      const int vl = VL[v], vr = VR[v];
      if (o < M) {
        const int kk = o & 7;
        const uint32_t byte = (byt[r / 4] >> (8 * (r % 4))) & 0xffu;
        const uint32_t below = byte & ((1u << kk) - 1u);
        const int dst = (byte >> kk) & 1u ? vr - __builtin_popcount(byte) + __builtin_popcount(below)
                                          : vl + kk - __builtin_popcount(below);
        W[dst] = ev[r];
      }
    }
    ord_fence();
    // children: pivot != smallest -> the left part, pivot != biggest -> the right part
    const bool lany = __ballot(lt) != 0, gany = __ballot(gt) != 0;
    if (lane == 0) {
      if (lany) {
        stk[3 * sp] = L;
        stk[3 * sp + 1] = pidx - 1;
        stk[3 * sp + 2] = it - 1;
      }
      if (gany) {
        const int s2 = sp + (lany ? 1 : 0);
        stk[3 * s2] = pidx;
        stk[3 * s2 + 1] = R;
        stk[3 * s2 + 2] = it - 1;
      }
    }
    sp += (lany ? 1 : 0) + (gany ? 1 : 0);
    ord_fence();
  }
  for (int i = lane; i < n; i += 64) perm[i] = (int32_t)(W[i] & kOrdIdx);
  if (lane == 0) a.tiepos[shot] = fallback ? -1 : n;
}

}  // namespace qldpc
