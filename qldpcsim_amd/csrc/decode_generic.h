// decode_generic.h — the generic check and variable node (any row degree, MS
// and BP, with the unrolled uniform-degree min-sum check node the other
// families reuse), and the three one-wave-per-half-shot LDS kernels built on
// them: decode_kernel and its two prior twins.
#pragma once
#include "decoder_common.h"

namespace qldpc {

struct LdsView {
  const uint32_t* cn_tab;   // [E] (relabeled var << 16) | csc position, CSR edge order
  const uint16_t* row_ptr;  // [m+1]
  const uint32_t* vn_info;  // [n]   csc start | degree << 16
  const uint8_t* chunk_dmax; // [ceil(n/64)] max degree of relabeled variables 64c..64c+63
  const uint16_t* vn_chk;   // [E]   check of each CSC position (layered)
  const uint16_t* lay_ptr;  // [L+1]
  const uint16_t* lay_rows; // [*]
  const uint16_t* adj_ptr;  // [L+1]
  const uint16_t* adj_vars; // [*]
  const qldpc_libm_tab* lt; // BP: NumPy libm tables (LDS)
};

// Graph table entry formats (capi_schedule.cpp builds them):
//  DC == 0 (generic):   cn_tab[row_ptr[c] + k] = (relabeled var << 16) | csc position
//  DC  > 0 (uniform row degree DC, rows padded to 8 entries, 16-byte aligned):
//                       cn_tab[8c + k] = (4 * csc position) << 16 | (8 * relabeled var)
//                       i.e. ready-made LDS byte offsets into c2v (f32) and post (f64).
template <int DC>
__device__ __forceinline__ int tab_var(uint32_t t) { return DC ? (int)((t & 0xffffu) >> 3) : (int)(t >> 16); }
template <int DC>
__device__ __forceinline__ int tab_pos(uint32_t t) { return DC ? (int)(t >> 18) : (int)(t & 0xffffu); }

// ---------------------------------------------------------------------------
// Min-sum check-node update for a uniform-degree code (DC = 7 or 8), the hot
// loop of the headline workload (decoders.py:155-169 for one row):
//   v_e   = post_j - c2v_e  (float64; FIRST: float32(L), :148-149)
//   min1 / first argmin / min2 of |v_e|, sign product with the syndrome sign
//   c2v_e = fl32(beta * (e == argmin ? min2 : min1)) with sign syn*prod*sign_e
// Signs and the parity of the hard decisions are folded from the high words
// (v_e is never -0.0 and post never -0.0 or NaN for finite L: DESIGN.md §4).
// Returns the check's "unsatisfied" bit for the posteriors it read.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void load_row8(const uint32_t* tab, uint32_t (&t)[8]) {
  const uint4 t0 = *(const uint4*)tab;
  const uint4 t1 = *(const uint4*)(tab + 4);
  t[0] = t0.x; t[1] = t0.y; t[2] = t0.z; t[3] = t0.w;
  t[4] = t1.x; t[5] = t1.y; t[6] = t1.z; t[7] = t1.w;
}

// Min-sum check-node update of one uniform-degree check (decoders.py:155-169)
// whose edges are given as absolute LDS byte addresses (pa: post f64, ca: c2v
// f32). `live` = 0 for a pad check (its writes land in the pad; flags masked).
template <int DC>
struct CnLoad {
  double pj[DC];
  float cv[DC];
};

template <int DC>
__device__ __forceinline__ void cn_ms_load(CnLoad<DC>& L, const uint32_t* pa, const uint32_t* ca) {
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    L.pj[k] = *QLDPC_LDS(const double, pa[k]);
    L.cv[k] = *QLDPC_LDS(const float, ca[k]);
  }
}

template <int DC>
__device__ __forceinline__ uint32_t cn_ms_compute(const DecodeArgs& a, const CnLoad<DC>& L, const uint32_t* ca,
                                                  uint32_t synb, uint32_t live, int& fl) {
  double v[DC];
  uint32_t hv[DC], hp[DC];
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    v[k] = L.pj[k] - (double)L.cv[k];                     // v2c = post - c2v (:177)
    hv[k] = hi_word(v[k]);
    hp[k] = hi_word(L.pj[k]);
  }
  double min1, min2;                                      // first min / min of the rest (:160-164)
  min12_tree<DC>(v, min1, min2);
  const uint32_t ph = xor_tree<DC>(hp);                   // hard-decision parity (:174)
  const uint32_t sh = xor_tree<DC>(hv);                   // np.sign product (:157-159)
  double m1 = min1, m2 = min2;
  // Rare cases behind one wave-uniform test: an infinite min (min2 = inf
  // whenever min1 is) and a zero min (min1 = 0, App. A.1.6 leak case, flagged).
  if (__builtin_expect(ballot((min1 == 0.0) | (min2 == __builtin_inf())) != 0, 0)) {
    m1 = __builtin_isinf(min1) ? 0.0 : min1;              // (:165)
    m2 = __builtin_isinf(min2) ? 0.0 : min2;              // (:166)
    if (m1 == 0.0 && live) fl |= FLAG_MIN_ZERO;
  }
  const uint32_t npm = ((sh >> 31) ^ synb) << 31;
  // c2v_e = fl32(beta * (|v_e| == min1 ? min2 : min1)), sign syn * prod *
  // sign_e (:167-168). The reference gives min2 to the first argmin only;
  // "every edge equal to min1" is the same thing: with a tie min2 == min1.
  const uint32_t c1n = opaque_always(__builtin_bit_cast(uint32_t, (float)(a.beta * m1)) ^ npm);
  const uint32_t c2n = opaque_always(__builtin_bit_cast(uint32_t, (float)(a.beta * m2)) ^ npm);
#pragma unroll
  for (int k = 0; k < DC; ++k) {
    const uint32_t c = (__builtin_fabs(v[k]) == min1) ? c2n : c1n;
    *QLDPC_LDS(uint32_t, ca[k]) = c ^ (hv[k] & 0x80000000u);
  }
  return ((ph >> 31) ^ synb) & live;
}

template <int DC>
__device__ __forceinline__ uint32_t cn_ms_abs(const DecodeArgs& a, const uint32_t* pa, const uint32_t* ca,
                                              uint32_t synb, uint32_t live, int& fl) {
  CnLoad<DC> L;
  cn_ms_load<DC>(L, pa, ca);
  return cn_ms_compute<DC>(a, L, ca, synb, live, fl);
}

// NC independent checks per call: every LDS read of all NC checks is issued
// before any arithmetic. `t[q]` holds check q's 8 table words (registers).
template <int DC, bool FIRST, int NC>
__device__ __forceinline__ uint32_t cn_ms_uniform(const DecodeArgs& a, const uint32_t (*t)[8],
                                                  const uint32_t* synb, const bool* live,
                                                  const unsigned char* post_b,
                                                  unsigned char* c2v_b, int& fl) {
  static_assert(DC >= 2 && DC <= 8, "uniform fast path handles row degrees 2..8");
  if constexpr (FIRST) {
    // every v_e = float32(L): min1 = min2 = |L32|, argmin 0, sign_e = L32 < 0
    const double vf = (double)a.L32;
    const double av = __builtin_fabs(vf);
    const float c = (float)(a.beta * av);
    const uint32_t neg = (uint32_t)(vf < 0.0);
    if (av == 0.0) fl |= FLAG_MIN_ZERO;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const uint32_t negprod = ((neg * DC) ^ synb[q]) & 1u;
      const float val = (neg ^ negprod) ? -c : c;
      if (live[q]) {
#pragma unroll
        for (int k = 0; k < DC; ++k) *(float*)(c2v_b + (t[q][k] >> 16)) = val;
      }
    }
    return 0;
  } else {
    // the flooding kernel's check node (cn_ms_load / cn_ms_compute) on
    // addresses formed from the packed table words
    uint32_t unsat = 0;
    const uint32_t pb = lds_addr(post_b), cb = lds_addr(c2v_b);
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      uint32_t pa[8], ca[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        pa[k] = pb + (t[q][k] & 0xffffu);
        ca[k] = cb + (t[q][k] >> 16);
      }
      if (live[q]) {
        CnLoad<DC> L;
        cn_ms_load<DC>(L, pa, ca);
        unsat |= cn_ms_compute<DC>(a, L, ca, synb[q], 1u, fl);
      }
    }
    return unsat;
  }
}

// Where a variable's prior comes from (PRI). PRI_MASK, two-level priors
// (decode_prior_kernel): bit j of `selw` (this wave's LDS slice, relabeled
// variable order) picks variable j's prior, L (bit 0) or L1 (bit 1). PRI_ROW,
// per-variable priors (decode_vprior_kernel): `selw` is the workgroup's LDS
// copy of the code's prior row, float64 [n] in relabeled order, and variable
// j's prior is one read of it. PRI_SCALAR: every variable's prior is a.L.
enum { PRI_SCALAR = 0, PRI_MASK = 1, PRI_ROW = 2 };
template <int PRI>
__device__ __forceinline__ double prior_of(const DecodeArgs& a, const uint32_t* selw, int j) {
  if constexpr (PRI == PRI_ROW) return ((const double*)selw)[j];
  if constexpr (PRI == PRI_MASK) return ((selw[j >> 5] >> (j & 31)) & 1u) ? a.L1 : a.L;
  return a.L;
}
// Mask bit of original column jo of half-shot hs (DecodeArgs::pmask)
__device__ __forceinline__ uint32_t pmask_bit(const DecodeArgs& a, long long hs, int jo) {
  if (a.pmask_bits) return (uint32_t)(((const uint64_t*)a.pmask)[hs * a.wn + (jo >> 6)] >> (jo & 63)) & 1u;
  return ((const uint8_t*)a.pmask)[hs * (long long)a.n + jo] & 1u;
}

// Check-node update of one check `c` (lane-local), any degree.
//   MS: decoders.py:155-169.  BP: decoders.py:249-262.
// Returns the check's current parity XOR syndrome bit ("unsatisfied"),
// computed from the hard decisions of the posteriors it reads (only
// meaningful when !first).
// ---------------------------------------------------------------------------
template <int ALGO, int DC, int PRI = PRI_SCALAR>
__device__ __forceinline__ uint32_t cn_update(const DecodeArgs& a, const LdsView& g, int c,
                                              uint32_t synb, bool first, const double* post,
                                              void* c2v_raw, int& fl, const uint32_t* selw = nullptr) {
  if constexpr (ALGO == ALGO_MS && DC > 0) {
    uint32_t t[1][8];
    load_row8(g.cn_tab + c * 8, t[0]);
    if constexpr (PRI) {
      if (first) {
        // v_e = float32(L_j) differs per edge: the general check node on those
        // values (c2v = 0) instead of the uniform closed form; parity unused
        CnLoad<DC> L;
        uint32_t ca[DC];
        const uint32_t cb = lds_addr(c2v_raw);
#pragma unroll
        for (int k = 0; k < DC; ++k) {
          L.pj[k] = (double)(float)prior_of<PRI>(a, selw, tab_var<DC>(t[0][k]));
          L.cv[k] = 0.0f;
          ca[k] = cb + (t[0][k] >> 16);
        }
        (void)cn_ms_compute<DC>(a, L, ca, synb, 1u, fl);
        return 0;
      }
    }
    const uint32_t sb[1] = {synb};
    const bool live[1] = {true};
    if (first) return cn_ms_uniform<DC, true, 1>(a, t, sb, live, (const unsigned char*)post, (unsigned char*)c2v_raw, fl);
    return cn_ms_uniform<DC, false, 1>(a, t, sb, live, (const unsigned char*)post, (unsigned char*)c2v_raw, fl);
  }
  const int e0 = DC ? c * 8 : (int)g.row_ptr[c];
  const int deg = DC ? DC : (int)g.row_ptr[c + 1] - e0;
  uint32_t par = 0;
  if constexpr (ALGO == ALGO_MS) {
    float* c2v = (float*)c2v_raw;
    double min1 = __builtin_inf(), min2 = __builtin_inf();
    int idx = 0;
    uint32_t negm = 0;
    const double vfirst = (double)a.L32;
    for (int k = 0; k < deg; ++k) {
      const uint32_t t = g.cn_tab[e0 + k];
      const int j = tab_var<DC>(t), pos = tab_pos<DC>(t);
      double v;
      if (first) {
        v = PRI ? (double)(float)prior_of<PRI>(a, selw, j) : vfirst;   // float32(L) (:148-149)
      } else {
        const double pj = post[j];
        par ^= (uint32_t)(pj < 0.0);                  // hard decision (:174)
        v = pj - (double)c2v[pos];                    // v2c = post - c2v (:177)
      }
      negm |= (uint32_t)(v < 0.0) << k;              // np.sign, 0 -> +1 (:157-158)
      const double av = __builtin_fabs(v);
      idx = (av < min1) ? k : idx;                   // first argmin (:161)
      min2 = __builtin_fmin(min2, __builtin_fmax(min1, av));  // min of the rest (:162-164)
      min1 = __builtin_fmin(min1, av);
    }
    if (deg == 0) return synb;                       // no edges: c2v stays 0
    if (__builtin_isinf(min1)) min1 = 0.0;           // (:165)
    if (__builtin_isinf(min2)) min2 = 0.0;           // (:166)
    if (min1 == 0.0) fl |= FLAG_MIN_ZERO;            // App. A.1.6 leak case (flagged, not emulated)
    const uint32_t negprod = (uint32_t)(__builtin_popcount(negm) & 1) ^ synb;
    // c2v_e = fl32(beta * syn * prod * min_e / sign_e): magnitude rounded from
    // the float64 product once, sign = syn * prod * sign_e (:167-168).
    const float c1 = (float)(a.beta * min1), c2 = (float)(a.beta * min2);
    for (int k = 0; k < deg; ++k) {
      const int pos = tab_pos<DC>(g.cn_tab[e0 + k]);
      const float mag = (k == idx) ? c2 : c1;
      c2v[pos] = (((negm >> k) & 1u) ^ negprod) ? -mag : mag;
    }
  } else {
    double* c2v = (double*)c2v_raw;
    if (deg == 0) return synb;                       // `continue` (:251-252)
    double prod = 1.0;
#pragma unroll
    for (int k = 0; k < (DC ? DC : 32); ++k) {
      if (!DC && k >= deg) break;
      const uint32_t t = g.cn_tab[e0 + k];
      const int j = tab_var<DC>(t), pos = tab_pos<DC>(t);
      const double pj = post[j];
      par ^= (uint32_t)(pj < 0.0);
      const double v = pj - c2v[pos];                // v2c (:269)
      const double th = qldpc_tanh_t(v / 2.0, g.lt->tanh_c);   // (:254) np.tanh
      prod *= th;                                    // np.prod: sequential fold
      c2v[pos] = th;                                 // scratch: own edge, rewritten below
    }
    if (!DC && deg > 32) {
      // generic degrees > 32: second half of the fold (rare; bicycle = 18)
      for (int k = 32; k < deg; ++k) {
        const uint32_t t = g.cn_tab[e0 + k];
        const int j = tab_var<DC>(t), pos = tab_pos<DC>(t);
        const double pj = post[j];
        par ^= (uint32_t)(pj < 0.0);
        const double th = qldpc_tanh_t((pj - c2v[pos]) / 2.0, g.lt->tanh_c);
        prod *= th;
        c2v[pos] = th;
      }
    }
    const double lim = 1.0 - a.eps;
    for (int k = 0; k < deg; ++k) {
      const int pos = tab_pos<DC>(g.cn_tab[e0 + k]);
      const double th = c2v[pos];
      if (th == 0.0) fl |= FLAG_NONFINITE;
      double th2 = prod / th;                        // (:256)
      if (__builtin_fabs(th2) >= lim)                // (:257-258)
        th2 = th2 - a.eps * (th2 > 0.0 ? 1.0 : (th2 < 0.0 ? -1.0 : 0.0));
      double val = 2.0 * qldpc_atanh_t(th2, g.lt->atanh_hl, g.lt->atanh_rcp);   // (:259) np.arctanh
      if (synb) val = -val;                          // (:260-261)
      if (!__builtin_isfinite(val)) fl |= FLAG_NONFINITE;
      c2v[pos] = val;
    }
  }
  return par ^ synb;
}

// Variable-node update of relabeled variable j: column sum in ascending check
// order. MS: float32 sequential (np.sum axis=0, decoders.py:172), post = L +
// (f64)S (:173). BP: np.sum pairwise rule, post = L0 + S (:269, :276).
// vn_info[j] = csc start | degree << 16.
template <int K>
__device__ __forceinline__ float ms_colsum(const float* c, int d) {
  // K unconditional loads (the c2v region is padded by 8 floats, so reading
  // past a short column stays inside this wave's slice), then the sequential
  // sum with the missing terms replaced by +0.0f — exact, since the running
  // sum starts at +0.0f and is never -0.0f.
  float x[K];
#pragma unroll
  for (int t = 0; t < K; ++t) x[t] = c[t];
  float s = 0.0f;
#pragma unroll
  for (int t = 0; t < K; ++t) s += (t < d) ? x[t] : 0.0f;
  return s;
}

// VN column sum with a wave-uniform degree bound dmax (unrolled loads).
__device__ __forceinline__ float ms_colsum_sw(const float* c, int d, int dmax) {
  switch (dmax) {
    case 0: return 0.0f;
    case 1: return ms_colsum<1>(c, d);
    case 2: return ms_colsum<2>(c, d);
    case 3: return ms_colsum<3>(c, d);
    case 4: return ms_colsum<4>(c, d);
    case 5: return ms_colsum<5>(c, d);
    case 6: return ms_colsum<6>(c, d);
    case 7: return ms_colsum<7>(c, d);
    case 8: return ms_colsum<8>(c, d);
    default: {
      float s = 0.0f;
      for (int t = 0; t < d; ++t) s += c[t];
      return s;
    }
  }
}

// dmax: wave-uniform upper bound of the degrees of the variables this pass
// covers (per 64-variable chunk, from the host), so the loads are unrolled.
template <int ALGO, int PRI = PRI_SCALAR>
__device__ __forceinline__ double vn_post(const DecodeArgs& a, const LdsView& g, int j,
                                          const void* c2v_raw, int dmax, const uint32_t* selw = nullptr) {
  const double Lj = prior_of<PRI>(a, selw, j);
  const uint32_t info = g.vn_info[j];
  const int p0 = (int)(info & 0xffffu), d = (int)(info >> 16);
  if constexpr (ALGO == ALGO_MS) {
    const float* c = (const float*)c2v_raw + p0;
    float s;
    switch (dmax) {
      case 0: s = 0.0f; break;
      case 1: s = ms_colsum<1>(c, d); break;
      case 2: s = ms_colsum<2>(c, d); break;
      case 3: s = ms_colsum<3>(c, d); break;
      case 4: s = ms_colsum<4>(c, d); break;
      case 5: s = ms_colsum<5>(c, d); break;
      case 6: s = ms_colsum<6>(c, d); break;
      case 7: s = ms_colsum<7>(c, d); break;
      case 8: s = ms_colsum<8>(c, d); break;
      default:
        s = 0.0f;
        for (int t = 0; t < d; ++t) s += c[t];
    }
    return Lj + (double)s;
  } else {
    const double* c2v = (const double*)c2v_raw;
    const double t = np_sum_col(c2v + p0, d);
    return d == 0 ? Lj : Lj + t;                     // L_post[j] = L0 (:277-278)
  }
}

// decode_kernel, its two-level-prior twin decode_prior_kernel (PRI_MASK:
// DecodeArgs::pmask / L1; instantiated in
// decode_prior_kernels.hip) and its per-variable-prior twin
// decode_vprior_kernel (PRI_ROW: DecodeArgs::vprior, DESIGN.md §3.12;
// decode_vprior_kernels.hip) share one body, decode_kernel_body.inc, included
// into each kernel: as a __device__ function taking the arguments, the same
// text compiled to different code for decode_kernel (register allocation of
// the by-value kernel arguments), and its code must stay what it was.
template <int ALGO, bool LAYERED, int DC>
__global__ void __launch_bounds__(QLDPC_MAX_THREADS) decode_kernel(DecodeArgs a) {
  constexpr int PRI = PRI_SCALAR;
  constexpr bool TALL = false;
#include "decode_kernel_body.inc"
}

template <int ALGO, bool LAYERED, int DC>
__global__ void __launch_bounds__(QLDPC_MAX_THREADS) decode_prior_kernel(DecodeArgs a) {
  constexpr int PRI = PRI_MASK;
  constexpr bool TALL = false;
#include "decode_kernel_body.inc"
}

template <int ALGO, bool LAYERED, int DC>
__global__ void __launch_bounds__(QLDPC_MAX_THREADS) decode_vprior_kernel(DecodeArgs a) {
  constexpr int PRI = PRI_ROW;
  constexpr bool TALL = false;
#include "decode_kernel_body.inc"
}

// Flooding with more than QLDPC_SYNREG_CHECKS checks (DC = 0: the fast table's
// 8 E < 65536 leaves row degree 7 / 8 at most 1170 checks): the same body with
// the syndrome bits in the slice's words instead of a register. Kernels of
// their own, so that the instances above stay instruction for instruction what
// they were.
template <int ALGO>
__global__ void __launch_bounds__(QLDPC_MAX_THREADS) decode_kernel_tall(DecodeArgs a) {
  constexpr int PRI = PRI_SCALAR, DC = 0;
  constexpr bool LAYERED = false, TALL = true;
#include "decode_kernel_body.inc"
}

template <int ALGO>
__global__ void __launch_bounds__(QLDPC_MAX_THREADS) decode_prior_kernel_tall(DecodeArgs a) {
  constexpr int PRI = PRI_MASK, DC = 0;
  constexpr bool LAYERED = false, TALL = true;
#include "decode_kernel_body.inc"
}

template <int ALGO>
__global__ void __launch_bounds__(QLDPC_MAX_THREADS) decode_vprior_kernel_tall(DecodeArgs a) {
  constexpr int PRI = PRI_ROW, DC = 0;
  constexpr bool LAYERED = false, TALL = true;
#include "decode_kernel_body.inc"
}

// The selector of one of the three kernels above, defined once per kernel in
// the translation unit that instantiates it: FN(algo, layered, dc, tall, &name)
// answers KERNEL<algo, layered, 7 | 8 | 0> (tall: KERNEL_tall<algo>, flooding
// and the generic table by necessity) and its name, the template arguments
// spelled as rocprofv3 prints them.
static_assert(ALGO_MS == 0 && ALGO_BP == 1, "the selector spells the algorithm as 0 / 1");
#define QLDPC_GENERIC_CASE(KERNEL, A, LAY, D) \
  if (al == A && layered == LAY && d == D) QLDPC_NAMED((&KERNEL<A, LAY, D>), #KERNEL "<" #A ", " #LAY ", " #D ">");
#define QLDPC_GENERIC_SELECTOR(FN, KERNEL)                                                      \
  const void* FN(int algo, bool layered, int dc, bool tall, const char** name) {                \
    const int al = algo == ALGO_MS ? 0 : 1, d = dc == 7 || dc == 8 ? dc : 0;                    \
    if (tall && (layered || d != 0)) return nullptr;                                            \
    if (tall && al == 0) QLDPC_NAMED((&KERNEL##_tall<0>), #KERNEL "_tall<0>");                  \
    if (tall) QLDPC_NAMED((&KERNEL##_tall<1>), #KERNEL "_tall<1>");                             \
    QLDPC_GENERIC_CASE(KERNEL, 0, true, 7) QLDPC_GENERIC_CASE(KERNEL, 0, false, 7)              \
    QLDPC_GENERIC_CASE(KERNEL, 0, true, 8) QLDPC_GENERIC_CASE(KERNEL, 0, false, 8)              \
    QLDPC_GENERIC_CASE(KERNEL, 0, true, 0) QLDPC_GENERIC_CASE(KERNEL, 0, false, 0)              \
    QLDPC_GENERIC_CASE(KERNEL, 1, true, 7) QLDPC_GENERIC_CASE(KERNEL, 1, false, 7)              \
    QLDPC_GENERIC_CASE(KERNEL, 1, true, 8) QLDPC_GENERIC_CASE(KERNEL, 1, false, 8)              \
    QLDPC_GENERIC_CASE(KERNEL, 1, true, 0) QLDPC_GENERIC_CASE(KERNEL, 1, false, 0)              \
    return nullptr;                                                                             \
  }

}  // namespace qldpc
