// bp_team.h — bp_team_kernel and bp_team_lg_kernel (instantiated in
// bp_team_kernels.hip).
#pragma once
#include "decode_generic.h"

namespace qldpc {

// ---------------------------------------------------------------------------
// Sum-product BP for uniform row degree DC (7 or 8): one TEAM of W wavefronts
// (one workgroup) decodes one half-shot, with the check-node update spread
// over the edges — 8 lanes per check, lane k owns edge k — instead of a lane
// per check. Same arithmetic, same results as decode_kernel<BP, …, DC>, bit
// for bit (decoders.py:249-262 per check):
//   t_k  = tanh(v_k / 2)                 one lane per edge
//   P    = ((t_0 t_1) t_2) ... t_{d-1}   np.prod's sequential fold, carried
//                                        lane to lane by d-1 shuffles
//   c2v_k = ±2 atanh(clip(P / t_k))       one lane per edge
// Why: BP's float64 state is large (LP118_2: 37 KB per half-shot), so a
// one-wave-per-half-shot kernel runs 3-7 waves per CU and stalls on the long
// dependent tanh / atanh chains (30-60 % VALU busy). A team puts 4-8x the
// lanes on one half-shot's state: more waves per CU for the same LDS, and a
// layered layer (30-60 checks) becomes one pass of 8-lane groups.
// Variable nodes: one lane per variable (np.sum pairwise rule), as before.
// Team-wide stop tests go through LDS slots (double-buffered, one barrier);
// layered: parity filters posted per wave (see the layered branch).
// ---------------------------------------------------------------------------
// Saturated check nodes. NumPy's tanh is +-1.0 exactly for |x| >= 19.5: the
// interval [16, 24) evaluates 1 + y r(y) with |y r(y)| ~ 2 exp(-2|x|) <=
// 2.3e-17, below half an ulp of 1 (2^-54), and [24, inf) has the constant
// polynomial 1 (include/qldpc_numpy_tables.h; checked on the host restatement
// and against NumPy, tests/test_libm.py). When every edge of a check has
// |v2c / 2| >= 19.5, all its t_k are +-1, np.prod is +-1, th2 = P / t_k is
// +-1 and clips to +-(1 - eps) (decoders.py:256-258), so c2v_k = +-2
// atanh(1 - eps): one constant, DecodeArgs::bp_csat (capi_decode.cpp, the same
// restated atanh). A finite |x| is >= 19.5 iff its high word (sign cleared)
// is >= 0x40338000 (19.5's low word is 0): DecodeArgs::bp_sat_hi, or
// 0x7ff00000 (never) when the constant is not finite (eps <= 0: atanh(1)).

// edge k of a check whose table word t (row table entry 8c + k) is given;
// SAT: with the saturated-check fast path
template <int DC, bool SAT>
__device__ __forceinline__ uint32_t cn_bp_word(const DecodeArgs& a, const qldpc_libm_tab* lt, uint32_t t, bool valid,
                                               int k, int lane, uint32_t synb, const double* post, double* c2v,
                                               int& fl) {
  const bool ek = valid && k < DC;
  // a wave with no check of this pass skips it (uniform); inside, every lane
  // loads and computes (t = 0 for a pad edge / check: variable 0, position
  // 0, in bounds) and the pad lanes' values are replaced by selects — no
  // exec-masked branches around the loads and the tanh
  if (ballot_b(valid) == 0) return 0u;
  constexpr int CP = SAT ? QLDPC_BP_CNPRIO : QLDPC_BP_FCNPRIO;   // check-node phase priorities
  if constexpr (CP == 1 || CP == 2) __builtin_amdgcn_s_setprio(1);
  const int j = (int)((t & 0xffffu) >> 3), p = (int)(t >> 18);
  const double pjr = post[j];
  const double x = (pjr - c2v[p]) / 2.0;                      // v2c (:269)
  // saturated (finite, |x| >= 19.5): the high word (sign cleared) in
  // [bp_sat_hi, 0x7ff00000), one unsigned compare after the subtraction
  const uint32_t xh = (uint32_t)(__builtin_bit_cast(uint64_t, x) >> 32) & 0x7fffffffu;
  const uint32_t shi = a.bp_sat_hi;
  const bool unsat = xh - shi >= 0x7ff00000u - shi;
  if (SAT && ballot_b(ek & unsat) == 0) {
    // every edge of the wave's checks saturated: t_k = sign(x_k), P = the
    // product of the group's signs (pad edges: +1), the message's sign =
    // sign(P / t_k), then the syndrome's (:260-261)
    const double csat = kargs_fresh<DecodeArgs>().bp_csat;
    const uint64_t nb = ballot_b(ek && x < 0.0);
    const uint32_t gs = (uint32_t)(nb >> (lane & 56)) & 0xffu;
    const uint32_t neg = ((uint32_t)__builtin_popcount(gs) ^ (gs >> (lane & 7)) ^ synb) & 1u;
    if (ek) c2v[p] = neg ? -csat : csat;
    const uint64_t hb = ballot_b(ek && pjr < 0.0);
    const uint32_t par = (uint32_t)__builtin_popcount((uint32_t)(hb >> (lane & 56)) & 0xffu) & 1u;
    if constexpr (CP == 1 || CP == 2) __builtin_amdgcn_s_setprio(0);
    return valid ? (par ^ synb) : 0u;
  }
  double th;                                                  // np.tanh (:254)
  if (__builtin_expect(ballot_b(!(__builtin_fabs(x) < 0x1p1023)) != 0, 0))
    th = qldpc_tanh_x(x, lt->tanh_c, 0);                      // a NaN / huge argument in the wave
  else
    th = qldpc_tanh_x(x, lt->tanh_c, 1);
  th = ek ? th : 1.0;
  if constexpr (CP == 1) __builtin_amdgcn_s_setprio(0);
  const double pj = ek ? pjr : 0.0;
  // np.prod: sequential left fold over the check's edges in ascending variable
  // order, ((t_0 t_1) t_2) ..., formed redundantly by every lane of the group
  // from the group's t values (one permute each): same rounding as a
  // lane-to-lane prefix chain, without its per-step index arithmetic, selects
  // and final broadcast (BP flooding is VALU-bound)
  const int base = lane & ~7;
  // (the permutes issued together before the fold, each waited for in turn
  // now: +1 % per BP-L launch through register spills, r06k_ab_cn_reads_bp_shfl.json)
  double P = __shfl(th, base, 64);
#pragma unroll
  for (int s = 1; s < DC; ++s) P = P * __shfl(th, base + s, 64);
  // parity of the hard decisions of the posteriors this check read (:283-285)
  const uint64_t hb = ballot_b(ek && pj < 0.0);
  const uint32_t par = (uint32_t)__builtin_popcount((uint32_t)(hb >> (lane & 56)) & 0xffu) & 1u;
  // Every lane computes (a pad lane: th = 1, its results discarded); only
  // the message store is guarded.
  // P / th (:256). QLDPC_DIV is IEEE division for nonzero operands in the
  // normal range (|th| <= 1 and |P| <= |th| here); a wave holding a zero
  // (a -0 product keeps its sign only through v_div_fixup), tiny or
  // non-finite one divides the general way.
  double th2;
  if (__builtin_expect(ballot_b(ek && !(__builtin_fabs(th) > 1e-150 && __builtin_fabs(P) > 1e-150)) != 0, 0))
    th2 = P / th;
  else
    th2 = QLDPC_DIV(P, th);
  // (:257-258): |th2| >= 1 - eps implies th2 != 0, so th2 - eps sign(th2)
  // is copysign(|th2| - eps, th2) (round-to-nearest is symmetric in sign;
  // a NaN compares false and stays)
  th2 = (__builtin_fabs(th2) >= 1.0 - a.eps) ? __builtin_copysign(__builtin_fabs(th2) - a.eps, th2) : th2;
  if constexpr (CP == 2) __builtin_amdgcn_s_setprio(0);
  if constexpr (CP == 3) __builtin_amdgcn_s_setprio(1);
  // np.arctanh (:259); SVML's rare path (|th2| >= 1, NaN) only when a lane
  // of the wave needs it
  double at;
  if (__builtin_expect(ballot_b(ek && !(__builtin_fabs(th2) < 1.0)) != 0, 0))
    at = qldpc_atanh_x(th2, lt->atanh_hl, lt->atanh_rcp, 0);
  else
    at = qldpc_atanh_x(th2, lt->atanh_hl, lt->atanh_rcp, 1);
  double val = 2.0 * at;
  if (synb) val = -val;                                   // (:260-261)
  if (ek && (th == 0.0 || !__builtin_isfinite(val))) fl |= FLAG_NONFINITE;
  if (ek) c2v[p] = val;
  if constexpr (CP == 3) __builtin_amdgcn_s_setprio(0);
  return valid ? (par ^ synb) : 0u;
}

template <int DC, bool SAT>
__device__ __forceinline__ uint32_t cn_bp_group(const DecodeArgs& a, const LdsView& g, int c, bool valid,
                                                int k, int lane, uint32_t synb, const double* post,
                                                double* c2v, int& fl) {
  const uint32_t tw = g.cn_tab[8 * c + k];                     // (c = 0 for a pad check)
  const uint32_t t = (valid && k < DC) ? tw : 0u;
  return cn_bp_word<DC, SAT>(a, g.lt, t, valid, k, lane, synb, post, c2v, fl);
}

// Every graph table in LDS: the flooding BP kernel (VALU-bound), and the
// layered fallback when the schedule has no global layer image (n > 2048 or a
// column degree > 31, capi_schedule.cpp); bp_team_lg_kernel is the layered default.
template <bool LAYERED, int DC, int W>
__global__ void __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(4))) bp_team_kernel(DecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  {
    const uint4* src = (const uint4*)a.blob;
    uint4* dst = (uint4*)lds;
    const int nvec = a.blob_bytes >> 4;
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) dst[i] = src[i];
  }
  LdsView g;
  g.lt = stage_libm(lds, a.off_libm);
  __syncthreads();
  g.cn_tab = (const uint32_t*)(lds + a.off_cn_tab);
  g.row_ptr = (const uint16_t*)(lds + a.off_row_ptr);
  g.vn_info = (const uint32_t*)(lds + a.off_vn_ptr);
  g.chunk_dmax = (const uint8_t*)(lds + a.off_chunk_dmax);
  g.vn_chk = (const uint16_t*)(lds + a.off_vn_chk);
  g.lay_ptr = (const uint16_t*)(lds + a.off_lay_ptr);
  g.lay_rows = (const uint16_t*)(lds + a.off_lay_rows);
  g.adj_ptr = (const uint16_t*)(lds + a.off_adj_ptr);
  g.adj_vars = (const uint16_t*)(lds + a.off_adj_vars);

  constexpr int TS = 64 * W;        // threads per team
  constexpr int GP = 8 * W;         // 8-lane check groups per pass
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int grp = tid >> 3, k = tid & 7;
  unsigned char* ws = lds + a.blob_bytes;
  double* post = (double*)ws;
  double* c2v = (double*)(ws + a.off_c2v);
  uint32_t* synw = (uint32_t*)(ws + a.off_synw);
  uint32_t* red = (uint32_t*)(ws + a.off_red);          // [2][W] any-slots, [2][2] tickets
  const int m = a.m, n = a.n;
  const double L = a.L;

  int rphase = 0;
  auto team_any = [&](bool pred) -> bool {              // one barrier
    const uint64_t b = ballot(pred);
    if (lane == 0) red[rphase * W + wid] = b != 0;
    __syncthreads();
    bool r = false;
#pragma unroll
    for (int w = 0; w < W; ++w) r |= red[rphase * W + w] != 0;
    rphase ^= 1;
    return r;
  };

  // team-level guided work queue (HalfShotQueue's policy, one ticket per team)
  long long hs = blockIdx.x, end = hs + 1;
  const long long stride = gridDim.x;
  uint32_t seen = 0, tlen = 1, tk = 0;
  int tphase = 0;
  while (hs < a.batch) {
    bool claimed = false;
    if (a.queue && hs + 1 == end) {
      const long long rem = a.batch - stride - (long long)seen;
      long long len = rem / (4 * stride);
      len = len < 1 ? 1 : (len > 64 ? 64 : len);
      tlen = (uint32_t)len;
      claimed = true;
      if (tid == 0) tk = atomicAdd(a.queue, tlen);
    }
    int fl = 0;
    int iters = a.max_iter;
    bool conv = false;

    // state: post = L, c2v = 0 (decoders.py:235-236); syndrome (and, layered,
    // initial parity) bit-words
    for (int j = tid; j < n; j += TS) post[j] = L;
    for (int p = tid; p < a.E; p += TS) c2v[p] = 0.0;
    team_syndrome_bits<2, TS>(a, hs, synw, tid);
    __syncthreads();

    if constexpr (!LAYERED) {
      for (int it = 0;; ++it) {
        uint32_t unsat = 0;
        for (int c0 = 0; c0 < m; c0 += GP) {
          const int c = c0 + grp;
          const bool valid = c < m;
          const uint32_t sb = valid ? (synw[c >> 5] >> (c & 31)) & 1u : 0u;
          unsat |= cn_bp_group<DC, false>(a, g, valid ? c : 0, valid, k, lane, sb, post, c2v, fl);
        }
        // the parity pass is the stop test of iteration it-1 (:283-285); its
        // team barrier also orders these c2v writes before the VN reads them
        if (it > 0) {
          if (!team_any(unsat != 0)) {
            iters = it;
            conv = true;
            break;
          }
        } else {
          __syncthreads();
        }
        for (int j = tid; j < n; j += TS) post[j] = vn_post<ALGO_BP>(a, g, j, c2v, -1);
        __syncthreads();
        if (it + 1 == a.max_iter) {
          uint32_t un = 0;
          for (int c = tid; c < m; c += TS) {
            uint32_t par = 0;
#pragma unroll
            for (int q = 0; q < DC; ++q) par ^= (uint32_t)(post[tab_var<DC>(g.cn_tab[8 * c + q])] < 0.0);
            un |= par ^ ((synw[c >> 5] >> (c & 31)) & 1u);
          }
          conv = !team_any(un != 0);
          break;
        }
      }
    } else {
      // Stop test after every layer (:283-285) by ms_layered_kernel's 32
      // parity filters: B = the syndrome's filter parities, F
      // = the hard decisions', kept current with the filter word of every
      // variable the VN flips; only F == B (convergence, or a 2^-32 false
      // match) runs the exact row check. Each wave posts its flips' XOR in a
      // slot read after the VN barrier, so a layer costs two team barriers,
      // not three, and no parity atomics.
      uint32_t bl = 0;
      for (int c = lane; c < m; c += 64) bl ^= ((synw[c >> 5] >> (c & 31)) & 1u) ? a.wc[c] : 0u;
      const uint32_t B = wave_xor(bl);
      uint32_t F = (L < 0.0) ? a.filt_all : 0u;           // every post starts at L
      uint32_t* fsl = red + 2 * W + 4;                    // [W] filter words of this layer's flips
      for (int it = 0; it < a.max_iter && !conv; ++it) {
        for (int l = 0; l < a.n_layers; ++l) {
          const int q0 = g.lay_ptr[l], q1 = g.lay_ptr[l + 1];
          for (int qb = q0; qb < q1; qb += GP) {
            const int q = qb + grp;
            const bool valid = q < q1;
            const int c = valid ? (int)g.lay_rows[q] : 0;
            const uint32_t sb = valid ? (synw[c >> 5] >> (c & 31)) & 1u : 0u;
            (void)cn_bp_group<DC, QLDPC_BP_SAT>(a, g, c, valid, k, lane, sb, post, c2v, fl);
          }
          __syncthreads();
          // VN over the layer's adjacent variables
          const int v0 = g.adj_ptr[l], v1 = g.adj_ptr[l + 1];
          uint32_t acc = 0;
          for (int q = v0 + tid; q < v1; q += TS) {
            const int j = g.adj_vars[q];
            const double old = post[j];
            const double nw = vn_post<ALGO_BP>(a, g, j, c2v, -1);
            post[j] = nw;
            if ((old < 0.0) != (nw < 0.0)) acc ^= a.avar[j];   // hard decision flipped
          }
          const uint32_t wacc = wave_xor(acc);
          if (lane == 0) fsl[wid] = wacc;
          __syncthreads();
#pragma unroll
          for (int w = 0; w < W; ++w) F ^= fsl[w];
          if (F == B) {                                   // team-uniform
            uint32_t un = 0;
            for (int c = tid; c < m; c += TS) {
              uint32_t par = 0;
#pragma unroll
              for (int q = 0; q < DC; ++q) par ^= (uint32_t)(post[tab_var<DC>(g.cn_tab[8 * c + q])] < 0.0);
              un |= par ^ ((synw[c >> 5] >> (c & 31)) & 1u);
            }
            if (!team_any(un != 0)) {
              iters = it + 1;
              conv = true;
              break;
            }
          }
        }
      }
    }
    write_outputs_strided<4, TS>(a, hs, tid, [&](int v) { return post[v]; });   // (:280)
    const bool nonfin = team_any((fl & FLAG_NONFINITE) != 0);
    if (tid == 0) {
      a.iters[hs] = iters;
      if (a.flags) a.flags[hs] = (int32_t)((nonfin ? FLAG_NONFINITE : 0) | (conv ? FLAG_CONVERGED : 0));
      if (claimed) {
        red[2 * W + 2 * tphase] = tk;
        red[2 * W + 2 * tphase + 1] = tlen;
      }
    }
    __syncthreads();                                      // slice reuse; ticket visible
    if (!a.queue) {
      hs += stride;
    } else if (++hs >= end) {
      const uint32_t t0 = red[2 * W + 2 * tphase], l0 = red[2 * W + 2 * tphase + 1];
      tphase ^= 1;
      seen = t0 + l0;
      hs = stride + (long long)t0;
      end = hs + l0;
    }
  }
}

// ---------------------------------------------------------------------------
// Layered BP teams with every graph table in global memory (L1/L2-resident):
// the rows in layer order (8 table words each) and their check indices, and
// per adjacency slot of a layer its (variable, degree, CSC start) word. LDS
// then holds only the team's float64 state (LP118_2: 37 KB), so a CU holds
// 4 four-wave teams (the VGPR cap) instead of 3 with the row table alone in
// global memory or 2 with every table in LDS. The table reads are issued a
// phase ahead: this layer's adjacency words while its check nodes run, the
// next layer's row words while this layer's variable nodes run. Same
// arithmetic as bp_team_kernel<true, DC, W>, bit for bit.
// ---------------------------------------------------------------------------
template <int DC, int W>
__global__ void __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(4))) bp_team_lg_kernel(DecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  {
    const uint4* src = (const uint4*)a.blob;                    // LDS part: layer pointers
    uint4* dst = (uint4*)lds;
    const int nvec = a.blob_bytes >> 4;
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) dst[i] = src[i];
  }
  const qldpc_libm_tab* lt = stage_libm(lds, a.off_libm);
  __syncthreads();
  const uint32_t* ltab_g = (const uint32_t*)(a.blob + a.off_cn_tab);      // [Q][8] rows, layer order
  const uint16_t* lrow_g = (const uint16_t*)(a.blob + a.off_lay_rows);    // [Q]    their checks
  const uint32_t* adj_g = (const uint32_t*)(a.blob + a.off_row_ptr);      // [A]    var<<21 | deg<<16 | start
  const uint16_t* lay_ptr = (const uint16_t*)(lds + a.off_lay_ptr);
  const uint16_t* adj_ptr = (const uint16_t*)(lds + a.off_adj_ptr);

  constexpr int TS = 64 * W;        // threads per team
  constexpr int GP = 8 * W;         // 8-lane check groups per pass
  constexpr int NPF = 2;            // CN passes prefetched per layer
  constexpr int NAF = 2;            // VN slots prefetched per thread
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int grp = tid >> 3, k = tid & 7;
  unsigned char* ws = lds + a.blob_bytes;
  double* post = (double*)ws;
  double* c2v = (double*)(ws + a.off_c2v);
  uint32_t* synw = (uint32_t*)(ws + a.off_synw);
  uint32_t* red = (uint32_t*)(ws + a.off_red);
  const int m = a.m, n = a.n, nl = a.n_layers;
  const double L = a.L;

  int rphase = 0;
  auto team_any = [&](bool pred) -> bool {              // one barrier
    const uint64_t b = ballot(pred);
    if (lane == 0) red[rphase * W + wid] = b != 0;
    __syncthreads();
    bool r = false;
#pragma unroll
    for (int w = 0; w < W; ++w) r |= red[rphase * W + w] != 0;
    rphase ^= 1;
    return r;
  };
  uint32_t pt[NPF], pc[NPF];                            // prefetched row words / checks
  auto rows_pf = [&](int l) {
    const int q0 = lay_ptr[l], q1 = lay_ptr[l + 1];
#pragma unroll
    for (int i = 0; i < NPF; ++i) {
      const int q = q0 + GP * i + grp;
      const bool v = q < q1;
      pt[i] = (v && k < DC) ? ltab_g[8 * q + k] : 0u;
      pc[i] = v ? lrow_g[q] : 0u;
    }
  };

  long long hs = blockIdx.x, end = hs + 1;
  const long long stride = gridDim.x;
  uint32_t seen = 0, tlen = 1, tk = 0;
  int tphase = 0;
  while (hs < a.batch) {
    bool claimed = false;
    if (a.queue && hs + 1 == end) {
      const long long rem = a.batch - stride - (long long)seen;
      long long len = rem / (4 * stride);
      len = len < 1 ? 1 : (len > 64 ? 64 : len);
      tlen = (uint32_t)len;
      claimed = true;
      if (tid == 0) tk = atomicAdd(a.queue, tlen);
    }
    int fl = 0;
    int iters = a.max_iter;
    bool conv = false;
    rows_pf(0);
    for (int j = tid; j < n; j += TS) post[j] = L;      // (decoders.py:235-236)
    for (int p = tid; p < a.E; p += TS) c2v[p] = 0.0;
    team_syndrome_bits<2, TS>(a, hs, synw, tid);
    __syncthreads();
    // stop test after every layer by the parity filters (bp_team_kernel)
    uint32_t bl = 0;
    for (int c = lane; c < m; c += 64) bl ^= ((synw[c >> 5] >> (c & 31)) & 1u) ? a.wc[c] : 0u;
    const uint32_t B = wave_xor(bl);
    uint32_t F = (L < 0.0) ? a.filt_all : 0u;
    uint32_t* fsl = red + 2 * W + 4;
    for (int it = 0; it < a.max_iter && !conv; ++it) {
      for (int l = 0; l < nl; ++l) {
        const int q0 = lay_ptr[l], q1 = lay_ptr[l + 1];
        const int v0 = adj_ptr[l], v1 = adj_ptr[l + 1];
        uint32_t pa[NAF];                                 // this layer's adjacency, in flight during the CN
#pragma unroll
        for (int i = 0; i < NAF; ++i) {
          const int q = v0 + TS * i + tid;
          pa[i] = q < v1 ? adj_g[q] : 0u;
        }
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
          if (q0 + GP * i < q1) {
            const bool valid = q0 + GP * i + grp < q1;
            const int c = (int)pc[i];
            // (c = 0 for a pad check: an unmasked in-bounds read)
            const uint32_t sb = (valid ? synw[c >> 5] >> (c & 31) : 0u) & 1u;
            (void)cn_bp_word<DC, QLDPC_BP_SAT>(a, lt, pt[i], valid, k, lane, sb, post, c2v, fl);
          }
        }
        for (int qb = q0 + GP * NPF; qb < q1; qb += GP) {  // layers of more than NPF passes
          const int q = qb + grp;
          const bool valid = q < q1;
          const int c = valid ? (int)lrow_g[q] : 0;
          const uint32_t t = (valid && k < DC) ? ltab_g[8 * q + k] : 0u;
          const uint32_t sb = valid ? (synw[c >> 5] >> (c & 31)) & 1u : 0u;
          (void)cn_bp_word<DC, QLDPC_BP_SAT>(a, lt, t, valid, k, lane, sb, post, c2v, fl);
        }
        rows_pf(l + 1 < nl ? l + 1 : 0);                  // in flight during the VN
        // the team's variable nodes ahead of other teams' check nodes on the
        // SIMD: a layer's VN is short and every wave of the team waits for it
        // at the next barrier
        if constexpr (QLDPC_BP_VNPRIO != 0) __builtin_amdgcn_s_setprio(QLDPC_BP_VNPRIO);
        __syncthreads();
        uint32_t acc = 0;                                 // VN over the layer's adjacent variables
        auto vn = [&](uint32_t info) {
          const int j = (int)(info >> 21), d = (int)((info >> 16) & 31u);
          const double old = post[j];
          const double sc = np_sum_col<true>(c2v + (info & 0xffffu), d);
          const double nw = d == 0 ? L : L + sc;            // (:276-278)
          post[j] = nw;
          if ((old < 0.0) != (nw < 0.0)) acc ^= a.avar[j];
        };
#pragma unroll
        for (int i = 0; i < NAF; ++i)
          if (v0 + TS * i + tid < v1) vn(pa[i]);
        for (int q = v0 + TS * NAF + tid; q < v1; q += TS) vn(adj_g[q]);
        const uint32_t wacc = wave_xor(acc);
        if (lane == 0) fsl[wid] = wacc;
        __syncthreads();
        if constexpr (QLDPC_BP_VNPRIO != 0) __builtin_amdgcn_s_setprio(QLDPC_BP_LHPRIO);
#pragma unroll
        for (int w = 0; w < W; ++w) F ^= fsl[w];
        if (F == B) {                                     // team-uniform
          uint32_t un = 0;
          for (int c = tid; c < m; c += TS) {
            const uint4 t0 = *(const uint4*)(a.rtab + 8 * (size_t)c);
            const uint4 t1 = *(const uint4*)(a.rtab + 8 * (size_t)c + 4);
            const uint32_t rv[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
            uint32_t par = 0;
#pragma unroll
            for (int q = 0; q < DC; ++q) par ^= (uint32_t)(post[rv[q]] < 0.0);
            un |= par ^ ((synw[c >> 5] >> (c & 31)) & 1u);
          }
          if (!team_any(un != 0)) {
            iters = it + 1;
            conv = true;
            break;
          }
        }
      }
    }
    write_outputs_strided<4, TS>(a, hs, tid, [&](int v) { return post[v]; });   // (:280)
    const bool nonfin = team_any((fl & FLAG_NONFINITE) != 0);
    if (tid == 0) {
      a.iters[hs] = iters;
      if (a.flags) a.flags[hs] = (int32_t)((nonfin ? FLAG_NONFINITE : 0) | (conv ? FLAG_CONVERGED : 0));
      if (claimed) {
        red[2 * W + 2 * tphase] = tk;
        red[2 * W + 2 * tphase + 1] = tlen;
      }
    }
    __syncthreads();                                      // slice reuse; ticket visible
    if (!a.queue) {
      hs += stride;
    } else if (++hs >= end) {
      const uint32_t t0 = red[2 * W + 2 * tphase], l0 = red[2 * W + 2 * tphase + 1];
      tphase ^= 1;
      seen = t0 + l0;
      hs = stride + (long long)t0;
      end = hs + l0;
    }
  }
}

}  // namespace qldpc
