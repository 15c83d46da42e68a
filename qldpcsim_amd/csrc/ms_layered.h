// ms_layered.h — ms_layered_kernel (instantiated in decoder_kernels.hip).
#pragma once
#include "decode_generic.h"

namespace qldpc {

// ---------------------------------------------------------------------------
// Check node of the layered kernel with G lanes per check (G = 1, 2, 4, 8):
// lane `sub` of a group owns the EPL = 8 / G consecutive edges sub*EPL ..
// of its check. Layers are short (LP118_2: 30 rows, LP118_0: 16, serial: 1),
// so one lane per check left most of the wave idle while it walked all DC
// edges; with G lanes the per-lane chain is EPL edges long and a wave covers
// 64 / G checks per pass. Per lane: min1/min2 of its |v| by the tournament,
// then merged across the group with DPP lane swaps (quad xor 1, quad xor 2,
// half-row mirror) by (l1,h1)+(l2,h2) -> (min(l1,l2), min(max(l1,l2),
// min(h1,h2))); min / max are exact, so the group ends with the reference's
// two values (decoders.py:160-166) whatever the order. The sign product is
// the XOR of the group's sign words over the same swaps. Missing edges (k >=
// DC) read post[0], count as |v| = inf and write nothing.
// ---------------------------------------------------------------------------

template <int CTRL>
__device__ __forceinline__ void group_merge(double& lo, double& hi, uint32_t& sh) {
  const double olo = dpp_f64<CTRL>(lo), ohi = dpp_f64<CTRL>(hi);
  sh ^= dpp_u32<CTRL>(sh);
  const double nlo = vmin_f64(lo, olo);
  hi = vmin_f64(vmax_f64(lo, olo), vmin_f64(hi, ohi));
  lo = nlo;
}

// Two lanes per check, every lane live (row degree 8: four edges per lane):
// the one-lane-per-check instance's layers of at most 32 rows (round 6).
// Lanes past the layer's last check repeat the trip's first check — the same
// reads, the same values stored — so nothing is masked (as cn_layer's UNI).
__device__ __forceinline__ void cn_ms_pair_uni(const DecodeArgs& a, const uint32_t* trow, int sub, uint32_t synb,
                                               bool first, uint32_t post_b, uint32_t c2v_b, int& fl) {
  const uint4 w = *(const uint4*)(trow + 4 * sub);
  const uint32_t t[4] = {w.x, w.y, w.z, w.w};
  double v[4];
  uint32_t hv[4];
  if (first) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (double)a.L32;            // (:148-149)
  } else {
    // the eight reads in one block, one wait: with the branch inside the edge
    // loop the compiler gave each edge its own block and LDS round trip
    float pf[4], cf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pf[i] = *QLDPC_LDS(const float, post_b + (t[i] & 0xffffu));
      cf[i] = *QLDPC_LDS(const float, c2v_b + (t[i] >> 16));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (a.L + (double)pf[i]) - (double)cf[i];   // (:173, :177)
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) hv[i] = hi_word(v[i]);
  double lo, hi;
  min12_tree<4>(v, lo, hi);
  uint32_t sh = xor_tree<4>(hv);                                  // (:157-159)
  group_merge<kDppQuadXor1>(lo, hi, sh);
  double m1 = lo, m2 = hi;
  if (__builtin_expect(ballot((lo == 0.0) | (hi == __builtin_inf())) != 0, 0)) {
    m1 = __builtin_isinf(lo) ? 0.0 : lo;                          // (:165)
    m2 = __builtin_isinf(hi) ? 0.0 : hi;                          // (:166)
    if (m1 == 0.0) fl |= FLAG_MIN_ZERO;
  }
  const uint32_t npm = ((sh >> 31) ^ synb) << 31;
  const uint32_t c1n = __builtin_bit_cast(uint32_t, (float)(a.beta * m1)) ^ npm;
  const uint32_t c2n = __builtin_bit_cast(uint32_t, (float)(a.beta * m2)) ^ npm;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t c = (__builtin_fabs(v[i]) == lo) ? c2n : c1n;   // (:167-168)
    *QLDPC_LDS(uint32_t, c2v_b + (t[i] >> 16)) = c ^ (hv[i] & 0x80000000u);
  }
}

template <int DC, int G>
__device__ __forceinline__ void cn_ms_split(const DecodeArgs& a, const uint32_t* trow, int sub, bool live,
                                            uint32_t synb, bool first, uint32_t post_b, uint32_t c2v_b,
                                            int& fl) {
  constexpr int EPL = 8 / G;
  uint32_t t[EPL];
  if constexpr (EPL == 8) {
    load_row8(trow, t);
  } else if constexpr (EPL == 4) {
    const uint4 w = *(const uint4*)(trow + 4 * sub);
    t[0] = w.x; t[1] = w.y; t[2] = w.z; t[3] = w.w;
  } else if constexpr (EPL == 2) {
    const uint2 w = *(const uint2*)(trow + 2 * sub);
    t[0] = w.x; t[1] = w.y;
  } else {
    t[0] = trow[sub];
  }
  bool ek[EPL];
#pragma unroll
  for (int i = 0; i < EPL; ++i) ek[i] = live && (DC == 8 || EPL * sub + i < DC);
  double v[EPL];
  uint32_t hv[EPL];
  if (first) {
#pragma unroll
    for (int i = 0; i < EPL; ++i) v[i] = (double)a.L32;          // (:148-149)
  } else {
    // all reads in one block, one wait (as cn_ms_pair_uni)
    float pf[EPL], cf[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
      pf[i] = *QLDPC_LDS(const float, post_b + (t[i] & 0xffffu));
      cf[i] = *QLDPC_LDS(const float, c2v_b + (t[i] >> 16));
    }
    // post_j = L + (f64)S_j rebuilt from the float32 column sum (exact: the
    // value the reference stores, decoders.py:173); v2c = post - c2v (:177)
#pragma unroll
    for (int i = 0; i < EPL; ++i) v[i] = (a.L + (double)pf[i]) - (double)cf[i];
  }
#pragma unroll
  for (int i = 0; i < EPL; ++i) hv[i] = ek[i] ? hi_word(v[i]) : 0u;
  double av[EPL];
#pragma unroll
  for (int i = 0; i < EPL; ++i) av[i] = ek[i] ? v[i] : __builtin_inf();
  double lo, hi;
  min12_tree<EPL>(av, lo, hi);
  uint32_t sh = xor_tree<EPL>(hv);                                // np.sign product (:157-159)
  if constexpr (G >= 2) group_merge<kDppQuadXor1>(lo, hi, sh);
  if constexpr (G >= 4) group_merge<kDppQuadXor2>(lo, hi, sh);
  if constexpr (G >= 8) group_merge<kDppHalfMirror>(lo, hi, sh);
  double m1 = lo, m2 = hi;
  if (__builtin_expect(ballot(live && ((lo == 0.0) | (hi == __builtin_inf()))) != 0, 0)) {
    m1 = __builtin_isinf(lo) ? 0.0 : lo;                          // (:165)
    m2 = __builtin_isinf(hi) ? 0.0 : hi;                          // (:166)
    if (m1 == 0.0 && live) fl |= FLAG_MIN_ZERO;
  }
  const uint32_t npm = ((sh >> 31) ^ synb) << 31;
  const uint32_t c1n = __builtin_bit_cast(uint32_t, (float)(a.beta * m1)) ^ npm;
  const uint32_t c2n = __builtin_bit_cast(uint32_t, (float)(a.beta * m2)) ^ npm;
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    const uint32_t c = (__builtin_fabs(v[i]) == lo) ? c2n : c1n;   // (:167-168)
    if (ek[i]) *QLDPC_LDS(uint32_t, c2v_b + (t[i] >> 16)) = c ^ (hv[i] & 0x80000000u);
  }
}


// ---------------------------------------------------------------------------
// Layered / serial min-sum for uniform-degree codes (decoders.py:153-177 with
// an explicit layer list). Per layer: CN over the layer's rows (Jacobi, the
// fast uniform path), VN over the variables adjacent to the layer, parity
// toggles for flipped hard decisions, stop test. The blob holds the layer
// rows' table words in layer order (ltab) and each adjacency slot's
// (variable, csc start | degree) so every phase is one dependent LDS hop
// shorter than decode_kernel<MS, true, DC>.
// ---------------------------------------------------------------------------

// Variable-node pass of one layer (decoders.py:172-174 over the layer's
// adjacent variables) for a wave-uniform degree bound K: two 64-variable
// chunks per trip with every LDS read of both issued before the sums (the
// chunks' variables are distinct, so their colS writes never alias the other
// chunk's reads). Hard decisions are compared in the float32 domain
// (S < hd_thresh is exactly L + (f64)S < 0). Each flipped hard decision
// contributes its variable's filter word (stop test, ms_layered_kernel); the
// lane-local XOR is returned.
// Variables per lane per pass: layers of more than 128 adjacent variables take
// QLDPC_VN_H (4: LP118_2's 240 / 480 in one / two passes instead of two / four,
// -6.5 % per launch), smaller ones 2 (a 4-wide pass over <= 128 variables
// idles half its lanes: LP118_0 +4 %)
// LO (round 6): every variable of the layer has degree >= LO (host flag, bit
// 7 of the layer's degree byte): the sum is formed as prefix sums over all K
// slots and the degree picks one of the last K - LO + 1 of them, instead of a
// compare and select per slot — the same float32 operations on the first d
// terms, so the same bits (s never is -0.0: it starts as 0 + x0)
// TWO (round 6): every degree is LO or K (bit 8; LP118_2's 3 / 5): one select
// of the two prefix sums (32.42 -> 31.71 ms per LP118_2 p = 0.1 launch,
// profiles/r06/r06h_ab_msl_two_min.json)
// one IEEE float32 add (round to nearest, the same v_add_f32 the compiler
// emits) that the SLP vectorizer cannot pair into v_pk_add_f32: the paired
// prefix sums of two variables needed a register move per pair to line up
// their operands (-0.8 % per LP118_2 p = 0.1 launch,
// profiles/r06/r06aa_ab_vn_asm_add.json)
__device__ __forceinline__ float vadd_f32(float a, float b) {
  float r;
  asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
template <int K, int H, int LO = 1, bool TWO = false>
__device__ __forceinline__ uint32_t vn_layer(const uint32_t* adj_info, const uint32_t* avar, float* colS,
                                             const float* c2v, int v0, int v1, int lane, float thr) {
  uint32_t acc = 0;
  auto trip = [&](int qb, const uint32_t (&info)[H]) {
    bool in[H];
#pragma unroll
    for (int h = 0; h < H; ++h) in[h] = qb + 64 * h + lane < v1;
    float old[H];
    uint32_t av[H];
    float x[H][K];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      old[h] = colS[info[h] >> 21];                         // column sum before this layer
      av[h] = avar[info[h] >> 21];
      const float* c = c2v + (info[h] & 0xffffu);
#pragma unroll
      for (int t = 0; t < K; ++t) x[h][t] = c[t];          // c2v padded by 8 floats
    }
    // every read issued before any sum: left alone, the compiler turned a
    // read whose value only feeds a select into an exec-masked read issued
    // after all the others, behind a wait for everything in flight
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int t = 0; t < K; ++t) asm volatile("" : "+v"(x[h][t]));
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int d = (int)((info[h] >> 16) & 31u);
      float s = 0.0f;                                       // sequential, ascending check (:172)
      if constexpr (LO > 1) {
        float pre = vadd_f32(0.0f, x[h][0]);
#pragma unroll
        for (int t = 1; t < LO; ++t) pre = vadd_f32(pre, x[h][t]);
        s = pre;                                            // d = LO
#pragma unroll
        for (int t = LO; t < K; ++t) {
          pre = vadd_f32(pre, x[h][t]);                     // (slots past d: discarded below)
          if constexpr (!TWO) s = d > t ? pre : s;
        }
        if constexpr (TWO) s = d > LO ? pre : s;            // every degree is LO or K
      } else {
#pragma unroll
        for (int t = 0; t < K; ++t) s += (t < d) ? x[h][t] : 0.0f;
      }
      // every lane stores: a pad lane (past v1) holds variable v1 - 1's word
      // and computes exactly the value that variable's lane stored (same reads — the
      // c2v entries do not change in the VN — same sum), so no exec mask is
      // needed around the store (-4.1 % per LP118_2 p = 0.1 launch,
      // -4.9 % LP118_0, profiles/r04ax/)
      colS[info[h] >> 21] = s;
      const bool flip = in[h] && ((old[h] < thr) != (s < thr));   // hard decision flipped (:173-174)
      acc ^= flip ? av[h] : 0u;
    }
  };
  for (int qb = v0; qb < v1; qb += 64 * H) {
    uint32_t info[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const int q = qb + 64 * h + lane;
      info[h] = adj_info[min(q, v1 - 1)];
    }
    trip(qb, info);
  }
  return acc;
}

// Exact stop test (decoders.py:175-176): every row's parity of the current
// hard decisions against its syndrome bit. Runs only when the filters pass.
template <int DC>
__device__ __forceinline__ bool layered_full_check(const DecodeArgs& a, const float* colS, const uint32_t* synw,
                                                   int lane, float thr) {
  uint32_t un = 0;
  for (int c = lane; c < a.m; c += 64) {
    const uint4 t0 = *(const uint4*)(a.rtab + 8 * (size_t)c);
    const uint4 t1 = *(const uint4*)(a.rtab + 8 * (size_t)c + 4);
    const uint32_t t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    uint32_t par = 0;
#pragma unroll
    for (int k = 0; k < DC; ++k) par ^= (uint32_t)(colS[t[k]] < thr);
    un |= par ^ ((synw[c >> 5] >> (c & 31)) & 1u);
  }
  return ballot(un != 0) == 0;
}

// Check nodes of one layer (rows q0..q1 of the layer-ordered table) with GG
// lanes per check: GG = 1 walks a row's DC edges in one lane (cn_ms_compute),
// GG > 1 splits them over a lane group (cn_ms_split). All rows read the same
// snapshot of the column sums (Jacobi within the layer, decoders.py:155-169).
// SYNL: the syndrome bit by layer position (synl[q]), else by check index
// (lrow[q], then synw) — see the synl build in ms_layered_kernel
template <int DC, int GG, bool UNI = false, bool SYNL = false>
__device__ __forceinline__ void cn_layer(const DecodeArgs& a, const uint32_t* ltab, const uint16_t* lrow,
                                         const uint32_t* synw, const uint32_t* synl, int q0, int q1, int lane,
                                         bool first,
                                         const float* colS, unsigned char* c2v_b, uint32_t post_b,
                                         uint32_t c2v_a, int& fl) {
  if constexpr (GG == 1) {
    // UNI (the one-lane-per-check kernel instance): a wave-uniform loop —
    // lanes past the layer's last check repeat that check (one v_min; the
    // same reads, all issued before any store, so they store exactly its
    // values) instead of sitting out under an exec mask: -0.9 % per LP118_2
    // p = 0.1 launch, but +2.1 % inside the per-layer switch of LP118_0's
    // instance, which keeps the masked loop (profiles/r04ay/)
    for (int qi = UNI ? q0 : q0 + lane; qi < q1; qi += 64) {
      const int q = !UNI ? qi : min(qi + lane, q1 - 1);
      uint32_t t[1][8];
      load_row8(ltab + q * 8, t[0]);
      const int c = SYNL ? q : lrow[q];
      const uint32_t* sw_base = SYNL ? synl : synw;
      // The row words and the check index go out in one LDS round trip, and
      // the syndrome word with the messages: left alone, the compiler waited
      // for the index before issuing the row reads and hoisted the syndrome
      // read above the branch with a wait of its own (-1.4 % per launch on
      // LP118_2 p = 0.1, profiles/r04aq/)
      __builtin_amdgcn_sched_barrier(0);
      const bool live[1] = {true};
      if (first) {
        const uint32_t sb[1] = {(sw_base[c >> 5] >> (c & 31)) & 1u};
        (void)cn_ms_uniform<DC, true, 1>(a, t, sb, live, (const unsigned char*)colS, c2v_b, fl);
      } else {
        CnLoad<DC> Ld;
        uint32_t ca[8];
        float pf[8];
#pragma unroll
        for (int k = 0; k < DC; ++k) {
          ca[k] = c2v_a + (t[0][k] >> 16);
          pf[k] = *QLDPC_LDS(const float, post_b + (t[0][k] & 0xffffu));
          Ld.cv[k] = *QLDPC_LDS(const float, ca[k]);
        }
        // every read issued before any arithmetic (left alone, the scheduler
        // split the 16 reads over three round trips)
        uint32_t sw = sw_base[c >> 5];
#pragma unroll
        for (int k = 0; k < DC; ++k) asm volatile("" : "+v"(pf[k]), "+v"(Ld.cv[k]));
        asm volatile("" : "+v"(sw));
#pragma unroll
        for (int k = 0; k < DC; ++k) Ld.pj[k] = a.L + (double)pf[k];   // (:173)
        (void)cn_ms_compute<DC>(a, Ld, ca, (sw >> (c & 31)) & 1u, 1u, fl);
      }
    }
  } else {
    // 64 / GG checks per pass; every lane takes part in the group swaps, so
    // the loop runs wave-uniformly
    for (int qb = q0; qb < q1; qb += 64 / GG) {
      const int q = qb + lane / GG;
      const bool live = q < q1;
      const int qs = live ? q : q0;
      const int c = SYNL ? qs : lrow[qs];
      const uint32_t sb = ((SYNL ? synl : synw)[c >> 5] >> (c & 31)) & 1u;
      cn_ms_split<DC, GG>(a, ltab + qs * 8, lane & (GG - 1), live, sb, first, post_b, c2v_a, fl);
    }
  }
}

// Stop test without per-check parity state: 32 fixed random parity checks
// w_k of H's rows. If H e = s then w_k H e = w_k s for every k, so the layer
// can only have converged when the 32 filter parities of the hard decisions
// (F, updated by the flipped variables' words a_j = bit k of w_k H) equal those
// of the syndrome (B); then the exact row-by-row test decides. A state with
// H e != s passes all 32 filters with probability 2^-32, so the exact test
// runs about once per decode, and the per-flip parity toggles (LDS atomics,
// one per edge of every flipped variable) are gone.
template <int DC, int G>
__global__ void __launch_bounds__(QLDPC_MAX_THREADS) ms_layered_kernel(DecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  // QLDPC_MSL_GT (the one-lane-per-check instance): the row table [Q][8] and
  // the filter words stay in global memory (L1/L2-resident; the LDS image
  // starts a.lds_skip bytes in, after the row table, and ends before the
  // filter words), so a CU holds 8 waves' state instead of 7 (LP118_2: 39.9
  // -> 36.5 ms per p = 0.1 launch; loading the next layer's row words a layer
  // ahead measured slower, profiles/r05/msl_global_tables_ab.json)
  constexpr int GT = G == 1 ? QLDPC_MSL_GT : 0;
  const int sk = GT ? a.lds_skip : 0;
  {
    const uint4* src = (const uint4*)(a.blob + sk);
    uint4* dst = (uint4*)lds;
    const int nvec = a.blob_bytes >> 4;
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const uint32_t* ltab_l = (const uint32_t*)(lds + a.off_cn_tab);    // [Q][8]
  const uint32_t* ltab_g = (const uint32_t*)(a.blob + a.off_cn_tab); // [Q][8] global (GT)
  const uint32_t* ltab = [&]() {
    if constexpr (GT != 0) return ltab_g;
    else return ltab_l;
  }();
  const uint16_t* lrow = (const uint16_t*)(lds + a.off_lay_rows - sk);    // [Q]
  const uint16_t* lay_ptr = (const uint16_t*)(lds + a.off_lay_ptr - sk);  // [L+1]
  const uint16_t* adj_ptr = (const uint16_t*)(lds + a.off_adj_ptr - sk);  // [L+1]
  const uint32_t* adj_info = (const uint32_t*)(lds + a.off_row_ptr - sk); // [A] var<<21 | deg<<16 | csc start
  const uint16_t* adj_dmax = (const uint16_t*)(lds + a.off_chunk_dmax - sk);// [L] max degree per layer
  const uint32_t* avar = [&]() {                                         // [n] filter word per variable
    if constexpr (GT != 0) return a.avar;
    else return (const uint32_t*)(lds + a.off_vn_chk - sk);
  }();
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  unsigned char* ws = lds + a.blob_bytes + wid * a.wave_bytes;
  // the slice keeps the float32 column sums S (post = L + (f64)S is rebuilt
  // where it is read): 4 n bytes instead of 8 n, so a CU holds more waves
  float* colS = (float*)ws;
  unsigned char* c2v_b = ws + a.off_c2v;
  float* c2v = (float*)c2v_b;
  uint32_t* synw = (uint32_t*)(ws + a.off_synw);
  uint32_t* synl = (uint32_t*)(ws + a.off_parw);                      // syndrome bits by layer position
  const uint32_t post_b = lds_addr(colS), c2v_a = lds_addr(c2v_b);
  const int m = a.m, n = a.n;
  const float thr = a.hd_thresh;

  // Layer bounds in registers (round 6): lane l holds layer l's row range,
  // adjacency range and degree byte, read at each layer head by v_readlane
  // instead of an LDS round trip (-3.5 % per LP118_2 p = 0.1 launch,
  // profiles/r06/r06c_msl_lreg_ab.json); schedules of more than 64 layers
  // (serial ones) keep the LDS reads (a uniform branch the compiler hoists)
  const bool lreg = a.n_layers <= 64;
  uint32_t lq_r = 0, lv_r = 0;
  int ld_r = 0;
  {
    if (lane < a.n_layers) {
      lq_r = (uint32_t)lay_ptr[lane] | ((uint32_t)lay_ptr[lane + 1] << 16);
      lv_r = (uint32_t)adj_ptr[lane] | ((uint32_t)adj_ptr[lane + 1] << 16);
      ld_r = (int)adj_dmax[lane];
    }
  }
  for (HalfShotQueue Q(a.batch, a.queue, waves, wid); Q.hs < a.batch; Q.advance()) {
    const long long hs = Q.hs;
    Q.prefetch(threadIdx.x & 63);
    int fl = 0;
    int iters = a.max_iter;
    bool conv = false;
    const double L = a.L;
    {
      const DecodeArgs& ak = QLDPC_MSL_KARGS ? kargs_fresh() : a;
      load_syndrome_bits<8>(ak, hs, synw, lane);
      // 16-byte stores (both regions are 16-byte aligned and padded to a
      // multiple of 4 floats: colS align16(4 n), c2v E + 8): a quarter of the
      // store instructions of the per-half-shot reset — LP118_2 p = 0.01
      // (1.16 iterations per half-shot) 10.86 -> 10.21 ms per launch, p = 0.05
      // -2.7 % (profiles/r06/r06ag_ab_zero4.json)
      const uint4 z = {0u, 0u, 0u, 0u};
      for (int j = 4 * lane; j < n; j += 256) *(uint4*)(colS + j) = z;   // post = L, c2v = 0 (:148-150)
      for (int p = 4 * lane; p < ak.E; p += 256) *(uint4*)(c2v + p) = z;
    }
    wave_sync();
    if constexpr (G == 0) {
      // the syndrome bits in layer order, once per half-shot (the per-layer
      // lane-group instance): each check node reads its bit by layer
      // position (synl) instead of the check index and then the syndrome
      // word: LP118_0 layered 55.08 -> 54.27 ms per launch; the one-lane
      // instance measured slower with it (LP118_2 p = 0.1 +0.9 %, p = 0.05
      // +2.3 %: the index read hides under the row words' global load, the
      // per-half-shot build does not), profiles/r06/r06y_ab_synl.json
      const int nq = lay_ptr[a.n_layers];
      for (int qb = 0; qb < nq; qb += 64) {
        const int q = qb + lane;
        const int c = q < nq ? lrow[q] : 0;
        const uint64_t bl = ballot(q < nq && ((synw[c >> 5] >> (c & 31)) & 1u));
        if (lane == 0) {
          synl[qb >> 5] = (uint32_t)bl;
          synl[(qb >> 5) + 1] = (uint32_t)(bl >> 32);
        }
      }
    }
    wave_sync();
    // filter parities of the syndrome (B) and of the hard decisions (F: all
    // variables start at post = L, so all ones iff L < 0)
    uint32_t bl = 0;
    uint32_t F;
    {
      const DecodeArgs& ak = QLDPC_MSL_KARGS ? kargs_fresh() : a;
      for (int c = lane; c < m; c += 64) bl ^= ((synw[c >> 5] >> (c & 31)) & 1u) ? ak.wc[c] : 0u;
      F = (L < 0.0) ? ak.filt_all : 0u;
    }
    const uint32_t B = wave_xor(bl);
    bool first = true;
    for (int it = 0; it < a.max_iter && !conv; ++it) {
      for (int l = 0; l < a.n_layers; ++l) {
        uint32_t dq, dv;
        int dsel;
        if (lreg) {
          dq = (uint32_t)__builtin_amdgcn_readlane((int)lq_r, l);
          dv = (uint32_t)__builtin_amdgcn_readlane((int)lv_r, l);
          dsel = __builtin_amdgcn_readlane(ld_r, l);
        } else {
          dq = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)lay_ptr[l] | ((uint32_t)lay_ptr[l + 1] << 16)));
          dv = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)adj_ptr[l] | ((uint32_t)adj_ptr[l + 1] << 16)));
          dsel = __builtin_amdgcn_readfirstlane((int)adj_dmax[l]);
        }
        const int q0 = (int)(dq & 0xffffu), q1 = (int)(dq >> 16);
        if constexpr ((QLDPC_ABLATE_L & 1) != 0) {
        } else if constexpr (G != 0) {
          if constexpr (QLDPC_MSL_PRIO == 1) __builtin_amdgcn_s_setprio(1);
          if constexpr (QLDPC_MSL_PRIO == 2) __builtin_amdgcn_s_setprio(0);
          if (G == 1 && DC == 8 && q1 - q0 <= 32) {
            // a layer of at most 32 rows: two lanes per check (four edges
            // each, one DPP merge) instead of half the wave repeating the
            // first check: 33.40 -> 32.77 ms per LP118_2 p = 0.1 launch
            // (profiles/r06/r06f_ab_g2s.json; the generic split check node
            // instead: 34.25 ms)
            for (int qb = q0; qb < q1; qb += 32) {
              const int q = qb + (lane >> 1);
              const int qs = min(q, q1 - 1);
              const int c = lrow[qs];
              const uint32_t sb = (synw[c >> 5] >> (c & 31)) & 1u;
              cn_ms_pair_uni(a, ltab + qs * 8, lane & 1, sb, first, post_b, c2v_a, fl);
            }
          } else
            cn_layer<DC, G, G == 1>(a, ltab, lrow, synw, synl, q0, q1, lane, first, colS, c2v_b, post_b, c2v_a, fl);
          if constexpr (QLDPC_MSL_PRIO == 1) __builtin_amdgcn_s_setprio(0);
          if constexpr (QLDPC_MSL_PRIO == 2) __builtin_amdgcn_s_setprio(1);
        } else {
          // lanes per check chosen per layer by the host (bits 5-6 of adj_dmax)
          switch ((dsel >> 5) & 3) {
            case 0: cn_layer<DC, 1, false, true>(a, ltab, lrow, synw, synl, q0, q1, lane, first, colS, c2v_b, post_b, c2v_a, fl); break;
            case 1: cn_layer<DC, 2, false, true>(a, ltab, lrow, synw, synl, q0, q1, lane, first, colS, c2v_b, post_b, c2v_a, fl); break;
            case 2: cn_layer<DC, 4, false, true>(a, ltab, lrow, synw, synl, q0, q1, lane, first, colS, c2v_b, post_b, c2v_a, fl); break;
            default: cn_layer<DC, 8, false, true>(a, ltab, lrow, synw, synl, q0, q1, lane, first, colS, c2v_b, post_b, c2v_a, fl); break;
          }
        }
        first = false;
        wave_sync();
        // VN over the layer's adjacent variables (decoders.py:172-174: the
        // other columns are unchanged, so this equals the full recompute)
        const int v0 = (int)(dv & 0xffffu), v1 = (int)(dv >> 16);
        const int dmax = dsel & 31;
        const bool lo3 = (dsel & 0x80) != 0;                // every adjacent variable of degree >= 3
        const bool two = (dsel & 0x100) != 0;               // ... and of degree 3 or dmax
        uint32_t acc = 0;
        switch ((QLDPC_ABLATE_L & 2) ? -1 : dmax) {
          case -1: break;
#define QLDPC_VN_CASE(K)                                                                              \
  case K:                                                                                             \
    if (K >= 5 && two)                                                                                \
      acc = v1 - v0 > 128 ? vn_layer<K, QLDPC_VN_H, 3, K >= 5>(adj_info, avar, colS, c2v, v0, v1, lane, thr) \
                          : vn_layer<K, 2, 3, K >= 5>(adj_info, avar, colS, c2v, v0, v1, lane, thr);  \
    else if (lo3)                                                                                     \
      acc = v1 - v0 > 128 ? vn_layer<K, QLDPC_VN_H, 3>(adj_info, avar, colS, c2v, v0, v1, lane, thr)  \
                          : vn_layer<K, 2, 3>(adj_info, avar, colS, c2v, v0, v1, lane, thr);          \
    else                                                                                              \
      acc = v1 - v0 > 128 ? vn_layer<K, QLDPC_VN_H>(adj_info, avar, colS, c2v, v0, v1, lane, thr)     \
                          : vn_layer<K, 2>(adj_info, avar, colS, c2v, v0, v1, lane, thr);             \
    break;
          QLDPC_VN_CASE(3) QLDPC_VN_CASE(4) QLDPC_VN_CASE(5) QLDPC_VN_CASE(6)
#undef QLDPC_VN_CASE
          default:
            for (int q = v0 + lane; q < v1; q += 64) {
              const uint32_t info = adj_info[q];
              const int j = (int)(info >> 21), d = (int)((info >> 16) & 31u);
              const float old = colS[j];
              const float s = ms_colsum_sw(c2v + (info & 0xffffu), d, dmax);
              colS[j] = s;
              if ((old < thr) != (s < thr)) acc ^= avar[j];       // hard decision flipped
            }
        }
        if constexpr ((QLDPC_ABLATE_L & 4) == 0) F ^= wave_xor(acc);
        wave_sync();
        // stop test (:175-176): filters first, the exact test only if they pass
        if (F == B && layered_full_check<DC>(QLDPC_MSL_KARGS ? kargs_fresh() : a, colS, synw, lane, thr)) {
          iters = it + 1;
          conv = true;
          break;
        }
      }
    }
    // ê, posteriors in original order (post = L + (f64)S, decoders.py:173-174)
    {
      const DecodeArgs& ak = QLDPC_MSL_KARGS ? kargs_fresh() : a;
      write_outputs_batched<4>(ak, hs, lane, [&](int v) { return L + (double)colS[v]; });
      const uint64_t b1 = ballot((fl & FLAG_MIN_ZERO) != 0);
      if (lane == 0) {
        ak.iters[hs] = iters;
        if (ak.flags) ak.flags[hs] = (int32_t)((b1 ? FLAG_MIN_ZERO : 0) | (conv ? FLAG_CONVERGED : 0));
      }
    }
    wave_sync();
  }
}

}  // namespace qldpc
