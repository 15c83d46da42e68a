// ms_flood_qc.h — the register-resident body of ms_flood_kernel for lift-16
// quasi-cyclic codes. Included by ms_flood.h inside
// namespace qldpc, after the check-node helpers it shares with the LDS body.
//
// A code whose 16 x 16 blocks are zero or weight-1 circulants (qc_tables.h)
// maps onto the DPP rows of a wave: lane = 16 q + k, row q decodes one
// half-shot, lane k owns position k of every check block and of every
// variable block. Per lane: MB x DC float32 messages (check block b, edge e)
// and, per variable block, the float64 posterior P = L + (double)S as the LDS
// body forms it (S the float32 column sum), formed once in the VN pass; the
// blocks past the first qc_np<T>() in qc_post64's order keep S and form the
// posterior per edge. A message exchange between check block b and variable
// block c is a rotation inside the DPP row by the block's shift s:
//   check position r  <->  variable position (r + s) % 16.
// row_ror:n gives lane i the value of lane (i - n) % 16 of its row, so a check
// reads its variable's P (both words) or S with n = (16 - s) % 16 and a
// variable reads its check's message with n = s. No LDS, no addresses, no
// wave barriers.
//
// The four rows of a wave advance independently: each has its own iteration
// count and stop test (ballot bits 16 q .. 16 q + 15); a row that finishes
// writes its outputs and takes the next half-shot under an exec mask while
// the others go on. Rotations never leave a row, so masked rows are harmless.
// The arithmetic is cn_ms_compute's and vn_sum's, bit for bit; a row starts
// with the messages of iteration 0 (every v2c = float32(L)) written directly,
// as the LDS body's it == 0 branch writes them.

template <typename F, int... I>
__device__ __forceinline__ void static_for_seq(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_seq(f, std::make_integer_sequence<int, N>{});
}

// lane i of a DPP row takes x of lane (i - N) % 16 (row_ror:N)
template <int N>
__device__ __forceinline__ float row_ror_f32(float x) {
  if constexpr ((N & 15) == 0) {
    return x;
  } else {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + (N & 15),
                                                                 0xf, 0xf, true));
  }
}

// the same rotation of a float64: low and high word by the same row_ror
template <int N>
__device__ __forceinline__ double row_ror_f64(double x) {
  if constexpr ((N & 15) == 0) {
    return x;
  } else {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, 0x120 + (N & 15), 0xf, 0xf, true);
    const uint32_t hi =
        (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), 0x120 + (N & 15), 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
  }
}

// Number of variable blocks whose posterior is held in float64 (the rest keep
// the float32 column sum and form the posterior per edge); -DQLDPC_QC_NP=n
// overrides it for A/B. DESIGN.md §3.1.1 for the measured choice.
#ifndef QLDPC_QC_NP
#define QLDPC_QC_NP 34
#endif
template <typename T>
constexpr int qc_np() { return QLDPC_QC_NP < T::NB ? QLDPC_QC_NP : T::NB; }

// Modelled cycles per trip saved by holding block c's posterior in float64
// (float64 instruction 4 cycles, 32-bit one 2): deg conversions and additions
// become one of each, and every non-zero shift rotates two words instead of one.
template <typename T>
constexpr int qc_post64_saving(int c) {
  int zero = 0;
  for (int t = 0; t < T::vdeg[c]; ++t) zero += T::vshift[c][t] == 0;
  return 8 * T::vdeg[c] - 2 * (T::vdeg[c] - zero) - 8;
}
// block c is among the qc_np<T>() blocks of largest saving (ties in table order)
template <typename T>
constexpr bool qc_post64(int c) {
  int rank = 0;
  for (int d = 0; d < T::NB; ++d) {
    const int sd = qc_post64_saving<T>(d), sc = qc_post64_saving<T>(c);
    rank += sd > sc || (sd == sc && d < c);
  }
  return rank < qc_np<T>();
}

// posterior of this lane's variable of block C
template <typename T, int C>
__device__ __forceinline__ double qc_post(double L, const float (&S)[T::NB], const double (&P)[T::NB]) {
  if constexpr (qc_post64<T>(C)) return P[C];
  else return L + (double)S[C];
}

// 16-bit slice of a ballot that belongs to this lane's row (rowsh = lane & 48)
__device__ __forceinline__ uint32_t row_bits(uint64_t b, int rowsh) {
  const uint32_t half = (rowsh & 32) ? (uint32_t)(b >> 32) : (uint32_t)b;
  return (half >> (rowsh & 16)) & 0xffffu;
}

// Work hand-out to the rows of a wave, HalfShotQueue's discipline with rows
// as the consumers: every row starts with one static half-shot (its global
// row index); with a queue, further half-shots come from the ticket counter
// in guided chunks (about remaining / (4 * rows), at most 64, at least 1),
// the next chunk claimed when the last half-shot of the current one is handed
// out, so the atomic's latency hides behind that half-shot's decode.
struct RowQueue {
  long long cur, end, rows, batch;
  uint32_t* q;
  uint32_t tk, tlen, seen;
  __device__ __forceinline__ RowQueue(const DecodeArgs& a, long long rows_, int lane)
      : cur(0), end(0), rows(rows_), batch(a.batch), q(a.queue), tk(0), tlen(1), seen(0) {
    if (q) claim(lane);
  }
  __device__ __forceinline__ void claim(int lane) {
    const long long rem = batch - rows - (long long)seen;
    long long len = rem / (4 * rows);
    len = len < 1 ? 1 : (len > 64 ? 64 : len);
    tlen = (uint32_t)len;
    if (lane == 0) tk = atomicAdd(q, tlen);
  }
  __device__ __forceinline__ long long take(int lane) {   // wave-uniform
    if (cur == end) {
      const uint32_t t = __builtin_amdgcn_readfirstlane(tk);
      seen = t + tlen;
      cur = uniform64(rows + (long long)t);
      end = uniform64(cur + tlen);
    }
    const long long h = cur;
    cur = uniform64(cur + 1);
    if (cur == end) claim(lane);
    return h;
  }
};

// Where check block B's minimum and select are taken (-DQLDPC_QC_CN32=n for
// A/B; DESIGN.md §3.1.1 for the measured choice):
//   0  on the float64 |v|: min12_tree, fl32(beta * min) twice, a float64
//      compare and select per edge (qc_min_select_f64), or QLDPC_QC_LOO's form
//   1  on w_e = bits(fl32(beta * |v_e|)) as unsigned integers: min12_tree_u32,
//      then per edge med3(w_e, w1, w2) ^ (w1 ^ w2), the other one of the two
// Rounding to float32 and multiplying by beta > 0 are monotone, so the smallest
// and second smallest w_e (with multiplicity) are fl32(beta * min1) and
// fl32(beta * min2), and (w_e == w1 ? w2 : w1) has the bits of the float64
// select: where w_e == w1 for an edge that is not the float64 argmin, w2 == w1.
// (A NaN v_e, inf - inf, exists only after a message overflowed float32, outside
// the contract of DESIGN.md §4; the integer order ranks it last, v_min_f64 /
// v_max_f64 skip it, and the two forms may then differ.)
#ifndef QLDPC_QC_CN32
#define QLDPC_QC_CN32 0
#endif

// Where a check block keeps its single bits (-DQLDPC_QC_S31=n for A/B;
// DESIGN.md §3.1.1 for the measured choice):
//   0  at bit 0: the syndrome bit as (synreg >> B) & 1, the sign product and
//      the hard-decision parity shifted down to it, npm shifted back up
//   1  at bit 31, where the float64 high words carry them: the caller passes
//      s31 = synreg << (31 - B) (bit 31 the check's syndrome bit, the bits
//      below it other checks' and not used), npm = (sh ^ s31) & 0x80000000 and
//      the running unsat word takes ph ^ s31; its bit 31 is the stop test's
#ifndef QLDPC_QC_S31
#define QLDPC_QC_S31 1
#endif
// What the wave-uniform rare branch of qc_min_select_f64 redefines
// (-DQLDPC_QC_RARE32=n for A/B):
//   0  the float64 minima m1, m2 that fl32(beta * m) is then formed from, so
//      the fast path copies min1 and min2 into the joined registers
//   1  the two float32 words themselves: they are formed from min1 and min2
//      ahead of the branch and the rare branch forms them again from the
//      substituted minima; no float64 value of the branch is read after it
#ifndef QLDPC_QC_RARE32
#define QLDPC_QC_RARE32 1
#endif

// The float64 minimum and select of one check (decoders.py:160-169), with the
// reference's substitutions for infinite and zero minima and FLAG_MIN_ZERO
template <int DC>
__device__ __forceinline__ void qc_min_select_f64(const DecodeArgs& a, const double (&v)[DC], const uint32_t (&hv)[DC],
                                                  uint32_t npm, float (&cv)[DC], int& fl) {
  double min1, min2;                                      // first min / min of the rest (:160-164)
  min12_tree<DC>(v, min1, min2);
#if QLDPC_QC_RARE32
  // (opaque: otherwise the two roundings are sunk below the branch again and
  // joined on their float64 operands)
  uint32_t c1 = opaque_always(__builtin_bit_cast(uint32_t, (float)(a.beta * min1)));
  uint32_t c2 = opaque_always(__builtin_bit_cast(uint32_t, (float)(a.beta * min2)));
  if (__builtin_expect(ballot((min1 == 0.0) | (min2 == __builtin_inf())) != 0, 0)) {
    const double m1 = __builtin_isinf(min1) ? 0.0 : min1;  // (:165)
    const double m2 = __builtin_isinf(min2) ? 0.0 : min2;  // (:166)
    c1 = __builtin_bit_cast(uint32_t, (float)(a.beta * m1));
    c2 = __builtin_bit_cast(uint32_t, (float)(a.beta * m2));
    if (m1 == 0.0) fl |= FLAG_MIN_ZERO;
  }
  const uint32_t c1n = opaque_always(c1 ^ npm);
  const uint32_t c2n = opaque_always(c2 ^ npm);
#else
  double m1 = min1, m2 = min2;
  if (__builtin_expect(ballot((min1 == 0.0) | (min2 == __builtin_inf())) != 0, 0)) {
    m1 = __builtin_isinf(min1) ? 0.0 : min1;              // (:165)
    m2 = __builtin_isinf(min2) ? 0.0 : min2;              // (:166)
    if (m1 == 0.0) fl |= FLAG_MIN_ZERO;
  }
  const uint32_t c1n = opaque_always(__builtin_bit_cast(uint32_t, (float)(a.beta * m1)) ^ npm);
  const uint32_t c2n = opaque_always(__builtin_bit_cast(uint32_t, (float)(a.beta * m2)) ^ npm);
#endif
  static_for<DC>([&](auto E) __attribute__((always_inline)) {
    constexpr int e = E;
    const uint32_t c = (__builtin_fabs(v[e]) == min1) ? c2n : c1n;
    cv[e] = __builtin_bit_cast(float, c ^ (hv[e] & 0x80000000u));
  });
}

// What a check block's float64 check node computes (-DQLDPC_QC_LOO=n for A/B,
// read with QLDPC_QC_CN32 == 0; DESIGN.md §3.1.1 for the measured choice):
//   0  min1 and min2, fl32(beta * min) of both and per edge a float64 compare
//      and select between them (qc_min_select_f64)
//   1  per edge the minimum over the other edges, loo_e (loo_min_tree), and
//      fl32(beta * loo_e) (qc_loo_f64)
//   2  per edge w_e = bits(fl32(beta * |v_e|)) first, then the leave-one-out
//      minima of the words as unsigned integers (loo_min_tree_u32, qc_loo_u32)
// loo_e is min2 for the argmin and for every edge tied at min1 (then min2 ==
// min1, the reference's "first min / min of the rest") and min1 for the others,
// so fl32(beta * loo_e) has the bits of the select wherever the substitutions of
// decoders.py:165-166 do not apply (min1 != 0, min2 finite). They are tested on
// the tree's two top minima t0, t1: min1 == 0 exactly when one of them is 0, and
// an infinite min2 makes one of them infinite (not the other way round: a wave
// with an infinite t takes the unchanged select form as a whole, which is exact).
// The message's sign npm ^ sign(v_e): npm goes into beta's sign once per check,
// round-to-nearest is symmetric, so fl32((-beta) * x) is fl32(beta * x) with the
// sign bit set, underflow to -0 and overflow to -inf included.
// (A NaN v_e, inf - inf, exists only after a message overflowed float32, outside
// the contract of DESIGN.md §4; v_min_f64 skips it in both forms, but the
// select's v_e == min1 is false for it and the two forms may then differ.)
#ifndef QLDPC_QC_LOO
#define QLDPC_QC_LOO 2
#endif

__device__ __forceinline__ bool zero_or_inf(double x) {   // v_cmp_class_f64: +-0, +-inf
  return __builtin_amdgcn_class(x, 0x264);
}

// The check node of qc_min_select_f64 through the leave-one-out minima
template <int DC>
__device__ __forceinline__ void qc_loo_f64(const DecodeArgs& a, const double (&v)[DC], const uint32_t (&hv)[DC],
                                           uint32_t npm, float (&cv)[DC], int& fl) {
  double loo[DC], t0, t1;
  loo_min_tree<DC>(v, loo, t0, t1);
  if (__builtin_expect(ballot_b(zero_or_inf(t0) | zero_or_inf(t1)) != 0, 0)) {
    qc_min_select_f64<DC>(a, v, hv, npm, cv, fl);
    return;
  }
  // beta with the sign npm (opaque: otherwise the word is formed again per edge)
  const uint64_t bu = __builtin_bit_cast(uint64_t, a.beta);
  const uint32_t bh = opaque_always((uint32_t)(bu >> 32) ^ npm);
  const double bs = __builtin_bit_cast(double, ((uint64_t)bh << 32) | (uint32_t)bu);
  static_for<DC>([&](auto E) __attribute__((always_inline)) {
    constexpr int e = E;
    cv[e] = __builtin_bit_cast(float, and_xor(hv[e], 0x80000000u, __builtin_bit_cast(uint32_t, (float)(bs * loo[e]))));
  });
}

// Whether qc_loo_u32's sign tree takes the syndrome word as a ninth input
// (-DQLDPC_QC_SYNFOLD=n for A/B, read with QLDPC_QC_LOO == 2 and QLDPC_QC_S31;
// DESIGN.md §3.1.1 for the measured choice):
//   0  npm = (xor of the eight high words ^ s31) & 0x80000000, beta's high word ^ npm
//   1  sn = xor of the eight high words and s31 (four xor3), beta's signed high
//      word as one and_xor(sn, 0x80000000, beta's high word); npm itself is
//      formed only where the fallback reads it
#ifndef QLDPC_QC_SYNFOLD
#define QLDPC_QC_SYNFOLD 0
#endif

__device__ __forceinline__ bool zero_or_inf(float x) {    // v_cmp_class_f32: +-0, +-inf
  return __builtin_amdgcn_classf(x, 0x264);
}

// The leave-one-out check node on w_e = bits(fl32(bs * |v_e|)), bs = beta with
// the sign npm: the roundings go in front of the tree, which then runs on 32-bit
// words (loo_min_tree_u32). x -> fl32(bs * x) is monotone in magnitude on x >= 0
// and all words of a lane carry npm's sign bit (on +-0 and +-inf too), so the
// unsigned order of the words is the order of the |v_e| for either sign and the
// minimum over e' != e of w_e' is bits(fl32(bs * loo_e)), the word qc_loo_f64
// forms. The rare test is a float32 class test on the tree's mA, mB and oA
// (top0, top1, out0): min1 == 0 makes min(mA, oA), the minimum of all, zero; an
// infinite min2 leaves at most one finite value, so mA or mB is infinite. A
// product that underflows to zero or overflows float32 there fires it as well.
// A wave that it fires on takes the unchanged select form on the v[] still held.
// (SN, QLDPC_QC_SYNFOLD: npm is given as a word whose bit 31 is npm's, the bits
// below it not used)
template <int DC, bool SN = false>
__device__ __forceinline__ void qc_loo_u32(const DecodeArgs& a, const double (&v)[DC], const uint32_t (&hv)[DC],
                                           uint32_t npm, float (&cv)[DC], int& fl) {
  // beta with the sign npm (opaque: otherwise the word is formed again per edge)
  const uint64_t bu = __builtin_bit_cast(uint64_t, a.beta);
  const uint32_t bh = opaque_always(SN ? and_xor(npm, 0x80000000u, (uint32_t)(bu >> 32)) : (uint32_t)(bu >> 32) ^ npm);
  const double bs = __builtin_bit_cast(double, ((uint64_t)bh << 32) | (uint32_t)bu);
  uint32_t w[DC], loo[DC], mA, mB, oA;
  static_for<DC>([&](auto E) __attribute__((always_inline)) {
    constexpr int e = E;
    w[e] = __builtin_bit_cast(uint32_t, (float)(bs * __builtin_fabs(v[e])));
  });
  loo_min_tree_u32<DC>(w, loo, mA, mB, oA);
  const bool rare = zero_or_inf(__builtin_bit_cast(float, mA)) | zero_or_inf(__builtin_bit_cast(float, mB)) |
                    zero_or_inf(__builtin_bit_cast(float, oA));
  if (__builtin_expect(ballot_b(rare) != 0, 0)) {
    qc_min_select_f64<DC>(a, v, hv, SN ? npm & 0x80000000u : npm, cv, fl);
    return;
  }
  static_for<DC>([&](auto E) __attribute__((always_inline)) {
    constexpr int e = E;
    cv[e] = __builtin_bit_cast(float, and_xor(hv[e], 0x80000000u, loo[e]));
  });
}

// posterior of the variable behind edge E of check block B, rotated to the
// check's lane
template <typename T, int B, int E>
__device__ __forceinline__ double qc_edge_post(double L, const float (&S)[T::NB], const double (&P)[T::NB]) {
  constexpr int c = T::cvar[B][E], s = T::cshift[B][E];
  if constexpr (qc_post64<T>(c)) return row_ror_f64<(16 - s) & 15>(P[c]);
  else return L + (double)row_ror_f32<(16 - s) & 15>(S[c]);
}

// Min-sum update of check block B (decoders.py:155-169 for the lane's check):
// cn_ms_compute with the posteriors rotated in from P (or formed from the
// rotated S) and the messages in registers. Returns the check's "unsatisfied"
// bit for the posteriors it read, or (QLDPC_QC_S31) ORs a word with that bit
// at bit 31 into unsat_acc; synb is then s31.
template <typename T, int B>
__device__ __forceinline__ uint32_t qc_check(const DecodeArgs& a, double L, float (&S)[T::NB], double (&P)[T::NB],
                                             float (&c2v)[T::MB][T::DC], uint32_t synb, int& fl,
                                             uint32_t& unsat_acc) {
  constexpr int DC = T::DC;
  // one check block's working set at a time: the inputs are pinned behind the
  // previous block's outputs (volatile asm statements keep their order), so no
  // widened copy of a later block's operands is formed ahead of its turn
  static_for<DC>([&](auto E) __attribute__((always_inline)) {
    float& cx = c2v[B][E];                              // (named: asm operands alone do not capture)
    if constexpr (qc_post64<T>(T::cvar[B][E])) {
      double& px = P[T::cvar[B][E]];
      asm volatile("" : "+v"(px), "+v"(cx));
    } else {
      float& sx = S[T::cvar[B][E]];
      asm volatile("" : "+v"(sx), "+v"(cx));
    }
  });
  double v[DC];
  uint32_t hv[DC], hp[DC];
  static_for<DC>([&](auto E) __attribute__((always_inline)) {
    const double post = qc_edge_post<T, B, E>(L, S, P);
    v[E] = post - (double)c2v[B][E];                      // v2c = post - c2v (:177)
    hv[E] = hi_word(v[E]);
    hp[E] = hi_word(post);
  });
  const uint32_t ph = xor_tree<DC>(hp);                   // hard-decision parity (:174)
#if QLDPC_QC_S31 && QLDPC_QC_SYNFOLD && QLDPC_QC_LOO == 2 && !QLDPC_QC_CN32
  uint32_t hs[DC + 1];
  static_for<DC>([&](auto E) __attribute__((always_inline)) { hs[E] = hv[E]; });
  hs[DC] = synb;
  const uint32_t npm = xor_tree<DC + 1>(hs);              // bit 31: np.sign product ^ syndrome bit
#elif QLDPC_QC_S31
  const uint32_t sh = xor_tree<DC>(hv);                   // np.sign product (:157-159)
  const uint32_t npm = (sh ^ synb) & 0x80000000u;
#else
  const uint32_t sh = xor_tree<DC>(hv);                   // np.sign product (:157-159)
  const uint32_t npm = ((sh >> 31) ^ synb) << 31;
#endif
#if QLDPC_QC_CN32
  uint32_t w[DC];
  static_for<DC>([&](auto E) __attribute__((always_inline)) {
    w[E] = __builtin_bit_cast(uint32_t, (float)(a.beta * __builtin_fabs(v[E])));
  });
  uint32_t w1, w2;                                        // bits of fl32(beta * min1), fl32(beta * min2)
  min12_tree_u32<DC>(w, w1, w2);
  w1 = opaque_always(w1), w2 = opaque_always(w2);
  // the reference's rules for zero and infinite minima (:165-166) and the
  // flag are defined on the float64 minima: a wave with a zero or a
  // non-finite float32 minimum takes the float64 check node as a whole
  if (__builtin_expect(ballot((w1 == 0u) | (w2 >= 0x7f800000u)) != 0, 0)) {
    qc_min_select_f64<DC>(a, v, hv, npm, c2v[B], fl);
  } else {
    // the median is w1 where w_e == w1 and w2 elsewhere: ^ (w1 ^ w2) gives the other one
    const uint32_t w12n = xor3(w1, w2, npm);
    static_for<DC>([&](auto E) __attribute__((always_inline)) {
      c2v[B][E] = __builtin_bit_cast(float, umed3(w[E], w1, w2) ^ and_xor(hv[E], 0x80000000u, w12n));
    });
  }
#elif QLDPC_QC_LOO == 2
  qc_loo_u32<DC, QLDPC_QC_S31 && QLDPC_QC_SYNFOLD>(a, v, hv, npm, c2v[B], fl);
#elif QLDPC_QC_LOO
  qc_loo_f64<DC>(a, v, hv, npm, c2v[B], fl);
#else
  qc_min_select_f64<DC>(a, v, hv, npm, c2v[B], fl);
#endif
#if QLDPC_QC_S31
  unsat_acc |= ph ^ synb;
  static_for<DC>([&](auto E) __attribute__((always_inline)) {
    float& cx = c2v[B][E];
    asm volatile("" : "+v"(cx));
  });
  asm volatile("" : "+v"(unsat_acc));
  return 0;
#else
  uint32_t unsat = (ph >> 31) ^ synb;
  static_for<DC>([&](auto E) __attribute__((always_inline)) {
    float& cx = c2v[B][E];
    asm volatile("" : "+v"(cx));
  });
  asm volatile("" : "+v"(unsat));
  return unsat;
#endif
}

// lane i of a DPP row takes x of lane (i - N) % 16 (row_ror:N)
template <int N>
__device__ __forceinline__ uint32_t row_ror_u32(uint32_t x) {
  if constexpr ((N & 15) == 0) {
    return x;
  } else {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x120 + (N & 15), 0xf, 0xf, true);
  }
}

// parity of check block B's hard decisions XOR its syndrome bit (the stop
// test after the last iteration, decoders.py:174-176); hw: this lane's hard
// decisions, bit c & 31 of word c >> 5 for variable block c. With QLDPC_QC_S31
// synb is s31 and the result's bit 31 is the parity (the bits below are not).
template <typename T, int B>
__device__ __forceinline__ uint32_t qc_parity(const uint32_t (&hw)[(T::NB + 31) / 32], uint32_t synb) {
  uint32_t ph = synb;
  static_for<T::DC>([&](auto E) __attribute__((always_inline)) {
    constexpr int e = E, c = T::cvar[B][e], s = T::cshift[B][e];
#if QLDPC_QC_S31
    ph ^= row_ror_u32<(16 - s) & 15>(hw[c >> 5]) << (31 - (c & 31));
#else
    ph ^= row_ror_u32<(16 - s) & 15>(hw[c >> 5]) >> (c & 31);
#endif
  });
#if !QLDPC_QC_S31
  ph &= 1u;
#endif
  asm volatile("" : "+v"(ph));                            // one check block at a time
  return ph;
}

// S_c = sum of variable block C's messages in ascending check order, float32,
// starting from the first term (vn_sum)
template <typename T, int C>
__device__ __forceinline__ float qc_colsum(const float (&c2v)[T::MB][T::DC]) {
  float s = row_ror_f32<T::vshift[C][0]>(c2v[T::vchk[C][0]][T::vslot[C][0]]);
  static_for<T::vdeg[C] - 1>([&](auto I) __attribute__((always_inline)) {
    constexpr int t = I + 1;
    s = s + row_ror_f32<T::vshift[C][t]>(c2v[T::vchk[C][t]][T::vslot[C][t]]);
  });
  return s;
}

template <typename T>
__device__ __forceinline__ void flood_qc_body(const DecodeArgs& a) {
  constexpr int MB = T::MB, NB = T::NB, DC = T::DC;
  static_assert(qc::kLift == 16, "one DPP row per half-shot");
  const int lane = threadIdx.x & 63;
  const int q = lane >> 4, rowsh = lane & 48;
  const int waves = blockDim.x >> 6;
  const long long rows = 4ll * gridDim.x * waves;
  const long long batch = a.batch;
  constexpr int n = 16 * NB, m = 16 * MB;
  constexpr int wn = (n + 63) / 64;

  float c2v[MB][DC], S[NB];
  double P[NB];                          // S[c] or P[c] per block (qc_post64): constant indices only
  int it = 0, fl = 0;
  uint32_t synreg = 0;
  long long hs = 4ll * ((long long)blockIdx.x * waves + (threadIdx.x >> 6)) + q;
  RowQueue Q(a, rows, lane);
  // One trip: finished rows write their outputs, take their next half-shot and
  // start it (the messages of iteration 0); then every live row's VN pass; then
  // the CN pass with the stop test. A row that reaches max_iter in its VN pass
  // sits out that trip's CN pass; either way a finished row joins the next VN
  // pass with its new half-shot, so a half-shot of i iterations costs i trips.
  bool live = false, fin = true;         // fin: rows to (re)start; at first all, on their static half-shot
  bool conv = false;
  int iters = 0;
  bool started = false;                  // wave-uniform

  for (;;) {
    const uint64_t finb = ballot_b(fin);
    if (finb != 0) {
      if (started) {
        if (fin) {
          // outputs in original variable order: column 16 c + k is this lane's block c.
          // Arguments and lane offsets used only here are formed here: read afresh
          // (kargs_fresh) and behind an opaque lane, they hold no registers in the loop
          const DecodeArgs& f = kargs_fresh();
          int ln = threadIdx.x;
          asm volatile("" : "+v"(ln));
          const int kl = ln & 15, rsh = ln & 48;
          // (a float32 block's posterior formed where it is used)
          if (f.eh_bits) {
            // word w of this row: blocks 4 w .. 4 w + 3, 16 ballot bits each; lane k = w stores it
            uint32_t lo = 0, hi = 0;
            static_for<wn>([&](auto W) __attribute__((always_inline)) {
              uint32_t r[4] = {0, 0, 0, 0};
              static_for<4>([&](auto I) __attribute__((always_inline)) {
                constexpr int c = 4 * W + I;
                if constexpr (c < NB) r[I] = row_bits(ballot_b(qc_post<T, c>(a.L, S, P) < 0.0), rsh);
              });
              if (kl == W) lo = r[0] | (r[1] << 16), hi = r[2] | (r[3] << 16);
            });
            if (kl < wn) ((uint64_t*)f.ehat)[hs * wn + kl] = ((uint64_t)hi << 32) | lo;
          } else {
            uint8_t* eo = f.ehat + hs * (long long)n + kl;
            static_for<NB>([&](auto C) __attribute__((always_inline)) {
              eo[16 * C] = (uint8_t)(qc_post<T, C>(a.L, S, P) < 0.0);
            });
          }
          if (f.post) {
            double* po = f.post + hs * (long long)n + kl;
            static_for<NB>([&](auto C) __attribute__((always_inline)) { po[16 * C] = qc_post<T, C>(a.L, S, P); });
          }
          const bool mz = row_bits(ballot_b((fl & FLAG_MIN_ZERO) != 0), rsh) != 0;
          if (kl == 0) {
            f.iters[hs] = iters;
            if (f.flags) f.flags[hs] = (int32_t)((mz ? FLAG_MIN_ZERO : 0) | (conv ? FLAG_CONVERGED : 0));
          }
        }
        // the finished rows' next half-shots
        if (Q.q) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if ((finb >> (16 * r)) & 1u) {
              const long long h = Q.take(lane);
              if (q == r) hs = h;
            }
          }
        } else if (fin) {
          hs += rows;
        }
      }
      started = true;
      if (fin) {
        // start this row on half-shot hs with the messages of iteration 0:
        // every v2c = float32(L) (decoders.py:148-149), one value per check
        live = hs < batch;
        it = 0, synreg = 0;
        if (live) {
          const DecodeArgs& f = kargs_fresh();
          int ln = threadIdx.x;
          asm volatile("" : "+v"(ln));
          const int kl = ln & 15;
          if (f.syn_bits) {              // 64-bit words: check 16 b + k is bit 16 (b & 1) + k of half-word b >> 1
            const uint32_t* row = (const uint32_t*)((const uint64_t*)f.syn + hs * f.wm);
            uint32_t w[(MB + 1) / 2];
#pragma unroll
            for (int i = 0; i < (MB + 1) / 2; ++i) w[i] = row[i];
#pragma unroll
            for (int b = 0; b < MB; ++b) synreg |= ((w[b >> 1] >> (16 * (b & 1) + kl)) & 1u) << b;
          } else {
            const uint8_t* row = f.syn + hs * (long long)m + kl;
            uint32_t w[MB];
#pragma unroll
            for (int b = 0; b < MB; ++b) w[b] = row[16 * b];
#pragma unroll
            for (int b = 0; b < MB; ++b) synreg |= (w[b] & 1u) << b;
          }
        }
        // (L32 and beta read afresh: their products hold no registers in the loop)
        const DecodeArgs& g = kargs_fresh();
        const double vf = (double)g.L32;
        const double av = __builtin_fabs(vf);
        const uint32_t cb = __builtin_bit_cast(uint32_t, (float)(g.beta * av));
        const uint32_t neg = (uint32_t)(vf < 0.0);
        fl = av == 0.0 ? FLAG_MIN_ZERO : 0;
        static_for<MB>([&](auto B) __attribute__((always_inline)) {
          const uint32_t negprod = ((neg * DC) ^ (synreg >> B)) & 1u;
          const float val = __builtin_bit_cast(float, cb | ((neg ^ negprod) << 31));
          static_for<DC>([&](auto E) __attribute__((always_inline)) { c2v[B][E] = val; });
        });
        fin = false;
      }
    }
    if (ballot_b(live) == 0) break;

    if (live) {
      static_for<NB>([&](auto C) __attribute__((always_inline)) {
        if constexpr (qc_post64<T>(C)) {
          double& pc = P[C];
          pc = a.L + (double)qc_colsum<T, C>(c2v);
          asm volatile("" : "+v"(pc));                    // one variable block at a time
        } else {
          float& sc = S[C];
          sc = qc_colsum<T, C>(c2v);
          asm volatile("" : "+v"(sc));
        }
      });
      it += 1;
      if (it == a.max_iter) {
        uint32_t hw[(NB + 31) / 32] = {};
        static_for<NB>([&](auto C) __attribute__((always_inline)) {
          hw[C / 32] |= (hi_word(qc_post<T, C>(a.L, S, P)) >> 31) << (C % 32);
        });
        uint32_t un = 0;
#if QLDPC_QC_S31
        static_for<MB>([&](auto B) __attribute__((always_inline)) {
          un |= qc_parity<T, B>(hw, synreg << (31 - B));
        });
        fin = true, iters = it;
        conv = row_bits(ballot_b((int32_t)un < 0), rowsh) == 0;
#else
        static_for<MB>([&](auto B) __attribute__((always_inline)) {
          un |= qc_parity<T, B>(hw, (synreg >> B) & 1u);
        });
        fin = true, iters = it;
        conv = row_bits(ballot_b(un != 0), rowsh) == 0;
#endif
      }
    }
    if (live && !fin) {
      uint32_t unsat = 0;
      // stop test of iteration it - 1 (decoders.py:175-176)
#if QLDPC_QC_S31
      static_for<MB>([&](auto B) __attribute__((always_inline)) {
        qc_check<T, B>(a, a.L, S, P, c2v, synreg << (31 - B), fl, unsat);
      });
      if (row_bits(ballot_b((int32_t)unsat < 0), rowsh) == 0) fin = true, conv = true, iters = it;
#else
      static_for<MB>([&](auto B) __attribute__((always_inline)) {
        unsat |= qc_check<T, B>(a, a.L, S, P, c2v, (synreg >> B) & 1u, fl, unsat);
      });
      if (row_bits(ballot_b(unsat != 0), rowsh) == 0) fin = true, conv = true, iters = it;
#endif
    }
  }
}
