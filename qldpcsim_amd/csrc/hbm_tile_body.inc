// hbm_tile_body.inc — the body of hbm_tile_kernel (QLDPC_HBM_VPRIOR 0: one
// scalar prior L = a.L) and of hbm_tile_vprior_kernel (QLDPC_HBM_VPRIOR 1: one
// prior per variable, pr.Lv[v] in relabeled variable order, DESIGN.md §3.17),
// included inside each kernel (hbm_kernels.hip) with `a` (HbmArgs), fl_var,
// fl_pos, lazy (the twin: pr, HbmPrior) and the template parameters ALGO, DCMAX, W in scope. Text
// inclusion with the prior spelled as a macro: the scalar kernels see the very
// tokens they were written with (as a __device__ function template, and with
// an `if constexpr` accessor, the same arithmetic compiled to other register
// allocations). Every lane of a wave works on the same variable at the same
// time, so pr.Lv[v] is a wave-uniform table read like the graph tables'; it is
// indexed only with variables taken from them.
#if QLDPC_HBM_VPRIOR
#define QLDPC_HBM_L(v) tb(pr.Lv, v)                  // the prior of relabeled variable v
#define QLDPC_HBM_L32(v) (float)tb(pr.Lv, v)         // msg_v2c = float32(L) of an edge of v (:148-149)
#define QLDPC_HBM_L_UNREAD 0.0                      // (a register default that is overwritten wherever it is read)
#define QLDPC_HBM_F0 pr.filt0                        // XOR of avar[v] over Lv[v] < 0, formed with the prior handle
#else
#define QLDPC_HBM_L(v) L
#define QLDPC_HBM_L32(v) a.L32
#define QLDPC_HBM_L_UNREAD L
#define QLDPC_HBM_F0 (L < 0.0) ? a.filt_all : 0u
#endif
  using Msg = typename std::conditional<ALGO == ALGO_MS, float, double>::type;
  using Post = Msg;                                 // MS: float32 column sum S; BP: float64 posterior
  constexpr int UC = QLDPC_HBM_UC;                   // checks per load step (1: 16 waves per CU; 2: 12, 4: 8 — slower, r03o)
  constexpr int UV = 4, KV = 8;                   // variables per load batch, messages loaded up front
  __shared__ uint32_t xb[3][W * 64];              // per-wave partials: [0] filters / flags, [1] stop test, [2] B
  __shared__ long long shot_s[64];
  const qldpc_libm_tab* lt = nullptr;
  if constexpr (ALGO == ALGO_BP) {
    __shared__ qldpc_libm_tab lt_s;
    const uint4* src = (const uint4*)&qldpc_libm_hbm_dev;
    uint4* dst = (uint4*)&lt_s;
    for (int i = threadIdx.x; i < (int)(sizeof(qldpc_libm_tab) / 16); i += blockDim.x) dst[i] = src[i];
    lt = &lt_s;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = a.m, n = a.n, E = a.E;
#if !QLDPC_HBM_VPRIOR
  const double L = a.L;
#endif
  // this tile's rows: element i of slot `lane` at base[i * 64 + lane] (uniform
  // 64-bit base, 32-bit per-lane offset: one saddr load / store per access)
  const long long g = blockIdx.x;
  Msg* const c2v_t = (Msg*)a.c2v + g * (long long)E * 64;
  Post* const post_t = (Post*)a.post + g * (long long)n * 64;
  uint8_t* const syn_t = a.synT + g * (long long)m * 64;
  auto C2V = [&](int p) -> Msg& { return c2v_t[(uint32_t)p * 64u + (uint32_t)lane]; };
  auto POST = [&](int v) -> Post& { return post_t[(uint32_t)v * 64u + (uint32_t)lane]; };
  auto SYN = [&](int c) -> uint8_t& { return syn_t[(uint32_t)c * 64u + (uint32_t)lane]; };
  auto rd_post = [&](int v) -> double {
    if constexpr (ALGO == ALGO_MS) return QLDPC_HBM_L(v) + (double)POST(v);
    else return POST(v);
  };

  // Check node of a row of more than DCMAX edges (rows of any degree decode,
  // as the reference's load_matrix takes any H): the same arithmetic in two
  // passes over the edges in CSR (ascending variable) order — pass 1 forms
  // min1 / min2 and the sign parity (MS) or np.prod's sequential fold (BP),
  // pass 2 re-forms each edge's v2c (its own c2v is still the old one: each
  // edge is read before it is written) and writes the new message.
  int fl = 0;
  auto cn_wide = [&](int e0, int d, uint32_t sbit, bool first, int l, bool lzf) {
    auto v2c = [&](int k) -> double {                 // post - c2v of edge k (:155-156, :247-248)
      const int e = e0 + k, var = tb(a.row_var, e), pos = tb(a.row_pos, e);
      if (ALGO == ALGO_MS && first && l == 0) return (double)QLDPC_HBM_L32(var);   // msg_v2c = float32(L) (:148-149)
      const bool okv = !lzf || !first || tb(fl_var, var) < l;
      const bool okc = !lzf || !first || tb(fl_pos, pos) < l;
      return (okv ? rd_post(var) : QLDPC_HBM_L(var)) - (double)(okc ? C2V(pos) : (Msg)0);
    };
    if constexpr (ALGO == ALGO_MS) {
      uint32_t par = sbit;
      double min1 = __builtin_inf(), min2 = __builtin_inf();
      for (int k = 0; k < d; ++k) {
        const double v = v2c(k);
        par ^= (uint32_t)(v < 0.0);                   // np.sign, 0 -> +1 (:157-158)
        const double x = __builtin_fabs(v);
        min2 = __builtin_fmin(min2, __builtin_fmax(min1, x));   // min of the rest (:162-164)
        min1 = __builtin_fmin(min1, x);
      }
      const double m1 = __builtin_isinf(min1) ? 0.0 : min1, m2 = __builtin_isinf(min2) ? 0.0 : min2;
      if (m1 == 0.0) fl |= FLAG_MIN_ZERO;
      const float c1 = (float)(a.beta * m1), c2 = (float)(a.beta * m2);   // (:167-168)
      for (int k = 0; k < d; ++k) {
        const double v = v2c(k);
        const float mag = (__builtin_fabs(v) == min1) ? c2 : c1;
        C2V(tb(a.row_pos, e0 + k)) = ((uint32_t)(v < 0.0) ^ par) ? -mag : mag;
      }
    } else {
      double prod = 1.0;
      for (int k = 0; k < d; ++k) prod *= qldpc_tanh_t(v2c(k) / 2.0, lt->tanh_c);   // np.prod (:254)
      for (int k = 0; k < d; ++k) {
        const double th = qldpc_tanh_t(v2c(k) / 2.0, lt->tanh_c);
        if (th == 0.0) fl |= FLAG_NONFINITE;
        double th2 = prod / th;                                        // (:256)
        th2 = (__builtin_fabs(th2) >= 1.0 - a.eps) ? th2 - __builtin_copysign(a.eps, th2) : th2;
        double val = 2.0 * qldpc_atanh_t(th2, lt->atanh_hl, lt->atanh_rcp);   // (:259)
        if (sbit) val = -val;                                          // (:260-261)
        if (!__builtin_isfinite(val)) fl |= FLAG_NONFINITE;
        C2V(tb(a.row_pos, e0 + k)) = val;
      }
    }
  };

  long long shot = -1;
  bool need = true;          // take a half-shot at the next iteration boundary (same on every wave)
  int it = 0, lstop = 0;
  uint32_t F = 0, B = 0;

  for (;;) {
    // --- slots without work take half-shots (one ticket per tile, wave 0) ---
    const uint64_t nm = __ballot(need);
    if (nm) {
      if (wave == 0) {
        const int leader = __builtin_ctzll(nm);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(a.queue, (uint32_t)__builtin_popcountll(nm));
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
        if (need) {
          const long long t = (long long)base +
                              __builtin_amdgcn_mbcnt_hi((uint32_t)(nm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nm, 0));
          shot_s[lane] = t < a.batch ? t : -1;
        }
      }
      __syncthreads();
      const bool init = need;
      if (need) {
        shot = shot_s[lane];
        need = false;
        it = 0;
        fl = 0;
        F = QLDPC_HBM_F0;                           // every posterior starts at its prior
      }
      // stage the new half-shots' syndromes (rows split over the waves) and
      // form their filter word B
      uint32_t bp = 0;
      const bool st = init && shot >= 0;
      if (__ballot(st)) {
        for (int c = wave; c < m; c += W) {
          if (st) {
            uint32_t b;
            if (a.syn_bits) b = (uint32_t)(((const uint64_t*)a.syn)[shot * a.wm + (c >> 6)] >> (c & 63)) & 1u;
            else b = a.syn[shot * (long long)m + c] & 1u;
            SYN(c) = (uint8_t)b;
            bp ^= b ? tb(a.wc, c) : 0u;
          }
        }
        if (!lazy) {                                // rows not a partition: zero the state
          for (int v = wave; v < n; v += W)
            if (st) POST(v) = ALGO == ALGO_MS ? (Post)0 : (Post)QLDPC_HBM_L(v);
          for (int p = wave; p < E; p += W)
            if (st) C2V(p) = (Msg)0;
        }
      }
      const uint32_t bt = wg_combine<W>(xb[2], bp, wave, lane, [](uint32_t x, uint32_t y) { return x ^ y; });
      if (init) B = bt;
      __syncthreads();                              // staged rows visible to every wave
    }
    if (__ballot(shot >= 0) == 0) break;             // queue drained, every slot idle (uniform)

    // --- one iteration over the layers ---
    bool stop = false;                               // this slot's decode ended inside the iteration
    for (int l = 0; l < a.n_layers; ++l) {
      const bool act = shot >= 0 && !stop;
      const bool first = it == 0;
      const bool it0 = __ballot(!first) == 0;        // uniform: no slot past its first iteration
      // check nodes of the layer (Jacobi: all read the same posteriors), UC
      // checks per step with every message load issued before any arithmetic
      const int q0 = tb(a.lay_ptr, l), q1 = tb(a.lay_ptr, l + 1);
      const bool lzf = lazy && __ballot(first && shot >= 0) != 0;   // (uniform) lazy init, a slot in its first iteration
      if (__ballot(act)) {
        for (int qb = q0 + wave * UC; qb < q1; qb += W * UC) {
          int e0[UC], dg[UC];
          uint32_t sb[UC];
          double pj[UC][DCMAX];
          Msg cj[UC][DCMAX];
          const bool l0 = ALGO == ALGO_MS && it0 && l == 0;   // every slot at v2c = float32(L): nothing to read
          // every load of the step is issued before the first wait: indices
          // past the row's degree read edge 0 (discarded), and the per-slot
          // choices (inactive slot, first-iteration "not reached yet") are
          // selects after the loads, not branches around them
          Post rp[UC][DCMAX];
          Msg rc[UC][DCMAX];
#pragma unroll
          for (int u = 0; u < UC; ++u) {
            const int c = qb + u < q1 ? tb(a.lay_rows, qb + u) : 0;
            e0[u] = tb(a.row_ptr, c);
            dg[u] = qb + u < q1 ? tb(a.row_ptr, c + 1) - e0[u] : 0;
            sb[u] = SYN(c);
#pragma unroll
            for (int k0 = 0; k0 < DCMAX; k0 += 8) {
              if (!l0 && (k0 == 0 || k0 < dg[u])) {    // (uniform)
#pragma unroll
                for (int k = k0; k < k0 + 8 && k < DCMAX; ++k) {
                  const int e = k < dg[u] ? e0[u] + k : 0;
                  rp[u][k] = POST(tb(a.row_var, e));
                  rc[u][k] = C2V(tb(a.row_pos, e));
                }
              }
            }
          }
#pragma unroll
          for (int u = 0; u < UC; ++u) {
            sb[u] = dg[u] ? sb[u] : 0u;
#pragma unroll
            for (int k = 0; k < DCMAX; ++k) {
              pj[u][k] = QLDPC_HBM_L_UNREAD;
              cj[u][k] = (Msg)0;
              if (k < dg[u] && !l0) {
                bool okv = true, okc = true;
                if (lzf) {                               // (uniform) first-layer tables
                  okv = !first || tb(fl_var, tb(a.row_var, e0[u] + k)) < l;
                  okc = !first || tb(fl_pos, tb(a.row_pos, e0[u] + k)) < l;
                }
                // (the prior's index is in range: k < the row's degree)
                const double pv = ALGO == ALGO_MS ? QLDPC_HBM_L(tb(a.row_var, e0[u] + k)) + (double)rp[u][k] : (double)rp[u][k];
                pj[u][k] = okv ? pv : QLDPC_HBM_L(tb(a.row_var, e0[u] + k));
                cj[u][k] = okc ? rc[u][k] : (Msg)0;
              }
            }
          }
#pragma unroll
          for (int u = 0; u < UC; ++u) {
            const int d = dg[u];
            if (!act || d == 0) continue;
            if (d > DCMAX) {                            // (uniform) a row wider than the kernel's
              cn_wide(e0[u], d, sb[u], first, l, lzf);  // registers: two passes over its edges
              continue;
            }
            if constexpr (ALGO == ALGO_MS) {
              double av[DCMAX];
              uint64_t negm = 0;
              double min1 = __builtin_inf(), min2 = __builtin_inf();
#pragma unroll
              for (int k = 0; k < DCMAX; ++k) {
                if (k < d) {
                  // v2c = post - c2v (:177); the first layer of the first
                  // iteration reads msg_v2c[H == 1] = L_ch as float32 (:148-149)
                  const double v = (first && l == 0) ? (double)QLDPC_HBM_L32(tb(a.row_var, e0[u] + k)) : pj[u][k] - (double)cj[u][k];
                  negm |= (uint64_t)(v < 0.0) << k;      // np.sign, 0 -> +1 (:157-158)
                  const double x = __builtin_fabs(v);
                  av[k] = x;
                  min2 = __builtin_fmin(min2, __builtin_fmax(min1, x));   // min of the rest (:162-164)
                  min1 = __builtin_fmin(min1, x);
                }
              }
              const double m1 = __builtin_isinf(min1) ? 0.0 : min1;        // (:165)
              const double m2 = __builtin_isinf(min2) ? 0.0 : min2;        // (:166)
              if (m1 == 0.0) fl |= FLAG_MIN_ZERO;                          // App. A.1.6 (flagged, not emulated)
              const uint32_t negprod = (uint32_t)(__builtin_popcountll(negm) & 1) ^ sb[u];
              const float c1 = (float)(a.beta * m1), c2 = (float)(a.beta * m2);   // fl32(beta * min) (:167-168)
#pragma unroll
              for (int k = 0; k < DCMAX; ++k) {
                if (k < d) {
                  const float mag = (av[k] == min1) ? c2 : c1;
                  C2V(tb(a.row_pos, e0[u] + k)) = (((negm >> k) & 1u) ^ negprod) ? -mag : mag;
                }
              }
            } else {
              double th[DCMAX];
              double prod = 1.0;
#pragma unroll
              for (int k = 0; k < DCMAX; ++k) {
                if (k < d) {
                  th[k] = qldpc_tanh_t((pj[u][k] - cj[u][k]) / 2.0, lt->tanh_c);   // v2c (:269), np.tanh (:254)
                  prod *= th[k];                                                  // np.prod: sequential fold
                }
              }
#pragma unroll
              for (int k = 0; k < DCMAX; ++k) {
                if (k < d) {
                  if (th[k] == 0.0) fl |= FLAG_NONFINITE;
                  double th2 = prod / th[k];                            // (:256)
                  th2 = (__builtin_fabs(th2) >= 1.0 - a.eps) ? th2 - __builtin_copysign(a.eps, th2) : th2;  // (:257-258)
                  double val = 2.0 * qldpc_atanh_t(th2, lt->atanh_hl, lt->atanh_rcp);   // (:259)
                  if (sb[u]) val = -val;                                // (:260-261)
                  if (!__builtin_isfinite(val)) fl |= FLAG_NONFINITE;
                  C2V(tb(a.row_pos, e0[u] + k)) = val;
                }
              }
            }
          }
        }
      }
      __syncthreads();                               // every c2v row of the layer written
      // variable nodes adjacent to the layer (others are unchanged, :172-177 /
      // :265-278), UV variables per step, their first KV messages loaded up front
      uint32_t Fp = 0;                               // this wave's flips
      const int v0 = tb(a.adj_ptr, l), v1 = tb(a.adj_ptr, l + 1);
      if (__ballot(act)) {
        for (int qb = v0 + wave * UV; qb < v1; qb += W * UV) {
          int vv[UV], p0[UV], dg[UV];
          [[maybe_unused]] uint32_t wide = 0;           // BP: columns past 128 entries, summed behind this step
          double old[UV];
          Msg cv[UV][KV];
          Post ro[UV];
          Msg rv[UV][KV];
#pragma unroll
          for (int u = 0; u < UV; ++u) {                // loads (past the degree: edge 0, discarded)
            vv[u] = qb + u < v1 ? tb(a.adj_vars, qb + u) : 0;
            p0[u] = tb(a.col_ptr, vv[u]);
            dg[u] = qb + u < v1 ? tb(a.col_ptr, vv[u] + 1) - p0[u] : 0;
            ro[u] = POST(vv[u]);
#pragma unroll
            for (int t = 0; t < KV; ++t) rv[u][t] = C2V(t < dg[u] ? p0[u] + t : 0);
          }
#pragma unroll
          for (int u = 0; u < UV; ++u) {                // per-slot selects
            const bool okv = !lzf || !first || tb(fl_var, vv[u]) < l;
            // (the prior of a slot past the layer's variables: variable 0's, discarded)
            old[u] = dg[u] && okv ? (ALGO == ALGO_MS ? QLDPC_HBM_L(vv[u]) + (double)ro[u] : (double)ro[u]) : QLDPC_HBM_L(vv[u]);
#pragma unroll
            for (int t = 0; t < KV; ++t) {
              const bool ok = !lzf || !first || (t < dg[u] && tb(fl_pos, p0[u] + t) <= l);
              cv[u][t] = t < dg[u] && ok ? rv[u][t] : (Msg)0;
            }
          }
#pragma unroll
          for (int u = 0; u < UV; ++u) {
            const int d = dg[u];
            if (!act || qb + u >= v1) continue;
            auto get = [&](int t) -> Msg {              // message t of the column (zeros past the layer)
              if (t < KV) return cv[u][t];
              const bool ok = !lzf || !first || tb(fl_pos, p0[u] + t) <= l;
              return ok ? C2V(p0[u] + t) : (Msg)0;
            };
            double nw;
            if constexpr (ALGO == ALGO_MS) {
              float S = 0.0f;                              // float32, ascending check (:172)
#pragma unroll
              for (int t = 0; t < KV; ++t)
                if (t < d) S += cv[u][t];
              for (int t = KV; t < d; ++t) S += get(t);
              POST(vv[u]) = S;
              nw = QLDPC_HBM_L(vv[u]) + (double)S;          // (:173)
            } else {
              if (d <= KV) {
                double r = -0.0;                           // np.sum: sequential below 8 terms
                if (d < 8) {
#pragma unroll
                  for (int t = 0; t < KV; ++t)
                    if (t < d) r += cv[u][t];
                } else {                                   // exactly 8: one pairwise block
                  r = ((cv[u][0] + cv[u][1]) + (cv[u][2] + cv[u][3])) + ((cv[u][4] + cv[u][5]) + (cv[u][6] + cv[u][7]));
                }
                nw = d == 0 ? QLDPC_HBM_L(vv[u]) : QLDPC_HBM_L(vv[u]) + (0.0 + r);   // (:269, :276; no edges: L0, :277-278)
              } else {
                if (d > 128) {                             // (uniform) NumPy splits the column: below
                  wide |= 1u << u;
                  continue;
                }
                nw = QLDPC_HBM_L(vv[u]) + np_pairwise_strided(d, get);
              }
              POST(vv[u]) = nw;
            }
            if ((old[u] < 0.0) != (nw < 0.0)) Fp ^= tb(a.avar, vv[u]);   // hard decision flipped
          }
          if constexpr (ALGO == ALGO_BP) {
            // The step's columns of more than 128 entries, one at a time and
            // from memory alone (their posterior is still the old one): a cold
            // path kept out of the unrolled loop above, its pending sums in the
            // launch's dynamic LDS (one slot per level and lane).
            extern __shared__ double wide_stack[];
            static_assert(UV == 4, "the variable's pick below");
#pragma nounroll
            for (int u = 0; u < UV; ++u) {
              const bool mine = (wide >> u) & 1u;          // (a lane without work took no part above)
              if (!__ballot(mine)) continue;
              const int v = u == 0 ? vv[0] : u == 1 ? vv[1] : u == 2 ? vv[2] : vv[3];
              const int c0 = tb(a.col_ptr, v), d = tb(a.col_ptr, v + 1) - c0;
              const bool okv = !lzf || !first || tb(fl_var, v) < l;
              const double was = okv ? (double)POST(v) : QLDPC_HBM_L(v);
              auto get = [&](int t) -> double {            // message t of the column (zeros past the layer)
                const bool ok = !lzf || !first || tb(fl_pos, c0 + t) <= l;
                return ok ? (double)C2V(c0 + t) : 0.0;
              };
              const double nw = QLDPC_HBM_L(v) + np_pairwise_deep(d, get, wide_stack + threadIdx.x, 64 * W);
              if (mine) {
                POST(v) = (Post)nw;
                if ((was < 0.0) != (nw < 0.0)) Fp ^= tb(a.avar, v);
              }
            }
          }
        }
      }
      // filters of every wave's flips; the barrier inside also publishes the
      // layer's posteriors to the stop test / the next layer
      F ^= wg_combine<W>(xb[0], Fp, wave, lane, [](uint32_t x, uint32_t y) { return x ^ y; });
      // stop test after the layer: filters, then the exact check (:174-176)
      const bool cand = act && F == B;
      if (__ballot(cand)) {                          // same on every wave (F, B, act are)
        uint32_t un = 0;
        if (cand) {
          for (int c = wave; c < m && !un; c += W) {
            uint32_t par = SYN(c);
            for (int e = tb(a.row_ptr, c); e < tb(a.row_ptr, c + 1); ++e) {
              const int j = tb(a.row_var, e);
              const bool pv = !first || !lazy || tb(fl_var, j) <= l;
              par ^= (uint32_t)((pv ? rd_post(j) : QLDPC_HBM_L(j)) < 0.0);
            }
            un |= par;
          }
        }
        un = wg_combine<W>(xb[1], un, wave, lane, [](uint32_t x, uint32_t y) { return x | y; });
        if (cand && !un) {
          stop = true;
          lstop = l;
        }
      }
    }
    // --- end of an iteration: finished decodes write their outputs ---
    bool fin = false;
    if (shot >= 0) {
      if (stop) {
        fin = true;
      } else if (it + 1 == a.max_iter) {
        fin = true;
        lstop = a.n_layers - 1;                      // every layer ran
      } else {
        ++it;
      }
    }
    if (__ballot(fin)) {
      __syncthreads();                               // xb[0] readers of the last layer are done
      const int fla = (int)wg_combine<W>(xb[0], (uint32_t)(fl & (FLAG_MIN_ZERO | FLAG_NONFINITE)), wave, lane,
                                         [](uint32_t x, uint32_t y) { return x | y; });
      if (fin && wave == 0) {
        if (stop) {
          if (a.flags) a.flags[shot] = FLAG_CONVERGED | fla;
          a.iters[shot] = it + 1;
        } else {
          if (a.flags) a.flags[shot] = fla;
          a.iters[shot] = a.max_iter;
        }
      }
      const bool lz = lazy != 0;
      for (int j0 = 64 * wave; j0 < n; j0 += 64 * W) {
        uint64_t w = 0;
        for (int jj = 0; jj < 64 && j0 + jj < n; ++jj) {
          if (fin) {
            const int j = j0 + jj, v = tb(a.vinv, j);
            // a variable no layer has reached yet keeps L (never written in
            // this decode: no layer adjacent to it, or a first-iteration stop)
            const bool unwritten = lz && (tb(fl_var, v) >= a.n_layers || (it == 0 && tb(fl_var, v) > lstop));
            const double pv = unwritten ? QLDPC_HBM_L(v) : rd_post(v);
            const bool bit = pv < 0.0;                   // (:174 / :280)
            if (a.eh_bits) w |= (uint64_t)bit << jj;
            else a.ehat[shot * (long long)n + j] = (uint8_t)bit;
            if (a.out_post) a.out_post[shot * (long long)n + j] = pv;
          }
        }
        if (fin && a.eh_bits) ((uint64_t*)a.ehat)[shot * a.wn + (j0 >> 6)] = w;
      }
      if (fin) need = true;
      __syncthreads();                               // xb[0] free again; outputs read before slots are reused
    }
  }
#undef QLDPC_HBM_L
#undef QLDPC_HBM_L32
#undef QLDPC_HBM_L_UNREAD
#undef QLDPC_HBM_F0
