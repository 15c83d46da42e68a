// relay_kernel_body.inc — the body of relay_ms_kernel (relay_kernels.hip,
// DESIGN.md §3.11: one scalar prior L = a.L) and of relay_vprior_kernel
// (relay_vprior_kernels.hip, §3.18), included inside each kernel with `ra`
// (RelayArgs), the template parameter DC and, in scope,
//   constexpr bool VP    variable j's prior is the row entry L_j, staged into
//                        LDS behind the graph image as decode_vprior_kernel's
//   wgt, cost            (VP) [n] int64 weights, relabeled order, global; cost
//                        1: a solution weighs the sum of wgt over its set
//                        bits, 0: their count. Unread without VP.
// Without VP every VP branch folds away and the kernel is the one it has
// always been.
//
// Per pass t of leg r (gamma = gamma[r]):
//   Lam_j = fl((1 - gamma_j) L_j) + fl(gamma_j M_j)     two products, one add
//   checks read X_j - c2v_e, X_j = Lam_j + (f64)S_j     (t = 0: X_j = (f64)(f32)Lam_j, c2v = S = 0)
//   S_j   = float32 column sum, M_j = Lam_j + (f64)S_j
//   stop test: H (M < 0) == s
// The slice holds two float64 rows: M, and X for the next check pass, which
// the variable pass forms from the Lam of the M it has just written.
  const DecodeArgs& a = ra.d;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  // Stage the read-only graph blob into LDS (16-byte vector copies).
  {
    const uint4* src = (const uint4*)a.blob;
    uint4* dst = (uint4*)lds;
    const int nvec = a.blob_bytes >> 4;
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) dst[i] = src[i];
  }
  if constexpr (VP) {
    // the code's prior row (relabeled order) behind the graph image: staged
    // once, shared by every wave of the workgroup
    double* dst = (double*)(lds + a.blob_bytes);
    for (int j = threadIdx.x; j < a.n; j += blockDim.x) dst[j] = a.vprior[j];
  }
  __syncthreads();

  LdsView g{};
  g.cn_tab = (const uint32_t*)(lds + a.off_cn_tab);
  g.row_ptr = (const uint16_t*)(lds + a.off_row_ptr);
  g.vn_info = (const uint32_t*)(lds + a.off_vn_ptr);
  g.chunk_dmax = (const uint8_t*)(lds + a.off_chunk_dmax);

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  const double* Lrow = (const double*)(lds + a.blob_bytes);   // (VP)
  unsigned char* ws = lds + a.blob_bytes + (VP ? a.vprior_bytes : 0) + wid * a.wave_bytes;
  double* X = (double*)ws;
  float* c2v = (float*)(ws + a.off_c2v);
  uint32_t* synw = (uint32_t*)(ws + a.off_synw);
  double* M = (double*)(ws + ra.off_m);
  uint32_t* ew = (uint32_t*)(ws + ra.off_ew);
  uint32_t* bw = (uint32_t*)(ws + ra.off_best);

  const int m = a.m, n = a.n;
  const int ewords = 2 * a.wn;
  const double L = a.L;
  // a solution's weight: a count (int) or, with VP, possibly a sum of wgt (int64)
  using Weight = std::conditional_t<VP, long long, int>;
  constexpr Weight kHeaviest = VP ? (Weight)0x7fffffffffffffffLL : (Weight)0x7fffffff;

  for (HalfShotQueue Q(a.batch, a.queue, waves, wid); Q.hs < a.batch; Q.advance()) {
    const long long hs = Q.hs;
    Q.prefetch(lane);
    int fl = 0;
    int iters = 0, found = 0, best_leg = -1;
    Weight best_w = kHeaviest;

    // M = L ("previous posterior" of leg 0); the syndrome as bit words
    for (int j = lane; j < n; j += 64) M[j] = VP ? Lrow[j] : L;
    for (int c0 = 0; c0 < m; c0 += 64) {
      const int c = c0 + lane;
      store_bits64(synw, c0, c < m ? (int)syn_bit(a, hs, c) : 0, lane);
    }
    wave_sync();

    for (int r = 0; r < ra.legs; ++r) {
      const double* gam = ra.gamma + (long long)r * n;
      const int T = ld_const(ra.leg_iters, r);
      // leg start: c2v = 0 and X = (f64)(f32)Lam, so that the first check pass
      // reads float32(Lam_j) through the same code as every later one
      // (x - 0 = x; + 0.0 turns a float32 underflow to -0 into +0: sign(0) = +1)
      for (int j = lane; j < n; j += 64)
        X[j] = (double)(float)relay_blend(ld_const(gam, j), VP ? Lrow[j] : L, M[j]) + 0.0;
      for (int p = lane; p < a.E; p += 64) c2v[p] = 0.0f;
      wave_sync();

      bool ok = false;
      int wt = 0;
      for (int t = 0; t < T; ++t) {
        // check nodes, Jacobi over every check (the parity they return is of
        // X, not of the posteriors M: unused)
        for (int c = lane; c < m; c += 64) {
          const uint32_t sb = (synw[c >> 5] >> (c & 31)) & 1u;
          if constexpr (DC > 0) {
            uint32_t tw[1][8];
            load_row8(g.cn_tab + c * 8, tw[0]);
            const uint32_t sbs[1] = {sb};
            const bool live[1] = {true};
            (void)cn_ms_uniform<DC, false, 1>(a, tw, sbs, live, (const unsigned char*)X, (unsigned char*)c2v, fl);
          } else {
            (void)cn_update<ALGO_MS, 0>(a, g, c, sb, false, X, c2v, fl);
          }
        }
        wave_sync();
        // variable nodes: S, M = Lam + S, and next pass's X = Lam(M) + S;
        // hard decisions as ballot words, their weight on the way
        wt = 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
          const int dmax = __builtin_amdgcn_readfirstlane((int)g.chunk_dmax[j0 >> 6]);
          const int j = j0 + lane;
          bool neg = false;
          if (j < n) {
            const uint32_t info = g.vn_info[j];
            const float s = ms_colsum_sw(c2v + (info & 0xffffu), (int)(info >> 16), dmax);
            const double gj = ld_const(gam, j);
            const double Lj = VP ? Lrow[j] : L;               // (VP: read once, both blends)
            const double Mn = relay_blend(gj, Lj, M[j]) + (double)s;
            M[j] = Mn;
            X[j] = relay_blend(gj, Lj, Mn) + (double)s;
            neg = Mn < 0.0;
          }
          const uint64_t b = ballot_b(neg);
          wt += __popcll(b);
          if (lane == 0) ew[j0 >> 5] = (uint32_t)b;
          if (lane == 1) ew[(j0 >> 5) + 1] = (uint32_t)(b >> 32);
        }
        ++iters;
        wave_sync();
        // stop test on M's sign bits: row parities against the syndrome
        uint32_t un = 0;
        for (int c = lane; c < m; c += 64) {
          uint32_t par = (synw[c >> 5] >> (c & 31)) & 1u;
          if constexpr (DC > 0) {
            uint32_t tw[8];
            load_row8(g.cn_tab + c * 8, tw);
#pragma unroll
            for (int k = 0; k < DC; ++k) {
              const int j = tab_var<DC>(tw[k]);
              par ^= ew[j >> 5] >> (j & 31);
            }
          } else {
            for (int e = g.row_ptr[c], e1 = g.row_ptr[c + 1]; e < e1; ++e) {
              const int j = tab_var<0>(g.cn_tab[e]);
              par ^= ew[j >> 5] >> (j & 31);
            }
          }
          un |= par & 1u;
        }
        ok = ballot_b(un != 0) == 0;
        if (ok) break;                              // the leg ends; the next starts from this M
      }
      if (ok) {
        ++found;
        Weight w = wt;
        if constexpr (VP) {
          if (cost) {
            // the solution's prior weight, formed only here: each lane sums the
            // weights of its own variables' set bits, then one wave reduction
            long long acc = 0;
            for (int j = lane; j < n; j += 64)
              if ((ew[j >> 5] >> (j & 31)) & 1u) acc += ld_const(wgt, j);
            w = relay_wave_sum(acc);
          }
        }
        if (w < best_w) {                           // ties keep the earlier one
          best_w = w;
          best_leg = r;
          for (int k = lane; k < ewords; k += 64) bw[k] = ew[k];
        }
      }
      wave_sync();
      if (found == ra.sols) break;
    }

    // ---------------- outputs (original column order) ----------------------
    const uint32_t* hw = found ? bw : ew;
    double* po = a.post ? a.post + hs * (long long)n : nullptr;
    for (int jo = lane; jo < n; jo += 64) {
      const int v = a.vinv[jo];
      put_ehat(a, hs, jo, ((hw[v >> 5] >> (v & 31)) & 1u) != 0);
      if (po) po[jo] = M[v];
    }
    const uint64_t bz = ballot((fl & FLAG_MIN_ZERO) != 0);
    if (lane == 0) {
      a.iters[hs] = iters;
      if (a.flags) a.flags[hs] = (int32_t)((bz ? FLAG_MIN_ZERO : 0) | (found ? FLAG_CONVERGED : 0));
      if (ra.info) {
        ra.info[2 * hs] = found;
        ra.info[2 * hs + 1] = best_leg;
      }
    }
    wave_sync();  // the next half-shot reuses this wave's LDS slice
  }
