// decode_kernel_body.inc — the body of decode_kernel / decode_prior_kernel /
// decode_vprior_kernel (decode_generic.h), included inside each kernel with
// `a` (DecodeArgs), ALGO, LAYERED, DC, a constexpr int PRI (PRI_SCALAR /
// PRI_MASK / PRI_ROW) and a constexpr bool TALL (flooding past
// QLDPC_SYNREG_CHECKS checks: the *_tall kernels, DC = 0) in scope.
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  // Stage the read-only graph blob into LDS (16-byte vector copies).
  {
    const uint4* src = (const uint4*)a.blob;
    uint4* dst = (uint4*)lds;
    const int nvec = a.blob_bytes >> 4;
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) dst[i] = src[i];
  }
  if constexpr (PRI == PRI_ROW) {
    // the code's prior row (relabeled order) behind the graph image: staged
    // once, shared by every wave of the workgroup
    double* dst = (double*)(lds + a.blob_bytes);
    for (int j = threadIdx.x; j < a.n; j += blockDim.x) dst[j] = a.vprior[j];
  }
  __syncthreads();

  LdsView g;
  g.cn_tab = (const uint32_t*)(lds + a.off_cn_tab);
  g.row_ptr = (const uint16_t*)(lds + a.off_row_ptr);
  g.vn_info = (const uint32_t*)(lds + a.off_vn_ptr);
  g.chunk_dmax = (const uint8_t*)(lds + a.off_chunk_dmax);
  g.vn_chk = (const uint16_t*)(lds + a.off_vn_chk);
  g.lay_ptr = (const uint16_t*)(lds + a.off_lay_ptr);
  g.lay_rows = (const uint16_t*)(lds + a.off_lay_rows);
  g.adj_ptr = (const uint16_t*)(lds + a.off_adj_ptr);
  g.adj_vars = (const uint16_t*)(lds + a.off_adj_vars);
  g.lt = nullptr;
  if constexpr (ALGO == ALGO_BP) {
    g.lt = stage_libm(lds, a.off_libm);
    __syncthreads();
  }

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int waves = blockDim.x >> 6;
  unsigned char* ws = lds + a.blob_bytes + (PRI == PRI_ROW ? a.vprior_bytes : 0) + wid * a.wave_bytes;
  double* post = (double*)ws;
  void* c2v = (void*)(ws + a.off_c2v);
  uint32_t* synw = (uint32_t*)(ws + a.off_synw);
  uint32_t* parw = (uint32_t*)(ws + a.off_parw);
  const uint32_t* selw = PRI == PRI_ROW    ? (const uint32_t*)(lds + a.blob_bytes)       // the prior row
                         : PRI == PRI_MASK ? (const uint32_t*)(ws + a.off_selw)
                                           : nullptr;

  const int m = a.m, n = a.n;
  const int nwords = (m + 31) >> 5;

  for (HalfShotQueue Q(a.batch, a.queue, waves, wid); Q.hs < a.batch; Q.advance()) {
    const long long hs = Q.hs;
    Q.prefetch(threadIdx.x & 63);
    int fl = 0;
    int iters = a.max_iter;
    bool conv = false;

    if constexpr (PRI == PRI_MASK) {
      // the half-shot's mask row (original column order) as selector bits in
      // relabeled order: lane reads the bit of variable j0 + lane's column,
      // one ballot per 64 variables (2 ceil(n / 64) words in the slice)
      uint32_t* sw = (uint32_t*)(ws + a.off_selw);
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const int bit = j < n ? (int)pmask_bit(a, hs, (int)a.vperm[j]) : 0;
        store_bits64(sw, j0, bit, lane);
      }
      wave_sync();
    }

    if constexpr (!LAYERED) {
      // ---------------- flooding: one layer holding every check ------------
      // Syndrome bits: a lane's checks are lane + 64 i, and one 32-bit register
      // holds bit i of up to 32 passes, QLDPC_SYNREG_CHECKS = 2048 checks. A
      // taller code runs the TALL instance, which keeps them in the slice's
      // synw words (wave_layout allocates those for flooding in that case
      // alone); every other instance is the code it was.
      uint32_t synreg = 0;  // bit i = syndrome of check lane + 64 i
      if constexpr (!TALL) {
        for (int i = 0, c = lane; c < m; ++i, c += 64) synreg |= syn_bit(a, hs, c) << i;
      } else {
        for (int c0 = 0; c0 < m; c0 += 64)
          store_bits64(synw, c0, c0 + lane < m ? (int)syn_bit(a, hs, c0 + lane) : 0, lane);
        wave_sync();
      }
#define QLDPC_SYNB(i, c) (TALL ? (synw[(c) >> 5] >> ((c) & 31)) & 1u : (synreg >> (i)) & 1u)
      if constexpr (ALGO == ALGO_BP) {
        // BP's first check-node pass reads v2c = L0 (decoders.py:235):
        // post = L0, c2v = 0. (MS's first pass reads float32(L) directly.)
        for (int j = lane; j < n; j += 64) post[j] = prior_of<PRI>(a, selw, j);
        double* cz = (double*)c2v;
        for (int p = lane; p < a.E; p += 64) cz[p] = 0.0;
        wave_sync();
      }
      for (int it = 0;; ++it) {
        // CN over all checks; its parity pass is the stop test of iteration it-1
        // (decoders.py:175-176 — checks read the posteriors the last VN wrote).
        uint32_t unsat = 0;
        if constexpr (QLDPC_ABLATE == 2) {
          unsat = 1;
        } else if constexpr (ALGO == ALGO_MS && DC > 0) {
          for (int i = 0, c = lane; c < m; ++i, c += 64) {
            uint32_t t[1][8];
            load_row8(g.cn_tab + c * 8, t[0]);
            const uint32_t sb[1] = {QLDPC_SYNB(i, c)};
            const bool live[1] = {true};
            if (PRI && it == 0)
              (void)cn_update<ALGO, DC, PRI>(a, g, c, sb[0], true, post, c2v, fl, selw);
            else if (it == 0)
              (void)cn_ms_uniform<DC, true, 1>(a, t, sb, live, (const unsigned char*)post, (unsigned char*)c2v, fl);
            else
              unsat |= cn_ms_uniform<DC, false, 1>(a, t, sb, live, (const unsigned char*)post, (unsigned char*)c2v, fl);
          }
        } else if (it == 0) {
          for (int i = 0, c = lane; c < m; ++i, c += 64)
            (void)cn_update<ALGO, DC, PRI>(a, g, c, QLDPC_SYNB(i, c), true, post, c2v, fl, selw);
        } else {
          for (int i = 0, c = lane; c < m; ++i, c += 64)
            unsat |= cn_update<ALGO, DC, PRI>(a, g, c, QLDPC_SYNB(i, c), false, post, c2v, fl, selw);
        }
        if (it > 0 && ballot(unsat != 0) == 0) {
          iters = it;
          conv = true;
          break;
        }
        wave_sync();
        if constexpr (QLDPC_ABLATE != 1) {
          for (int j0 = 0; j0 < n; j0 += 64) {
            const int dmax = __builtin_amdgcn_readfirstlane((int)g.chunk_dmax[j0 >> 6]);
            const int j = j0 + lane;
            if (j < n) post[j] = vn_post<ALGO, PRI>(a, g, j, c2v, dmax, selw);
          }
        }
        wave_sync();
        if (it + 1 == a.max_iter) {
          // final stop test after the last VN (its result only sets the flag:
          // both branches of the reference return max_iter, :176 / :182)
          uint32_t un = 0;
          for (int i = 0, c = lane; c < m; ++i, c += 64) {
            const int e0 = DC ? c * 8 : (int)g.row_ptr[c];
            const int deg = DC ? DC : (int)g.row_ptr[c + 1] - e0;
            uint32_t par = 0;
            for (int k = 0; k < deg; ++k) par ^= (uint32_t)(post[tab_var<DC>(g.cn_tab[e0 + k])] < 0.0);
            un |= par ^ QLDPC_SYNB(i, c);
          }
          conv = ballot(un != 0) == 0;
          break;
        }
      }
#undef QLDPC_SYNB
    } else {
      // ---------------- layered / serial: explicit row lists ----------------
      // State starts at c2v = 0, post = L (msg_v2c = L, :148-149 / :235).
      const double L = a.L;
      for (int j = lane; j < n; j += 64) post[j] = prior_of<PRI>(a, selw, j);
      if constexpr (ALGO == ALGO_MS) {
        float* c = (float*)c2v;
        for (int p = lane; p < a.E; p += 64) c[p] = 0.0f;
      } else {
        double* c = (double*)c2v;
        for (int p = lane; p < a.E; p += 64) c[p] = 0.0;
      }
      // syndrome bits and the parity of the initial hard decisions (all = L<0)
      for (int c0 = 0; c0 < m; c0 += 64) {
        const int c = c0 + lane;
        const int in = c < m;
        store_bits64(synw, c0, in ? (int)syn_bit(a, hs, c) : 0, lane);
        int deg = 0;
        if (in) deg = DC ? DC : (int)g.row_ptr[c + 1] - (int)g.row_ptr[c];
        if constexpr (PRI) {
          // (L_j < 0 differs per variable: the row's parity edge by edge)
          uint32_t par = 0;
          const int e0 = DC ? c * 8 : (in ? (int)g.row_ptr[c] : 0);
          for (int k = 0; k < deg; ++k)
            par ^= (uint32_t)(prior_of<PRI>(a, selw, tab_var<DC>(g.cn_tab[e0 + k])) < 0.0);
          store_bits64(parw, c0, (int)par, lane);
        } else {
          store_bits64(parw, c0, in && (L < 0.0) && (deg & 1), lane);
        }
      }
      wave_sync();
      bool first = true;
      for (int it = 0; it < a.max_iter && !conv; ++it) {
        for (int l = 0; l < a.n_layers; ++l) {
          // CN over the layer's rows (Jacobi: all read the same posteriors)
          const int q0 = g.lay_ptr[l], q1 = g.lay_ptr[l + 1];
          for (int q = q0 + lane; q < q1; q += 64) {
            const int c = g.lay_rows[q];
            const uint32_t sb = (synw[c >> 5] >> (c & 31)) & 1u;
            (void)cn_update<ALGO, DC, PRI>(a, g, c, sb, first, post, c2v, fl, selw);
          }
          first = false;
          wave_sync();
          // VN over the variables adjacent to the layer (others are unchanged,
          // so recomputing every column as decoders.py:172 / :265 does is
          // bit-identical); hard-decision flips toggle check parities.
          const int v0 = g.adj_ptr[l], v1 = g.adj_ptr[l + 1];
          for (int q = v0 + lane; q < v1; q += 64) {
            const int j = g.adj_vars[q];
            const double old = post[j];
            const double nw = vn_post<ALGO, PRI>(a, g, j, c2v, -1, selw);
            post[j] = nw;
            if ((old < 0.0) != (nw < 0.0)) {
              const uint32_t info = g.vn_info[j];
              for (int p = (int)(info & 0xffffu), pe = p + (int)(info >> 16); p < pe; ++p) {
                const int c = g.vn_chk[p];
                atomicXor(&parw[c >> 5], 1u << (c & 31));
              }
            }
          }
          wave_sync();
          // stop test after every layer (:175-176 / :283-285)
          uint32_t un = 0;
          for (int w = lane; w < nwords; w += 64) un |= parw[w] ^ synw[w];
          if (ballot(un != 0) == 0) {
            iters = it + 1;
            conv = true;
            break;
          }
        }
      }
    }

    // ---------------- outputs (original column order) ----------------------
    double* po = a.post ? a.post + hs * (long long)n : nullptr;
    for (int jo = lane; jo < n; jo += 64) {
      const double pv = post[a.vinv[jo]];
      put_ehat(a, hs, jo, pv < 0.0);                  // e_hat = post < 0 (:174 / :280)
      if (po) po[jo] = pv;
    }
    // OR the lane-local flags across the wave
    uint32_t fall = 0;
    {
      const uint64_t b1 = ballot((fl & FLAG_MIN_ZERO) != 0);
      const uint64_t b2 = ballot((fl & FLAG_NONFINITE) != 0);
      fall = (b1 ? FLAG_MIN_ZERO : 0) | (b2 ? FLAG_NONFINITE : 0) | (conv ? FLAG_CONVERGED : 0);
    }
    if (lane == 0) {
      a.iters[hs] = iters;
      if (a.flags) a.flags[hs] = (int32_t)fall;
    }
    wave_sync();  // the next half-shot reuses this wave's LDS slice
  }
