// osd_block_body.inc — the body of osd_block_kernel, osd_block_cs_kernel and osd_block_cs_prior_kernel
// (osd_block.h; template parameters NW, SL, RT, argument `a`; LDS bytes: osd_block_lds, osd_kernels.h),
// included once per kernel. QLDPC_OSD_BLOCK_CS = 1 ends it with the OSD-CS epilogue
// (osd_cs_epilogue), 2 with the prior-weighted one (osd_cs_prior_epilogue) instead of the order-0 one; with 0 the text is the
// order-0 kernel's alone, so that kernel's machine code does not depend on
// the other's.
  // LDS: inv_perm[n] | J list [m+2] | inJ bytes [n] | emask [NW] | Wd [MR] | Cm [MR] |
  //      PW [64][NW] | PX [32][NW] (QLDPC_OSD_PAIRS) | CT [64] | pkof [MR] | pidx [MR] | crow [MR] | pk [64] | misc [16] | set table
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int m = a.m, n = a.n;
  const int B = blockDim.x, MR = RT * B;
  int* inv = (int*)lds;
  int* Jl = inv + n;
  unsigned char* inJ = (unsigned char*)(Jl + m + 2);
  uint64_t* emask = (uint64_t*)(lds + ((4 * (n + m + 2) + n + 15) & ~15));
  uint64_t* Wd = emask + NW;
  uint64_t* Cm = Wd + MR;
  uint64_t* PW = Cm + MR;                            // [64][NW]
  uint64_t* PX = PW + 64 * NW;                       // [32][NW] pivot pairs (QLDPC_OSD_PAIRS)
  uint64_t* CT = PX + (QLDPC_OSD_PAIRS ? 32 * NW : 0);   // C of this block's pivot by its column bit
  int* pkof = (int*)(CT + 64);                       // pivot tag per row: 64 w + k, -1 none
  int* pidx = pkof + MR;                             // pivot index of each row (m: none)
  int* crow = pidx + MR;                             // compact position -> row (free rows)
  int* pk = crow + MR;                               // pivot k: compact position << 6 | column bit
  int* misc = pk + 64;                               // [0] nJ [1] rank [2] i0 [3] flag [4] done [5] K
                                                     // [6..7] this block's pivot-column mask
                                                     // [8..11] SIMD of each wave [12] engine SIMD
  int* table = misc + 16;

  const int t = threadIdx.x;
  // readfirstlane: `wave` is then known to be wave-uniform, so the engine's
  // branch is scalar and the counters it updates stay in SGPRs
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const long long shot = blockIdx.x;
  if (osd_host_shot(a, shot, n, misc + 7)) return;
  const int32_t* perm = a.perm + shot * (long long)n;
  const uint8_t* syn = a.syn + shot * (long long)m;
  uint8_t* ehat = a.ehat + shot * (long long)n;

  for (int i = t; i < n; i += blockDim.x) {
    inv[perm[i]] = i;
    inJ[i] = 0;
  }
#pragma unroll
  for (int h = 0; h < RT; ++h) {
    pkof[t + h * B] = -1;
    pidx[t + h * B] = m;
  }
  // Phase B runs on one "engine" wave while the workgroup's other waves wait
  // at the barrier, and a CU runs 4 shots (workgroups) whose 4 waves sit on
  // its 4 SIMDs, wave 0 on a SIMD that rotates between workgroups: engines of
  // co-resident shots often shared a SIMD. Each workgroup takes a per-CU
  // ticket and runs its engine on the wave placed on SIMD (ticket mod 4), so
  // the engines of 4 consecutive workgroups of a CU use 4 SIMDs.
  if (lane == 0 && wave < 4) misc[8 + wave] = (int)((__builtin_amdgcn_s_getreg(kHwRegHwId) >> 4) & 3u);
  if (t == 0) {
    misc[3] = 0;
    uint32_t tk = 0;
    if (a.cu_tickets) {
      const uint32_t hw = __builtin_amdgcn_s_getreg(kHwRegHwId), xcc = __builtin_amdgcn_s_getreg(kHwRegXccId);
      tk = atomicAdd(a.cu_tickets + (((xcc & 15u) << 8) | ((hw >> 8) & 0xffu)), 1u);
    }
    misc[12] = (int)(tk & 3u);
  }
  __syncthreads();
  int engine = 0;
  {
    const int target = misc[12], nwv = (int)(blockDim.x >> 6);
    for (int w = 0; w < 4 && w < nwv; ++w)
      if (misc[8 + w] == target) engine = w;
    engine = __builtin_amdgcn_readfirstlane(engine);
  }

  // my rows of Hp (+ syndrome bit at column n)
  uint64_t R[RT][NW];
  bool own[RT];
#pragma unroll
  for (int h = 0; h < RT; ++h) {
    const int r = t + h * B;
    own[h] = r < m;
#pragma unroll
    for (int w = 0; w < NW; ++w) R[h][w] = 0;
    if (own[h]) {
      for (int e = a.row_ptr[r]; e < a.row_ptr[r + 1]; ++e) {
        const int i = inv[a.col_idx[e]];
#pragma unroll
        for (int w = 0; w < NW; ++w)
          if ((i >> 6) == w) R[h][w] |= 1ull << (i & 63);
      }
      if (syn[r] & 1) {
#pragma unroll
        for (int w = 0; w < NW; ++w)
          if ((n >> 6) == w) R[h][w] |= 1ull << (n & 63);
      }
    }
  }

  int rank = 0, nJ = 1;
  bool done = a.rank == 0;                            // rank(H) = 0: IndexError below
  if (t == 0) {
    Jl[0] = 0;                                        // column 0 always (decoders.py:329)
    inJ[0] = 1;
  }

  // runtime block loop (one copy of phase B); R is only ever indexed by the
  // compile-time x of the unrolled word loops, so it stays in VGPRs
  unsigned long long tp[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long tc = QLDPC_OSD_TIMING ? clock64() : 0;
#define QLDPC_TICK(k)                            \
  if constexpr (QLDPC_OSD_TIMING != 0) {         \
    const unsigned long long now = clock64();    \
    tp[k] += now - tc;                           \
    tc = now;                                    \
  }
  QLDPC_TICK(0);                                      // setup
  for (int w = 0; w < NW && 64 * w < n && !done; ++w) {   // done: uniform, re-read per block
#pragma unroll
    for (int h = 0; h < RT; ++h)                      // A
      if (own[h]) {
        uint64_t v = 0;
#pragma unroll
        for (int x = 0; x < NW; ++x)
          if (x == w) v = R[h][x];
        Wd[t + h * B] = v;
      }
    __syncthreads();
    QLDPC_TICK(1);
    if (wave == engine) {                             // B
      // The engine is its shot's critical path while the SIMD also runs
      // other shots' phase-D waves: raised priority lets it issue first.
      if constexpr (QLDPC_OSD_PRIO != 0) __builtin_amdgcn_s_setprio(QLDPC_OSD_PRIO);
      // the engine works on the rows still free (no pivot yet), compacted:
      // crow[c] = the c-th free row; earlier pivots are reduced in phase D
      const int rank0 = rank;
      int F = 0;
      // every read of a slot loop issued before the first use (left alone,
      // each slot's read sat in its own exec-masked block with its own wait:
      // 8 dependent LDS round trips on the engine's chain, twice per block)
      int pv[SL];
#pragma unroll
      for (int s = 0; s < SL; ++s) pv[s] = pidx[64 * s + lane];     // (64 SL = MR row slots)
#pragma unroll
      for (int s = 0; s < SL; ++s) asm volatile("" : "+v"(pv[s]));
#pragma unroll
      for (int s = 0; s < SL; ++s) {
        const int row = 64 * s + lane;
        const bool fr = row < m && pv[s] == m;
        const uint64_t bf = __ballot(fr);
        if (fr) crow[F + __builtin_amdgcn_mbcnt_hi((uint32_t)(bf >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bf, 0))] = row;
        F += __builtin_popcountll(bf);
      }
      uint32_t lo[SL], hi[SL], cl[SL], ch[SL];
      uint64_t fm[SL];                                // slot s: lanes whose compact row is not yet a pivot
      uint32_t alo = 0, ahi = 0;                      // columns some free row holds
      int cr[SL];
#pragma unroll
      for (int s = 0; s < SL; ++s) cr[s] = crow[64 * s + lane];     // (this wave's writes above: in order)
#pragma unroll
      for (int s = 0; s < SL; ++s) asm volatile("" : "+v"(cr[s]));
      uint64_t wv[SL];
#pragma unroll
      for (int s = 0; s < SL; ++s) wv[s] = Wd[64 * s + lane < F ? cr[s] : 0];
#pragma unroll
      for (int s = 0; s < SL; ++s) asm volatile("" : "+v"(wv[s]));
#pragma unroll
      for (int s = 0; s < SL; ++s) {
        const int cp = 64 * s + lane;
        const uint64_t v = cp < F ? wv[s] : 0ull;
        lo[s] = (uint32_t)v;
        hi[s] = (uint32_t)(v >> 32);
        cl[s] = ch[s] = 0;
        fm[s] = __ballot(cp < F);
        alo |= lo[s];
        ahi |= hi[s];
      }
      uint64_t cols = ((uint64_t)wave_or32(ahi) << 32) | wave_or32(alo);
      if (n - 64 * w < 64) cols &= (1ull << (n - 64 * w)) - 1;
      if constexpr ((QLDPC_ABLATE_OSD & 2) != 0) cols = 0;
      const int SF = (F + 63) >> 6;
      uint64_t pivm = 0;
      // low half-word columns, then high (each loop's column order ascends)
      const int nJ0 = nJ;
      int pkv = 0;
      int K = block_half_n<SL, SL, false>(SF, lo, hi, cl, ch, fm, (uint32_t)cols, 0, w, lane, rank, nJ, done,
                                          pivm, a.rank, m, pkv);
      K = block_half_n<SL, SL, true>(SF, lo, hi, cl, ch, fm, (uint32_t)(cols >> 32), K, w, lane, rank, nJ, done,
                                     pivm, a.rank, m, pkv);
#pragma unroll
      for (int s = 0; s < SL; ++s) {
        const int cp = 64 * s + lane;
        if (cp < F) Cm[crow[cp]] = ((uint64_t)ch[s] << 32) | cl[s];
      }
      // (one wave: its LDS accesses complete in order, so the reads below see
      // the writes above)
      {
        // the block's J entries (column 0 is J's first entry from the start)
        const int ivv = 64 * w + (pkv & 63);
        const int z = (K > 0 && __builtin_amdgcn_readlane(ivv, 0) == 0) ? 1 : 0;
        if (lane < K) {
          pk[lane] = pkv;
          if (ivv != 0) {
            Jl[nJ0 + lane - z] = ivv;
            inJ[ivv] = 1;
          }
          const int e = pkv;
          const int row = crow[e >> 6];
          CT[e & 63] = Cm[row] ^ (1ull << lane);      // reduced pivot k = its own row + C
          pkof[row] = 64 * w + lane;
          pidx[row] = rank0 + lane;                   // REF moves the k-th pivot row to row k
        }
        if (lane == 0) {
          misc[0] = nJ;
          misc[1] = rank;
          misc[4] = done;
          misc[5] = K;
          misc[6] = (int)(uint32_t)pivm;
          misc[7] = (int)(uint32_t)(pivm >> 32);
        }
      }
      if constexpr (QLDPC_OSD_PRIO != 0) __builtin_amdgcn_s_setprio(0);
    }
    QLDPC_TICK(2);
    __syncthreads();
    QLDPC_TICK(3);
    nJ = __builtin_amdgcn_readfirstlane(misc[0]);    // (LDS loads count as per-lane values)
    rank = __builtin_amdgcn_readfirstlane(misc[1]);
    done = __builtin_amdgcn_readfirstlane(misc[4]) != 0;
    const int K = __builtin_amdgcn_readfirstlane(misc[5]);
    const uint64_t pivm = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(misc[7]) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane(misc[6]);
    // C: pivot rows publish their words w.. as they were at the block start
    int tag[RT];
#pragma unroll
    for (int h = 0; h < RT; ++h) {
      tag[h] = own[h] ? pkof[t + h * B] : -1;
      if (tag[h] >= 0 && (tag[h] >> 6) == w) {
        uint64_t* dst = PW + (tag[h] & 63) * NW;
#pragma unroll
        for (int x = 0; x < NW; ++x)
          if (x >= w) dst[x] = R[h][x];
      }
    }
    __syncthreads();
    if constexpr (QLDPC_OSD_PAIRS != 0) {
      // pair rows PX[j] = PW[2j] ^ PW[2j + 1], words w.. (pairs of this block's pivots)
      if (K > 1) {                                    // (uniform)
        const int np = K >> 1, nx = NW - w;
        for (int i = t; i < np * nx; i += B) {
          const int j = i / nx, x = w + i - j * nx;
          PX[j * NW + x] = PW[2 * j * NW + x] ^ PW[(2 * j + 1) * NW + x];
        }
        __syncthreads();
      }
    }
    QLDPC_TICK(4);
    // D: every row applies its combination of this block's pivot rows
#pragma unroll
    for (int h = 0; h < RT; ++h)
    if (own[h] && K > 0 && (QLDPC_ABLATE_OSD & 1) == 0) {
      uint64_t cm;
      if (tag[h] >= 0 && (tag[h] >> 6) < w) {
        // a pivot row of an earlier block: clear this block's pivot columns
        // from it. Its result is unique (word w + the reduced block pivots it
        // holds a 1 for), so C = XOR of those pivots' C (no engine pass).
        uint64_t v = 0;
#pragma unroll
        for (int x = 0; x < NW; ++x)
          if (x == w) v = R[h][x];
        cm = osd_gather_xor4(CT, v & pivm);
      } else {
        cm = Cm[t + h * B];
      }
      // (per-lane gathers of the pivot rows: a uniform loop over all K with
      // broadcast reads measured 2x slower, VALU-bound). The word range is a
      // compile-time one per block (switch on w), so a pivot row's words are
      // all read before any XOR — one LDS round trip per pivot row instead
      // of one per word behind a uniform branch.
      osd_apply_rows<NW>(R[h], cm, PW, PX, w);
    }
    QLDPC_TICK(5);
  }
  if constexpr (QLDPC_OSD_TIMING != 0) {
    if (lane == 0 && (wave == engine || wave == (engine ^ 1)))   // [0]: the engine wave, [1]: another
      for (int k = 0; k < 6; ++k) atomicAdd(a.prof + 8 * (wave == engine ? 0 : 1) + k, tp[k]);
  }
#undef QLDPC_TICK
  if (rank < a.rank) {                              // greedy loop runs past column n-1
    if (t == 0) a.status[shot] = 1;                 // (the reference raises IndexError)
    return;
  }
  // a row left without pivot is zero on every column of H; a 1 in its
  // syndrome column means s is outside H's column space (status 3)
  int mypos[RT];
#pragma unroll
  for (int h = 0; h < RT; ++h) {
    mypos[h] = own[h] ? pidx[t + h * B] : m;
    uint64_t sbit = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w)
      if (w == (n >> 6)) sbit = (R[h][w] >> (n & 63)) & 1ull;   // (compile-time R index)
    if (own[h] && mypos[h] >= nJ && sbit) misc[3] = 1;
  }
  if (t == 0) {
    int i0 = -1;
    if (a.order == 1 && nJ < n) i0 = first_setdiff(n, inJ, nJ, table);   // (decoders.py:344)
    misc[2] = i0;
  }
  __syncthreads();
  const int i0 = misc[2];
  if (misc[3]) {
    if (t == 0) a.status[shot] = 3;
    return;
  }
  // information-set values e_I (e_perm = e_hat[perm], decoders.py:345)
  for (int i0w = 64 * wave; i0w < 64 * NW; i0w += blockDim.x) {
    const int i = i0w + lane;
    const bool bit = i < n && !inJ[i] && (ehat[perm[i]] & 1);
    const uint64_t bits = __ballot(bit);
    if (lane == 0) emask[i0w >> 6] = bits;
  }
  __syncthreads();
#if QLDPC_OSD_BLOCK_CS
#if QLDPC_OSD_BLOCK_CS == 2
  osd_cs_prior_epilogue<NW, RT>(a, R, own, mypos, nJ, Jl, inJ, emask, Wd, perm, ehat);
#else
  osd_cs_epilogue<NW, RT>(a, R, own, mypos, nJ, Jl, inJ, emask, Wd, perm, ehat);
#endif
  if (t == 0) a.status[shot] = 0;
  return;
#endif
  if (t == 0 && i0 >= 0) emask[i0 >> 6] ^= 1ull << (i0 & 63);   // order-1 flip (:349-350)
  __syncthreads();
  // e_J = (T sJ)[:|J|]: the k-th pivot row gives entry k   (decoders.py:352-358)
#pragma unroll
  for (int h = 0; h < RT; ++h)
    if (own[h] && mypos[h] < nJ) {
      uint64_t acc = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (w == (n >> 6)) acc ^= (R[h][w] >> (n & 63)) & 1ull;   // T s (augmented column)
        acc ^= (uint64_t)(__builtin_popcountll(R[h][w] & emask[w]) & 1);
      }
      ehat[perm[Jl[mypos[h]]]] = (uint8_t)(acc & 1ull);         // e_hat[perm] = ... (:368)
    }
  if (t == 0 && i0 >= 0) ehat[perm[i0]] ^= 1;
  if (t == 0) a.status[shot] = 0;
