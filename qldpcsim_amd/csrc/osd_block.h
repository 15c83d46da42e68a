// osd_block.h — osd_block_kernel<NW, SL, RT>, its two OSD-CS twins (Hamming and prior-weighted cost) and their
// helpers; the body is osd_block_body.inc.
#pragma once
#include "osd_common.h"

namespace qldpc {

// ---------------------------------------------------------------------------
// Block elimination (the default GPU OSD): one workgroup barrier per 64-column
// word instead of one per column (osd_kernel spends most of its instructions
// on that per-column protocol). Thread t owns row t of Hp (+ syndrome).
//
// Pivot rows are chosen by row index (the first unused row holding a 1), not
// by REF's row order. That changes T but not what OSD reads from it: the
// pivot columns J are the columns independent of their predecessors (a
// property of Hp), and the fully reduced pivot row of column j_k gives the
// k-th entry of e_J = the unique solution of H_J x = s + H_I e_I (DESIGN.md
// §3, OSD). Two cases need REF's own order and go to osd_kernel instead: an
// all-zero column 0 (the host never selects this kernel for an H with a zero
// column) and a syndrome outside the column space of H (status 3 here, then
// osd_kernel redoes those shots in the same stream).
//
// Per word w:
//   A  every row publishes its word w
//   B  wave 0 runs the elimination over the 64 columns of word w alone on
//      that copy (row 64 s + lane in slot s): word value, and C = the set of
//      this block's pivot rows (by block-start value) XOR-ed into it so far.
//      Column i: pivot = first unused row with a 1 (ballots), every other row
//      with a 1 is XOR-ed with it: word ^= pivot word, C ^= C_pivot ^ {pivot}.
//      Columns no unused row holds are skipped unseen: XORs among unused rows
//      never set a bit that none of them held.
//   C  the block's pivot rows publish their words w.. (still block-start values)
//   D  every row applies its C to words w..: each update added a current
//      pivot row = its block-start value + earlier pivot rows of the block.
// ---------------------------------------------------------------------------
// x with lane `l` replaced by the wave-uniform v (v_writelane_b32)
__device__ __forceinline__ uint32_t write_lane(uint32_t x, uint32_t v, int l) {
  asm("v_writelane_b32 %0, %1, m0" : "+v"(x) : "s"(v), "{m0}"(l));   // (gfx9: one SGPR operand, lane in M0)
  return x;
}

__device__ __forceinline__ uint32_t wave_or32(uint32_t x) {
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xf, 0xf, false);  // row_half_mirror
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xf, 0xf, false);  // row_mirror
  return (uint32_t)(__builtin_amdgcn_readlane((int)x, 0) | __builtin_amdgcn_readlane((int)x, 16) |
                    __builtin_amdgcn_readlane((int)x, 32) | __builtin_amdgcn_readlane((int)x, 48));
}

// Phase B over the columns `cols` of one half-word (HI: bits 32..63, read
// from hi[]) on the first SF compact slots, straight-line per column: one
// ballot per slot masked by the slot's still-free rows (fm[s], a wave-uniform
// lane mask in SGPRs); the slot that hits reads the pivot's values (readlane
// under its compile-time slot index: no dispatch on the slot afterwards) and
// clears the pivot's own column bit in the pivot row, so the elimination
// needs no per-slot exclusion of the pivot row: within the block the row's
// bits at this or earlier columns are never read again, and the engine's
// lo/hi words are dropped at the block end (only cl/ch leave it).
// Pivot k's compact position and column bit go to pk[k]; returns the pivot
// count K.
template <int SL, int SF, bool HI>
__device__ __forceinline__ int block_half(uint32_t (&lo)[SL], uint32_t (&hi)[SL], uint32_t (&cl)[SL],
                                          uint32_t (&ch)[SL], uint64_t (&fm)[SL], uint32_t cols, int K,
                                          int w, int lane, int& rank, int& nJ, bool& done, uint64_t& pivm,
                                          int rankH, int m, int& pkv) {
  while (cols && !done) {
    // loop-carried scalars re-asserted wave-uniform: otherwise the compiler
    // keeps them per lane and turns the loop into an exec-masked one
    cols = (uint32_t)__builtin_amdgcn_readfirstlane((int)cols);
    K = __builtin_amdgcn_readfirstlane(K);
    rank = __builtin_amdgcn_readfirstlane(rank);
    nJ = __builtin_amdgcn_readfirstlane(nJ);
    pivm = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(pivm >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)pivm);
    // next column with a pivot: slots scanned in ascending order, the scan
    // stops at the first hit (uniform branches) — once rows fill up, slot 0
    // almost always holds the pivot. Dependent columns (no free row holds
    // them) are skipped without touching the state; they are not in J.
    int f = -1, bit = 0;
    uint32_t plo = 0, phi = 0, pcl = 0, pch = 0;
    while (cols && f < 0) {
      bit = (int)__builtin_ctz(cols);
      cols &= cols - 1;
      const uint32_t bm = 1u << bit;
#pragma unroll
      for (int s = 0; s < SF; ++s) {
        const uint64_t c = __ballot(((HI ? hi[s] : lo[s]) & bm) != 0) & fm[s];
        if (c) {
          const int fl = (int)__builtin_ctzll(c);
          f = 64 * s + fl;
          plo = __builtin_amdgcn_readlane((int)lo[s], fl);
          phi = __builtin_amdgcn_readlane((int)hi[s], fl);
          pcl = __builtin_amdgcn_readlane((int)cl[s], fl);
          if (HI) pch = __builtin_amdgcn_readlane((int)ch[s], fl);
          fm[s] &= ~(1ull << fl);                     // no longer free
          if (HI) hi[s] = write_lane(hi[s], phi & ~bm, fl);
          else lo[s] = write_lane(lo[s], plo & ~bm, fl);
          break;
        }
      }
      f = __builtin_amdgcn_readfirstlane(f);
    }
    if (f < 0) break;                               // (dependent columns: not in J)
    // (+ the pivot itself; the 64-bit form, (pch:pcl) ^ (1ull << K), was
    // miscompiled in the 128-VGPR spilling instance: wrong eliminations,
    // correct at 3 waves per SIMD without spills — tools/osd_check.py)
    if (HI) {
      const uint32_t kb = 1u << (K & 31);
      pcl ^= K < 32 ? kb : 0u;
      pch ^= K < 32 ? 0u : kb;
    } else {
      pcl ^= 1u << K;                               // (low half: K < 32)
    }
    // Rows holding a 1 (above and below) take the pivot: x ^= p & mask with
    // mask = 0 / ~0 from the column bit (one bit-field extract) — branch-free
    // (v_bitop3), no exec-mask round trip from a VALU compare through SALU
    // per slot. The low half is done in HI. In the low half the block has
    // fewer than 32 pivots, so every C word's high half is still zero (no
    // ch update).
#pragma unroll
    for (int s = 0; s < SF; ++s) {
      const uint32_t mk = (uint32_t)__builtin_amdgcn_sbfe((int)(HI ? hi[s] : lo[s]), bit, 1);   // 0 / -1
      if (!HI) lo[s] ^= plo & mk;
      hi[s] ^= phi & mk;
      cl[s] ^= pcl & mk;
      if (HI) ch[s] ^= pch & mk;
    }
    const int wb = (HI ? 32 : 0) + bit;
    const int i = 64 * w + wb;
    pivm |= 1ull << wb;
    // pivot K's record (compact row << 6 | column bit) goes to lane K of a
    // VGPR (no exec-masked LDS store per pivot); the block's pk / Jl / inJ
    // entries are written once after the engine loop
    pkv = lane == K ? ((f << 6) | wb) : pkv;
    if (i != 0) ++nJ;
    ++K;
    ++rank;
    if (rank >= rankH || rank >= m) done = true;
    if (i == 0 && done) rank = -1;                  // column 0 alone reaches rank(H): the
                                                    // greedy loop never breaks (:333-342)
  }
  return K;
}

// block_half on the smallest power-of-two slot count >= SF (code per count)
template <int SL, int SFMAX, bool HI>
__device__ __forceinline__ int block_half_n(int SF, uint32_t (&lo)[SL], uint32_t (&hi)[SL], uint32_t (&cl)[SL],
                                            uint32_t (&ch)[SL], uint64_t (&fm)[SL], uint32_t cols, int K,
                                            int w, int lane, int& rank, int& nJ, bool& done, uint64_t& pivm,
                                            int rankH, int m, int& pkv) {
  if constexpr (SFMAX > 1) {
    if (SF <= SFMAX / 2)
      return block_half_n<SL, SFMAX / 2, HI>(SF, lo, hi, cl, ch, fm, cols, K, w, lane, rank, nJ, done, pivm,
                                             rankH, m, pkv);
  }
  return block_half<SL, SFMAX, HI>(lo, hi, cl, ch, fm, cols, K, w, lane, rank, nJ, done, pivm, rankH, m, pkv);
}

// XOR of the 64-bit table entries tab[k] over the set bits k of v, four
// gathers in flight per trip
__device__ __forceinline__ uint64_t osd_gather_xor4(const uint64_t* tab, uint64_t v) {
  uint64_t acc = 0;
  while (v) {
    int k[4];
    uint64_t mk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mk[j] = v ? ~0ull : 0ull;
      k[j] = v ? (int)__builtin_ctzll(v) : 0;
      v &= v - 1;
    }
    uint64_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = tab[k[j]];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc ^= c[j] & mk[j];
  }
  return acc;
}

template <int NW, int W0>
__device__ __forceinline__ void osd_apply_from(uint64_t (&R)[NW], uint64_t cm, const uint64_t* PW, const uint64_t* PX) {
  // a pivot row's words W0.. in one read batch, or in two when more than
  // QLDPC_OSD_DSPLIT words remain: the peak register need of phase D is the
  // rows' state plus one batch. QLDPC_OSD_PAIRS: pivots taken two at a time
  // (k = 2j, 2j + 1), PX[j] = PW[2j] ^ PW[2j + 1]: one row read per nonzero
  // pair of cm's bits instead of one per bit
  constexpr int NB = NW - W0, B1 = (QLDPC_OSD_DSPLIT > 0 && NB > QLDPC_OSD_DSPLIT) ? (NB + 1) / 2 : NB;
  uint64_t it = QLDPC_OSD_PAIRS ? (cm | (cm >> 1)) & 0x5555555555555555ull : cm;
  while (it) {
    const int k = (int)__builtin_ctzll(it);
    it &= it - 1;
    const uint64_t* src;
    if constexpr (QLDPC_OSD_PAIRS != 0) {
      const int b = (int)(cm >> k) & 3;
      src = b == 3 ? PX + (k >> 1) * NW : PW + (k + (b >> 1)) * NW;
    } else {
      src = PW + k * NW;
    }
    uint64_t v[B1];
#pragma unroll
    for (int x = 0; x < B1; ++x) v[x] = src[W0 + x];
#pragma unroll
    for (int x = 0; x < B1; ++x) R[W0 + x] ^= v[x];
    if constexpr (B1 < NB) {
      uint64_t u[NB - B1];
#pragma unroll
      for (int x = 0; x < NB - B1; ++x) u[x] = src[W0 + B1 + x];
#pragma unroll
      for (int x = 0; x < NB - B1; ++x) R[W0 + B1 + x] ^= u[x];
    }
  }
}

// R[x] ^= PW[k][x] for x >= w and every set bit k of cm (w wave-uniform)
template <int NW, int W0 = 0>
__device__ __forceinline__ void osd_apply_rows(uint64_t (&R)[NW], uint64_t cm, const uint64_t* PW, const uint64_t* PX,
                                               int w) {
  if constexpr (W0 < NW) {
    if (w == W0) osd_apply_from<NW, W0>(R, cm, PW, PX);
    else osd_apply_rows<NW, W0 + 1>(R, cm, PW, PX, w);
  }
}

// ---------------------------------------------------------------------------
// OSD-CS epilogue of osd_block_kernel: the combination sweep
// over the fully reduced [Hp | s] the block loop leaves in registers. With J
// the pivot columns and T the others (ascending), pivot row r holds row r of
// B^-1 H_T on T's columns and of B^-1 s in the syndrome column. Candidates in
// order: the order-0 estimate e0; one flip of T[k], every k; two flips T[a],
// T[b], a < b < L = min(lambda, |T|). Flipping a set F of T columns XORs those
// columns of B^-1 H_T into e0_J, so its cost change is
//   sum over F of (1 - 2 e_T) + sum over pivot rows r of x[r] (1 - 2 e0_J[r]),
// x = the XOR of F's columns. The first candidate of strictly smallest cost
// wins: the minimum of (cost change + 2048) << 13 | candidate index, index 0 =
// e0, 1 + c = the flip of perm position c, 2048 + 64 a + b = the pair (a, b).
//
// A column over the pivot rows is the ballots of "my row holds a 1" (word q =
// h * waves + wave covers rows 64 wave + lane + h * blockDim); two scalar
// popcounts against the same ballots of e0_J give the wave's share of the
// column's sum, added to an LDS counter per column. The first L columns'
// ballots stay in LDS; a pair costs one XOR and two popcounts per word.
//
// LDS: the block loop's Wd | Cm | PW | PX | CT, dead by now, as
//   colv [64][Q] u64 | ejm [Q] u64 | tmask [NW] u64 | cnt [64 NW] i32 | tl [64] i32 | red [4] i32
// with Q = MR / 64 words per column: osd_cs_lds bytes of the region's
// osd_block_cs_room (osd_kernels.h; the launcher checks that they fit).
// ---------------------------------------------------------------------------
constexpr int kCsIdxBits = 13, kCsBias = 2048, kCsPair = 2048;

template <int NW, int RT>
__device__ __forceinline__ void osd_cs_epilogue(const OsdArgs& a, const uint64_t (&R)[RT][NW], const bool (&own)[RT],
                                                const int (&mypos)[RT], int nJ, const int* Jl,
                                                const unsigned char* inJ, const uint64_t* emask, uint64_t* region,
                                                const int32_t* perm, uint8_t* ehat) {
  const int n = a.n, t = threadIdx.x, B = blockDim.x, lane = t & 63;
  const int nwaves = B >> 6, wave = __builtin_amdgcn_readfirstlane(t >> 6), Q = RT * nwaves;
  const int L = min(a.cs_lambda, n - nJ);
  uint64_t* colv = region;
  uint64_t* ejm = colv + 64 * Q;
  uint64_t* tmask = ejm + Q;
  int* cnt = (int*)(tmask + NW);
  int* tl = cnt + 64 * NW;
  int* red = tl + 64;

  // e0_J: the k-th pivot row gives entry k, as the order-0 epilogue
  bool piv[RT];
  uint32_t ej[RT];
  uint64_t ejb[RT];
#pragma unroll
  for (int h = 0; h < RT; ++h) {
    piv[h] = own[h] && mypos[h] < nJ;
    uint64_t acc = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w == (n >> 6)) acc ^= (R[h][w] >> (n & 63)) & 1ull;
      acc ^= (uint64_t)(__builtin_popcountll(R[h][w] & emask[w]) & 1);
    }
    ej[h] = piv[h] ? (uint32_t)(acc & 1ull) : 0u;
    ejb[h] = __ballot(ej[h] != 0);
    if (lane == 0) ejm[h * nwaves + wave] = ejb[h];
  }
  for (int i0w = 64 * wave; i0w < 64 * NW; i0w += B) {
    const int i = i0w + lane;
    const uint64_t bits = __ballot(i < n && !inJ[i]);
    if (lane == 0) tmask[i0w >> 6] = bits;
  }
  for (int i = t; i < 64 * NW; i += B) cnt[i] = 0;
  if (t == 0) red[0] = kCsBias << kCsIdxBits;         // e0: cost change 0, index 0
  __syncthreads();

  // every T column's sum into cnt, the first L columns' ballots into colv
  int k = 0;
  for (int w = 0; w < NW && 64 * w < n; ++w) {
    uint64_t rw[RT];
#pragma unroll
    for (int h = 0; h < RT; ++h) {
      uint64_t v = 0;
#pragma unroll
      for (int x = 0; x < NW; ++x)
        if (x == w) v = R[h][x];
      rw[h] = piv[h] ? v : 0ull;
    }
    const uint64_t tm = tmask[w];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      uint32_t bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tm >> (32 * half)));
      uint32_t r32[RT];
#pragma unroll
      for (int h = 0; h < RT; ++h) r32[h] = (uint32_t)(rw[h] >> (32 * half));
      while (bits) {
        bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)bits);
        k = __builtin_amdgcn_readfirstlane(k);
        const int b = (int)__builtin_ctz(bits);
        bits &= bits - 1;
        const int c = 64 * w + 32 * half + b;
        int d = 0;
#pragma unroll
        for (int h = 0; h < RT; ++h) {
          const uint64_t bal = __ballot(((r32[h] >> b) & 1u) != 0);
          d += __builtin_popcountll(bal) - 2 * __builtin_popcountll(bal & ejb[h]);
          if (k < L && lane == 0) colv[k * Q + h * nwaves + wave] = bal;
        }
        if (lane == 0 && d != 0) atomicAdd(&cnt[c], d);
        if (k < L && t == 0) tl[k] = c;
        ++k;
      }
    }
  }
  __syncthreads();

  auto flip_cost = [&](int c) { return ((emask[c >> 6] >> (c & 63)) & 1ull) ? -1 : 1; };
  int best = 0x7fffffff;
  for (int c = t; c < n; c += B)
    if (!inJ[c]) best = min(best, ((cnt[c] + flip_cost(c) + kCsBias) << kCsIdxBits) | (1 + c));
  for (int idx = t; idx < 64 * L; idx += B) {
    const int pa = idx >> 6, pb = idx & 63;
    if (pa < pb && pb < L) {
      int d = flip_cost(tl[pa]) + flip_cost(tl[pb]);
      for (int q = 0; q < Q; ++q) {
        const uint64_t x = colv[pa * Q + q] ^ colv[pb * Q + q];
        d += __builtin_popcountll(x) - 2 * __builtin_popcountll(x & ejm[q]);
      }
      best = min(best, ((d + kCsBias) << kCsIdxBits) | (kCsPair + idx));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
  if (lane == 0) atomicMin(&red[0], best);
  __syncthreads();

  // the winner's columns into e0_J (pivot rows), its T flips into e_hat
  const int idx = red[0] & ((1 << kCsIdxBits) - 1);
  int c1 = -1, c2 = -1;
  if (idx >= kCsPair) {
    c1 = tl[(idx - kCsPair) >> 6];
    c2 = tl[(idx - kCsPair) & 63];
  } else if (idx > 0) {
    c1 = idx - 1;
  }
#pragma unroll
  for (int h = 0; h < RT; ++h)
    if (piv[h]) {
      uint64_t v1 = 0, v2 = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (c1 >= 0 && w == (c1 >> 6)) v1 = R[h][w];
        if (c2 >= 0 && w == (c2 >> 6)) v2 = R[h][w];
      }
      const uint32_t e = ej[h] ^ (c1 >= 0 ? (uint32_t)(v1 >> (c1 & 63)) & 1u : 0u) ^
                         (c2 >= 0 ? (uint32_t)(v2 >> (c2 & 63)) & 1u : 0u);
      ehat[perm[Jl[mypos[h]]]] = (uint8_t)e;
    }
  if (t == 0) {
    if (c1 >= 0) ehat[perm[c1]] ^= 1;
    if (c2 >= 0) ehat[perm[c2]] ^= 1;
  }
}

// ---------------------------------------------------------------------------
// OSD-CS epilogue with the prior-weighted cost: the same
// candidates, order and index coding as osd_cs_epilogue; the cost of an
// estimate is the sum of w over its support, w = a.cs_w by original column
// (llrint(L 2^20), |w| < 2^30, negative where p > 1/2). Pivot row r carries its
// signed weight sw_r = w[perm[J[r]]] (1 - 2 e0_J[r]) (0 for rows without
// pivot): the cost change of a flip set is the flips' own signed weights plus
// the sum of sw_r over the set bits r of x = the XOR of its columns.
//
// A column's sum: each lane adds sw of its rows that hold a 1, split as
// sw = hi 2^21 + lo (0 <= lo < 2^21, |hi| < 2^9) so that a wave's sums of 128
// terms fit 32 bits; two DPP wave sums, joined to one int64 that lane 0 adds
// to the column's LDS counter. A pair's sum over the XOR of its two stored
// columns is their two counters less twice the sum of sw over the set bits of
// their AND. The key is (cost change + 2^42) << 13 | index: the
// change is below 2^41 in magnitude (1088 columns of |w| < 2^30), 64 bits,
// unsigned order = order of (cost, index).
//
// LDS (osd_cs_prior_lds bytes of osd_block_cs_room):
//   colv [64][Q] u64 | cnt [64 NW] i64 | tmask [NW] u64 | red [2] u64 | sw [MR] i32 | tl [64] i32
// ---------------------------------------------------------------------------
constexpr int kCswSplit = 21, kCswBiasLog = 42;

// sum over the wave (every lane active), wave-uniform
__device__ __forceinline__ int wave_sum32(int x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
  x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
  x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xf, 0xf, false);   // row_half_mirror
  x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xf, 0xf, false);   // row_mirror
  return __builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) + __builtin_amdgcn_readlane(x, 32) +
         __builtin_amdgcn_readlane(x, 48);
}

template <int NW, int RT>
__device__ __forceinline__ void osd_cs_prior_epilogue(const OsdArgs& a, const uint64_t (&R)[RT][NW],
                                                      const bool (&own)[RT], const int (&mypos)[RT], int nJ,
                                                      const int* Jl, const unsigned char* inJ, const uint64_t* emask,
                                                      uint64_t* region, const int32_t* perm, uint8_t* ehat) {
  const int n = a.n, t = threadIdx.x, B = blockDim.x, lane = t & 63;
  const int nwaves = B >> 6, wave = __builtin_amdgcn_readfirstlane(t >> 6), Q = RT * nwaves;
  const int L = min(a.cs_lambda, n - nJ);
  uint64_t* colv = region;
  unsigned long long* cnt = (unsigned long long*)(colv + 64 * Q);   // int64 sums, two's complement
  uint64_t* tmask = (uint64_t*)(cnt + 64 * NW);
  unsigned long long* red = (unsigned long long*)(tmask + NW);
  int* sw = (int*)(red + 2);                          // [MR], row t + h B at that index = bit of colv's word
  int* tl = sw + RT * B;
  const int64_t* wcol = a.cs_w;

  // e0_J as the order-0 epilogue, and each pivot row's signed weight
  bool piv[RT];
  uint32_t ej[RT];
  int swlo[RT], swhi[RT];
#pragma unroll
  for (int h = 0; h < RT; ++h) {
    piv[h] = own[h] && mypos[h] < nJ;
    uint64_t acc = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w == (n >> 6)) acc ^= (R[h][w] >> (n & 63)) & 1ull;
      acc ^= (uint64_t)(__builtin_popcountll(R[h][w] & emask[w]) & 1);
    }
    ej[h] = piv[h] ? (uint32_t)(acc & 1ull) : 0u;
    int s = 0;
    if (piv[h]) {
      const int wj = (int)wcol[perm[Jl[mypos[h]]]];
      s = ej[h] ? -wj : wj;
    }
    sw[t + h * B] = s;
    swlo[h] = s & ((1 << kCswSplit) - 1);
    swhi[h] = s >> kCswSplit;                         // (arithmetic: s = swhi 2^21 + swlo)
  }
  for (int i0w = 64 * wave; i0w < 64 * NW; i0w += B) {
    const int i = i0w + lane;
    const uint64_t bits = __ballot(i < n && !inJ[i]);
    if (lane == 0) tmask[i0w >> 6] = bits;
  }
  for (int i = t; i < 64 * NW; i += B) cnt[i] = 0ull;
  if (t == 0) red[0] = 1ull << (kCswBiasLog + kCsIdxBits);   // e0: cost change 0, index 0
  __syncthreads();

  // every T column's sum into cnt, the first L columns' ballots into colv
  int k = 0;
  for (int w = 0; w < NW && 64 * w < n; ++w) {
    uint64_t rw[RT];
#pragma unroll
    for (int h = 0; h < RT; ++h) {
      uint64_t v = 0;
#pragma unroll
      for (int x = 0; x < NW; ++x)
        if (x == w) v = R[h][x];
      rw[h] = piv[h] ? v : 0ull;
    }
    const uint64_t tm = tmask[w];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      uint32_t bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(tm >> (32 * half)));
      uint32_t r32[RT];
#pragma unroll
      for (int h = 0; h < RT; ++h) r32[h] = (uint32_t)(rw[h] >> (32 * half));
      while (bits) {
        bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)bits);
        k = __builtin_amdgcn_readfirstlane(k);
        const int b = (int)__builtin_ctz(bits);
        bits &= bits - 1;
        const int c = 64 * w + 32 * half + b;
        int lo = 0, hi = 0;
#pragma unroll
        for (int h = 0; h < RT; ++h) {
          const int mk = __builtin_amdgcn_sbfe((int)r32[h], b, 1);   // 0 / -1
          lo += swlo[h] & mk;
          hi += swhi[h] & mk;
          if (k < L) {
            const uint64_t bal = __ballot(mk != 0);
            if (lane == 0) colv[k * Q + h * nwaves + wave] = bal;
          }
        }
        const int slo = wave_sum32(lo), shi = wave_sum32(hi);
        // (the two halves join here, after the lanes: no 64-bit value crosses them)
        const long long d = (long long)shi * (1ll << kCswSplit) + (long long)slo;
        if (lane == 0 && d != 0) atomicAdd(&cnt[c], (unsigned long long)d);
        if (k < L && t == 0) tl[k] = c;
        ++k;
      }
    }
  }
  __syncthreads();

  auto flip_cost = [&](int c) {
    const long long wc = (long long)wcol[perm[c]];
    return ((emask[c >> 6] >> (c & 63)) & 1ull) ? -wc : wc;
  };
  auto key_of = [](long long d, int idx) {
    return ((unsigned long long)(d + (1ll << kCswBiasLog)) << kCsIdxBits) | (unsigned long long)idx;
  };
  unsigned long long best = ~0ull;
  for (int c = t; c < n; c += B)
    if (!inJ[c]) best = min(best, key_of((long long)cnt[c] + flip_cost(c), 1 + c));
  for (int idx = t; idx < 64 * L; idx += B) {
    const int pa = idx >> 6, pb = idx & 63;
    if (pa < pb && pb < L) {
      // sum of sw over a ^ b = the two columns' sums less twice the sum over a & b (fewer set bits to walk
      // than a ^ b while the columns are less than 2/3 full)
      const int ca = tl[pa], cb = tl[pb];
      long long both = 0;
      for (int q = 0; q < Q; ++q) {
        uint64_t x = colv[pa * Q + q] & colv[pb * Q + q];
        // (word q's bit j is row slot 64 q + j: q = h nwaves + wave, j = lane)
        while (x) {
          both += (long long)sw[64 * q + (int)__builtin_ctzll(x)];
          x &= x - 1;
        }
      }
      const long long d = flip_cost(ca) + flip_cost(cb) + (long long)cnt[ca] + (long long)cnt[cb] - 2 * both;
      best = min(best, key_of(d, kCsPair + idx));
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)best, off, 64);
    const uint32_t ohi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), off, 64);
    best = min(best, ((unsigned long long)ohi << 32) | olo);
  }
  if (lane == 0) atomicMin(&red[0], best);
  __syncthreads();

  // the winner's columns into e0_J (pivot rows), its T flips into e_hat
  const int idx = (int)(red[0] & ((1ull << kCsIdxBits) - 1));
  int c1 = -1, c2 = -1;
  if (idx >= kCsPair) {
    c1 = tl[(idx - kCsPair) >> 6];
    c2 = tl[(idx - kCsPair) & 63];
  } else if (idx > 0) {
    c1 = idx - 1;
  }
#pragma unroll
  for (int h = 0; h < RT; ++h)
    if (piv[h]) {
      uint64_t v1 = 0, v2 = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        if (c1 >= 0 && w == (c1 >> 6)) v1 = R[h][w];
        if (c2 >= 0 && w == (c2 >> 6)) v2 = R[h][w];
      }
      const uint32_t e = ej[h] ^ (c1 >= 0 ? (uint32_t)(v1 >> (c1 & 63)) & 1u : 0u) ^
                         (c2 >= 0 ? (uint32_t)(v2 >> (c2 & 63)) & 1u : 0u);
      ehat[perm[Jl[mypos[h]]]] = (uint8_t)e;
    }
  if (t == 0) {
    if (c1 >= 0) ehat[perm[c1]] ^= 1;
    if (c2 >= 0) ehat[perm[c2]] ^= 1;
  }
}

// SL = rows per wave-0 lane (m <= 64 SL), sized to the code so the state stays
// in VGPRs; RT = rows per thread (thread t holds rows t, t + blockDim, ..):
// with 2, a 450-row shot takes 4 waves and a CU holds 4 shots (4 engines, one
// per SIMD) instead of 2
template <int NW, int SL, int RT>
__global__ void __launch_bounds__(64 * SL / RT) __attribute__((amdgpu_waves_per_eu(RT == 2 ? QLDPC_OSD_WPE : 1))) osd_block_kernel(OsdArgs a) {
#define QLDPC_OSD_BLOCK_CS 0
#include "osd_block_body.inc"
#undef QLDPC_OSD_BLOCK_CS
}

// the same elimination, finished by the OSD-CS epilogue (osd_cs_epilogue)
template <int NW, int SL, int RT>
__global__ void __launch_bounds__(64 * SL / RT) __attribute__((amdgpu_waves_per_eu(RT == 2 ? QLDPC_OSD_WPE : 1))) osd_block_cs_kernel(OsdArgs a) {
#define QLDPC_OSD_BLOCK_CS 1
#include "osd_block_body.inc"
#undef QLDPC_OSD_BLOCK_CS
}

// and by the OSD-CS epilogue with the prior-weighted cost (osd_cs_prior_epilogue)
template <int NW, int SL, int RT>
__global__ void __launch_bounds__(64 * SL / RT) __attribute__((amdgpu_waves_per_eu(RT == 2 ? QLDPC_OSD_WPE : 1))) osd_block_cs_prior_kernel(OsdArgs a) {
#define QLDPC_OSD_BLOCK_CS 2
#include "osd_block_body.inc"
#undef QLDPC_OSD_BLOCK_CS
}

}  // namespace qldpc
