// osd_kernels.hip — batched OSD post-decoding on MI355X (gfx950).
//
// Replaces OSDdec (qLDPCsim/decoders.py:299-370) with its gf2math.rank /
// gf2math.REF calls (gf2math.py:91-187) for a batch of non-converged shots.
// One workgroup = one shot; thread t owns row t of the column-permuted matrix
// Hp = H[:, perm] (perm = the reliability order, computed by the caller with
// NumPy exactly as decoders.py:320-325), held bit-packed in VGPRs, with the
// syndrome as an augmented column.
//
// Equivalences used (OSD):
//  * Gaussian elimination over the columns of Hp in order, pivot = first row at
//    or below the current pivot row holding a 1 (gf2math.REF's rule), finds a
//    pivot exactly in the columns that raise the rank — the greedy
//    complementary information set J of decoders.py:329-342 (plus column 0,
//    which the reference takes unconditionally).
//  * Non-pivot columns cause no row operation, so the row operations equal
//    those of REF(Hp[:, J], reduced=True); applied to the augmented syndrome
//    they give T @ s. With R = T @ Hp: T @ sJ = T @ s + R[:, I] @ e_I (mod 2),
//    so e_J = (T @ sJ)[:|J|] (decoders.py:352-358) needs one elimination.
//  * Order semantics with the reference's aliasing: order 1
//    flips e_perm[infoSet[0]] (CPython set order, emulated), order >= 2 is
//    order 0.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "osd_kernels.h"
#include "tuning.h"
#include "../../include/qldpc_libm.h"

namespace qldpc {

__device__ int first_setdiff(int n, const unsigned char* inJ, int nJ, int* table);

// a status-2 shot's posterior row into the spill buffer (OsdArgs), whole
// workgroup; `slot` is an LDS int the block may overwrite
__device__ __forceinline__ void spill_shot(const OsdArgs& a, long long shot, int n, int* slot) {
  if (!a.spill_count) return;
  if (threadIdx.x == 0) *slot = atomicAdd(a.spill_count, 1);
  __syncthreads();
  const long long q = *slot;
  if (q >= a.spill_cap) return;
  const double* src = a.post + shot * (long long)n;
  double* dst = a.spill_post + q * (long long)n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
  if (threadIdx.x == 0) a.spill_idx[q] = (int32_t)(a.shot_base + shot);
}

// Shots whose reliability order the device leaves to NumPy on the host
// (osd_order_kernel's tiepos -1: a NaN posterior, or x86-simd-sort's
// std::sort fallback): status 2, posteriors spilled, before any elimination.
__device__ __forceinline__ bool osd_host_shot(const OsdArgs& a, long long shot, int n, int* slot) {
  if (!a.tiepos || a.tiepos[shot] >= 0) return false;        // uniform per workgroup
  if (threadIdx.x == 0) a.status[shot] = 2;
  spill_shot(a, shot, n, slot);
  return true;
}

// s_getreg immediates: (size - 1) << 11 | offset << 6 | register id
constexpr int kHwRegHwId = (31 << 11) | 4;    // HW_ID: SIMD bits 4-5, CU 8-11, SH 12, SE 13-15
constexpr int kHwRegXccId = (31 << 11) | 20;  // XCC_ID: bits 0-3

template <int NW>
__global__ void __launch_bounds__(1024) osd_kernel(OsdArgs a) {
  // LDS: inv_perm[n] | J list [m+2] | inJ bytes [n] | emask [NW] u64 |
  //      candidate rows [2][16][NW] | xrow rows [2][NW] | candidate ids [2][16] |
  //      misc [4] | set table
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int m = a.m, n = a.n;
  int* inv = (int*)lds;
  int* Jl = inv + n;
  unsigned char* inJ = (unsigned char*)(Jl + m + 2);
  // offsets from `lds` itself (a cast through an integer would turn every
  // access below into a generic flat access instead of ds_read / ds_write)
  uint64_t* emask = (uint64_t*)(lds + ((4 * (n + m + 2) + n + 15) & ~15));
  uint64_t* cbuf = emask + NW;                     // [2][16][NW]
  uint64_t* xbuf = cbuf + 2 * 16 * NW;             // [2][NW]
  int* slots = (int*)(xbuf + 2 * NW);              // [2][16]
  int* misc = slots + 32;                          // [0]=|J| [1]=status [2]=first info index
  int* table = misc + 4;                           // CPython set emulation (order 1)

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6, nwaves = blockDim.x >> 6;
  const long long shot = blockIdx.x;
  if (a.redo && a.status[shot] != 3) return;       // second pass after osd_block_kernel
  if (!a.redo && osd_host_shot(a, shot, n, slots)) return;
  const int32_t* perm = a.perm + shot * (long long)n;
  const uint8_t* syn = a.syn + shot * (long long)m;
  uint8_t* ehat = a.ehat + shot * (long long)n;

  for (int i = t; i < n; i += blockDim.x) {
    inv[perm[i]] = i;
    inJ[i] = 0;
  }
  __syncthreads();

  // my row of Hp (+ syndrome bit at column n); thread t holds the row at
  // position t of REF's current row order (rows move by REF's swaps)
  uint64_t R[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) R[w] = 0;
  const bool own = t < m;
  if (own) {
    for (int e = a.row_ptr[t]; e < a.row_ptr[t + 1]; ++e) {
      const int i = inv[a.col_idx[e]];
#pragma unroll
      for (int w = 0; w < NW; ++w)
        if ((i >> 6) == w) R[w] |= 1ull << (i & 63);
    }
    if (syn[t] & 1) {
#pragma unroll
      for (int w = 0; w < NW; ++w)
        if ((n >> 6) == w) R[w] |= 1ull << (n & 63);
    }
  }

  int xrow = 0, rank = 0, nJ = 0, step = 0;
  bool done = a.rank == 0;                          // rank(H) = 0: IndexError below
  if (t == 0) {
    Jl[0] = 0;                                      // column 0 always (decoders.py:329)
    inJ[0] = 1;
  }
  nJ = 1;
  // One workgroup barrier per column. Before it, each wave's first candidate
  // row (a 1 in column i at a position >= xrow) and the row at position xrow
  // publish their words >= w; after it, every thread knows the pivot (the
  // smallest candidate position: REF's "first row at or below") and reads its
  // row from the winning wave's slot. Rows at positions >= xrow are zero in
  // every column < i (a nonzero there would have been a pivot), so words < w
  // never need to move. Two slot sets alternate: a wave writing set s at
  // column k+2 has passed column k+1's barrier, which every reader of column
  // k's set s had reached after its reads.
  // Fully unrolled over the NW words, so every R[w] / R[q] index is a
  // compile-time constant and the row stays in VGPRs (a runtime word index
  // would put R in scratch memory: one global access per touch).
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    if (done || 64 * w >= n) continue;
    for (int b = 0; b < 64; ++b) {
      const int i = 64 * w + b;
      if (i >= n || done) break;
      const bool has = own && ((R[w] >> b) & 1ull);
      const uint64_t bal = __ballot(has && t >= xrow);
      const int set = step & 1;
      uint64_t* cb = cbuf + (set * 16 + wave) * NW;
      uint64_t* xb = xbuf + set * NW;
      int* sl = slots + 16 * set;
      if (bal) {
        if (lane == __builtin_ctzll(bal)) {
#pragma unroll
          for (int q = w; q < NW; ++q) cb[q] = R[q];
          sl[wave] = t;
        }
      } else if (lane == 0) {
        sl[wave] = 0x7fffffff;
      }
      if (t == xrow) {
#pragma unroll
        for (int q = w; q < NW; ++q) xb[q] = R[q];
      }
      __syncthreads();
      int piv = 0x7fffffff;
      for (int q = 0; q < nwaves; ++q) piv = min(piv, sl[q]);
      ++step;
      if (piv == 0x7fffffff) continue;              // dependent column: not in J
      // pivot row `piv` moves to position xrow (REF's row swap), then every
      // other row holding a 1 in column i is XOR-ed with it (below and above)
      const uint64_t* pr = cbuf + (set * 16 + (piv >> 6)) * NW;
      if (t == piv && piv != xrow) {
#pragma unroll
        for (int q = w; q < NW; ++q) R[q] = xb[q];   // old row xrow: 0 in column i
      } else if (t == xrow) {
#pragma unroll
        for (int q = w; q < NW; ++q) R[q] = pr[q];
      } else if (has) {
#pragma unroll
        for (int q = w; q < NW; ++q) R[q] ^= pr[q];  // pivot row is 0 left of column i
      }
      if (i != 0) {
        if (t == 0) {
          Jl[nJ] = i;
          inJ[i] = 1;
        }
        ++nJ;
      }
      ++xrow;
      ++rank;
      if (rank >= a.rank || xrow >= m) done = true;
      if (i == 0 && done) rank = -1;                // column 0 alone reaches rank(H): the
    }                                               // greedy loop never breaks (:333-342)
  }
  if (rank < a.rank) {                              // greedy loop runs past column n-1
    if (t == 0) a.status[shot] = 1;                 // (the reference raises IndexError)
    return;
  }
  __syncthreads();
  // information-set values e_I (e_perm = e_hat[perm], decoders.py:345):
  // one column per thread, words assembled by ballots (all loads in flight)
  for (int i0w = 64 * wave; i0w < 64 * NW; i0w += blockDim.x) {
    const int i = i0w + lane;
    const bool bit = i < n && !inJ[i] && (ehat[perm[i]] & 1);
    const uint64_t bits = __ballot(bit);
    if (lane == 0) emask[i0w >> 6] = bits;
  }
  if (t == 0) {
    int i0 = -1;
    if (a.order == 1 && nJ < n) {
      // first element of CPython's set(range(n)) - set(J) (decoders.py:344)
      i0 = first_setdiff(n, inJ, nJ, table);
    }
    misc[2] = i0;
  }
  __syncthreads();
  const int i0 = misc[2];
  if (t == 0 && i0 >= 0) emask[i0 >> 6] ^= 1ull << (i0 & 63);  // order-1 flip (:349-350)
  __syncthreads();
  // e_J = (T sJ)[:|J|], T sJ = T s + R[:, I] e_I (mod 2)   (decoders.py:352-358)
  if (own && t < nJ) {
    uint64_t acc = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w == (n >> 6)) acc ^= (R[w] >> (n & 63)) & 1ull;      // T s (augmented column)
      acc ^= (uint64_t)(__builtin_popcountll(R[w] & emask[w]) & 1);
    }
    ehat[perm[Jl[t]]] = (uint8_t)(acc & 1ull);                // e_hat[perm] = ... (:368)
  }
  if (t == 0)                                                  // (J past T sJ's m rows: 0, as
    for (int p = m; p < nJ; ++p) ehat[perm[Jl[p]]] = 0;        // the host OSD; osd_hbm_kernel)
  if (t == 0 && i0 >= 0) ehat[perm[i0]] ^= 1;
  if (t == 0) a.status[shot] = 0;
}

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
// with Q = MR / 64 words per column: 8 MR + MR / 8 + 264 NW + 272 bytes of the
// region's 16 MR + 512 NW + 512 at least (osd_cs_lds, checked by the launcher).
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

size_t osd_order_lds(int n) { return (size_t)8 * n + 96 * 4 + 512 * 2 + 16; }

hipError_t launch_osd_order(const OrderArgs& a, long long count, hipStream_t stream) {
  const void* k = a.n <= 256 ? (const void*)&osd_order_kernel<4>
                : a.n <= 512 ? (const void*)&osd_order_kernel<8>
                : a.n <= 1024 ? (const void*)&osd_order_kernel<16>
                : (const void*)&osd_order_kernel<32>;
  long long done = 0;
  while (done < count) {
    const long long g = count - done < (1ll << 30) ? count - done : (1ll << 30);
    OrderArgs ai = a;
    ai.post = a.post + done * a.n;
    ai.perm = a.perm + done * a.n;
    ai.tiepos = a.tiepos + done;
    void* params[] = {(void*)&ai};
    hipError_t e = hipLaunchKernel(k, dim3((unsigned)g), dim3(64), params, osd_order_lds(a.n), stream);
    if (e != hipSuccess) return e;
    done += g;
  }
  return hipSuccess;
}

// CPython setobject.c emulation (set_difference -> set_add_entry with
// resize; LINEAR_PROBES 9, PERTURB_SHIFT 5) for small-int keys, one thread.
__device__ int first_setdiff(int n, const unsigned char* inJ, int nJ, int* table) {
  if ((n >> 2) > nJ) {
    for (int i = 0; i < n; ++i)
      if (!inJ[i]) return i;
    return -1;
  }
  unsigned mask = 7, fill = 0, used = 0;
  for (unsigned s = 0; s <= mask; ++s) table[s] = -1;
  for (int key = 0; key < n; ++key) {
    if (inJ[key]) continue;
    unsigned perturb = (unsigned)key, i = (unsigned)key & mask;
    while (true) {
      unsigned probes = (i + 9 <= mask) ? 9 : 0, k = i;
      bool placed = false;
      while (true) {
        if (table[k] < 0) { table[k] = key; placed = true; break; }
        if (probes-- == 0) break;
        ++k;
      }
      if (placed) break;
      perturb >>= 5;
      i = (i * 5 + 1 + perturb) & mask;
    }
    ++fill;
    ++used;
    if (fill * 5 >= mask * 3) {
      const unsigned minused = used > 50000 ? used * 2 : used * 4;
      unsigned newsize = 8;
      while (newsize <= minused) newsize <<= 1;
      // re-insert (old table order) into the new one: copy old entries to the
      // upper half of the scratch first (newsize > 2*(mask+1) always here)
      int* old = table + newsize;
      for (unsigned s = 0; s <= mask; ++s) old[s] = table[s];
      for (unsigned s = 0; s < newsize; ++s) table[s] = -1;
      const unsigned nmask = newsize - 1;
      for (unsigned s = 0; s <= mask; ++s) {
        const int kk = old[s];
        if (kk < 0) continue;
        unsigned pt = (unsigned)kk, j = (unsigned)kk & nmask;
        while (true) {
          if (table[j] < 0) { table[j] = kk; break; }
          bool ok = false;
          if (j + 9 <= nmask) {
            for (int q = 0; q < 9; ++q) {
              ++j;
              if (table[j] < 0) { table[j] = kk; ok = true; break; }
            }
          }
          if (ok) break;
          pt >>= 5;
          j = (j * 5 + 1 + pt) & nmask;
        }
      }
      mask = nmask;
    }
  }
  for (unsigned s = 0; s <= mask; ++s)
    if (table[s] >= 0) return table[s];
  return -1;
}

const void* select_osd_kernel(int nw) {
  if (nw <= 0) return nullptr;                      // (osd_nw_of: more than 33 words)
  if (nw <= 4) return (const void*)&osd_kernel<4>;
  if (nw <= 9) return (const void*)&osd_kernel<9>;
  if (nw <= 17) return (const void*)&osd_kernel<17>;
  if (nw <= 33) return (const void*)&osd_kernel<33>;
  return nullptr;
}

// ---------------------------------------------------------------------------
// OSD for codes past the register / LDS kernels (m > 1024 rows, or more than
// 33 row words: n > 2111): osd_kernel's exact-REF column protocol with the
// working matrix in a per-shot global scratch slice (OsdHbmArgs). Thread t
// owns the REF row positions t, t + B, ...; the current word of every row is
// cached in LDS (cw), so the pivot search and the "holds a 1" tests never
// touch global memory; a pivot's words w.. are staged in LDS (prow, and the
// row it displaces in xr), and every row holding a 1 in the column XORs them
// into its words w.. in global memory (word-major, so a word of consecutive
// positions is contiguous). Per column: the pivot is the first position >=
// xrow holding a 1 (REF, gf2math.py:139-187), rows below and above are
// reduced, J and e_J as in osd_kernel (decoders.py:329-368). Two workgroup
// barriers per pivot column, one per dependent column.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) osd_hbm_kernel(OsdArgs a, OsdHbmArgs h) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int m = a.m, n = a.n, NWr = h.nwr, MP = h.mp;
  uint64_t* cw = (uint64_t*)lds;                       // [MP] word w of each row position
  uint64_t* prow = cw + MP;                            // [NWr] the pivot row
  uint64_t* xr = prow + NWr;                           // [NWr] the row the pivot displaces
  uint64_t* emask = xr + NWr;                          // [NWr] e_I bits (decoders.py:345)
  int* slots = (int*)(emask + NWr);                    // [2][16] per-wave candidates
  int* misc = slots + 32;
  const int t = threadIdx.x, B = blockDim.x, lane = t & 63, wave = t >> 6, nwaves = B >> 6;
  const long long shot = blockIdx.x;
  if (osd_host_shot(a, shot, n, slots)) return;
  unsigned char* base = h.scratch + (size_t)shot * (size_t)h.stride;
  uint64_t* R = (uint64_t*)base;
  int* inv = (int*)(base + h.off_inv);
  int* Jl = (int*)(base + h.off_jl);
  unsigned char* inJ = base + h.off_inj;
  int* table = (int*)(base + h.off_table);
  const int32_t* perm = a.perm + shot * (long long)n;
  const uint8_t* syn = a.syn + shot * (long long)m;
  uint8_t* ehat = a.ehat + shot * (long long)n;
  auto word = [&](int q, int p) -> uint64_t& { return R[(size_t)q * MP + p]; };

  for (int i = t; i < n; i += B) {
    inv[perm[i]] = i;
    inJ[i] = 0;
  }
  for (size_t x = t; x < (size_t)NWr * MP; x += B) R[x] = 0;
  __syncthreads();
  // Hp's rows (+ the syndrome bit at column n); row r starts at position r
  for (int r = t; r < m; r += B) {
    for (int e = a.row_ptr[r]; e < a.row_ptr[r + 1]; ++e) {
      const int i = inv[a.col_idx[e]];
      word(i >> 6, r) |= 1ull << (i & 63);
    }
    if (syn[r] & 1) word(n >> 6, r) |= 1ull << (n & 63);
  }
  int xrow = 0, rank = 0, nJ = 1, step = 0;
  bool done = a.rank == 0;                              // rank(H) = 0: IndexError below
  if (t == 0) {
    Jl[0] = 0;                                          // column 0 always (decoders.py:329)
    inJ[0] = 1;
  }
  const int K = (m + B - 1) / B;
  for (int w = 0; w < NWr && 64 * w < n && !done; ++w) {
    __syncthreads();                                    // (the previous word's last pivot applied)
    for (int p = t; p < m; p += B) cw[p] = word(w, p);
    for (int b = 0; b < 64; ++b) {
      const int i = 64 * w + b;
      if (i >= n || done) break;
      // the first position >= xrow holding a 1 in column i: per wave, the
      // lowest hit of the lowest position round that has one
      int cand = 0x7fffffff;
      for (int k = 0; k < K; ++k) {
        const int p = t + k * B;
        const uint64_t bal = __ballot(p < m && p >= xrow && ((cw[p] >> b) & 1ull));
        if (bal) {
          cand = k * B + 64 * wave + __builtin_ctzll(bal);
          break;
        }
      }
      // two slot sets alternate (a wave writing set s at column k + 2 has
      // passed column k + 1's barrier, after every read of column k's set s)
      const int set = step & 1;
      if (lane == 0) slots[16 * set + wave] = cand;
      __syncthreads();
      int piv = 0x7fffffff;
      for (int q = 0; q < nwaves; ++q) piv = min(piv, slots[16 * set + q]);
      ++step;
      if (piv == 0x7fffffff) continue;                // dependent column: not in J
      for (int q = w + t; q < NWr; q += B) {
        prow[q] = word(q, piv);
        xr[q] = word(q, xrow);
      }
      __syncthreads();
      // the pivot row moves to position xrow (REF's swap; the row it
      // displaces has a 0 in column i), every other row holding a 1 in
      // column i takes it, below and above (rows at positions >= xrow are 0
      // left of column i, and so is the pivot row: words < w never change)
      for (int p = t; p < m; p += B) {
        const uint64_t c = cw[p];
        if (p == piv && piv != xrow) {
          for (int q = w; q < NWr; ++q) word(q, p) = xr[q];
          cw[p] = xr[w];
        } else if (p == xrow) {
          for (int q = w; q < NWr; ++q) word(q, p) = prow[q];
          cw[p] = prow[w];
        } else if ((c >> b) & 1ull) {
          for (int q = w; q < NWr; ++q) word(q, p) ^= prow[q];
          cw[p] = c ^ prow[w];
        }
      }
      if (i != 0) {
        if (t == 0) {
          Jl[nJ] = i;
          inJ[i] = 1;
        }
        ++nJ;
      }
      ++xrow;
      ++rank;
      if (rank >= a.rank || xrow >= m) done = true;
      if (i == 0 && done) rank = -1;                  // column 0 alone reaches rank(H): the
    }                                                 // greedy loop never breaks (:333-342)
  }
  if (rank < a.rank) {                                // greedy loop runs past column n-1
    if (t == 0) a.status[shot] = 1;                   // (the reference raises IndexError)
    return;
  }
  __syncthreads();
  // information-set values e_I (e_perm = e_hat[perm], decoders.py:345)
  for (int i0w = 64 * wave; i0w < 64 * NWr; i0w += B) {
    const int i = i0w + lane;
    const bool bit = i < n && !inJ[i] && (ehat[perm[i]] & 1);
    const uint64_t bits = __ballot(bit);
    if (lane == 0) emask[i0w >> 6] = bits;
  }
  if (t == 0) {
    int i0 = -1;
    if (a.order == 1 && nJ < n) i0 = first_setdiff(n, inJ, nJ, table);   // (decoders.py:344)
    misc[2] = i0;
  }
  __syncthreads();
  const int i0 = misc[2];
  if (t == 0 && i0 >= 0) emask[i0 >> 6] ^= 1ull << (i0 & 63);  // order-1 flip (:349-350)
  __syncthreads();
  // e_J = (T sJ)[:|J|], T sJ = T s + R[:, I] e_I (mod 2)   (decoders.py:352-358)
  for (int p = t; p < nJ && p < m; p += B) {
    uint64_t acc = (word(n >> 6, p) >> (n & 63)) & 1ull;   // T s (augmented column)
    for (int q = 0; q < NWr; ++q) acc ^= (uint64_t)(__builtin_popcountll(word(q, p) & emask[q]) & 1);
    ehat[perm[Jl[p]]] = (uint8_t)(acc & 1ull);            // e_hat[perm] = ... (:368)
  }
  // an all-zero column 0 with rank(H) = m: J holds m + 1 entries, one more
  // than T sJ has rows (the reference's assignment fails to broadcast); the
  // host OSD writes 0 there, and so does this kernel
  if (t == 0)
    for (int p = m; p < nJ; ++p) ehat[perm[Jl[p]]] = 0;
  if (t == 0 && i0 >= 0) ehat[perm[i0]] ^= 1;
  if (t == 0) a.status[shot] = 0;
}

const void* osd_hbm_kernel_ptr() { return (const void*)&osd_hbm_kernel; }

template <int NW, bool CS>
static const void* osd_block_by_rows(int m, int* rt) {
  *rt = m <= 256 ? 1 : 2;
  if (m <= 256) return CS ? (const void*)&osd_block_cs_kernel<NW, 4, 1> : (const void*)&osd_block_kernel<NW, 4, 1>;
  if (m <= 512) return CS ? (const void*)&osd_block_cs_kernel<NW, 8, 2> : (const void*)&osd_block_kernel<NW, 8, 2>;
  return nullptr;                                   // (the engine state would spill: column kernel)
}

template <bool CS>
static const void* osd_block_by_words(int nw, int m, int* rows_per_thread) {
  if (nw <= 0) return nullptr;
  if (nw <= 4) return osd_block_by_rows<4, CS>(m, rows_per_thread);
  if (nw <= 9) return osd_block_by_rows<9, CS>(m, rows_per_thread);
  if (nw <= 17) return osd_block_by_rows<17, CS>(m, rows_per_thread);
  return nullptr;
}

// block kernel configurations whose state fits the VGPR budget without
// spills (m <= 512 rows, n <= 1087 columns); null -> osd_kernel. cs: the
// OSD-CS instance of the same configuration
const void* select_osd_block_kernel(int nw, int m, int* rows_per_thread, bool cs) {
  return cs ? osd_block_by_words<true>(nw, m, rows_per_thread) : osd_block_by_words<false>(nw, m, rows_per_thread);
}

int osd_nw_of(int nw) { return nw <= 4 ? 4 : nw <= 9 ? 9 : nw <= 17 ? 17 : nw <= 33 ? 33 : 0; }

}  // namespace qldpc
