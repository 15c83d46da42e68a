// osd_column.h — osd_kernel<NW>: exact REF, one barrier per column; alone, or the redo pass behind osd_block_kernel.
#pragma once
#include "osd_common.h"

namespace qldpc {

template <int NW>
__global__ void __launch_bounds__(1024) osd_kernel(OsdArgs a) {
  // LDS: inv_perm[n] | J list [m+2] | inJ bytes [n] | emask [NW] u64 |
  //      candidate rows [2][16][NW] | xrow rows [2][NW] | candidate ids [2][16] |
  //      misc [4] | set table                     (bytes: osd_column_lds, osd_kernels.h)
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

}  // namespace qldpc
