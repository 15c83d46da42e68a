// hard_kernels.hip — the reference's two hard-decision decoders on gfx950:
//   bf_kernel  BF_decoder (decoders.py:74-102)   bit flipping
//   ng_kernel  NG_decoder (decoders.py:27-66)    naive greedy
// One wavefront decodes one half-shot start to finish; waves are persistent
// and take half-shots from the guided work queue of DESIGN.md §3.6 (or a
// static stride). Integer only. The graph tables are 16-bit, in original
// variable labels, and stay in global memory (tens of KB per code, read by
// every wave alike: cache hits); LDS holds only each wave's own state, so the
// registers bound the occupancy, not LDS.
#include "hard_kernels.h"
#include "wave_common.h"

namespace qldpc {
namespace {

typedef uint32_t __attribute__((may_alias)) u32a;   // ng_kernel reads its u16 scores in pairs

// wave_sync, ld_const and the persistent half-shot loop (HalfShotQueue: one
// static half-shot per wave, then guided chunks of a global ticket counter)
// are wave_common.h's, shared with the MS / BP kernels. NG's step count varies
// from 0 to 2n between half-shots: the queue is what balances it.

// 64 predicate bits of the chunk starting at index i0 (a multiple of 64) into a word array
__device__ __forceinline__ void store_chunk(uint32_t* words, int i0, uint64_t bits, int lane) {
  if (lane == 0) {
    words[i0 >> 5] = (uint32_t)bits;
    words[(i0 >> 5) + 1] = (uint32_t)(bits >> 32);
  }
}

__device__ __forceinline__ uint32_t bit_of(const uint32_t* words, int i) { return (words[i >> 5] >> (i & 31)) & 1u; }

// Syndrome of half-shot hs as 2 wm 32-bit words in w (and w2, if given), bits
// past m cleared whatever the input holds there.
__device__ __forceinline__ void load_syndrome(const HardArgs& a, long long hs, uint32_t* w, uint32_t* w2, int lane) {
  const int m = a.m;
  if (a.syn_bits) {
    const uint32_t* src = (const uint32_t*)((const uint64_t*)a.syn + hs * a.wm);
    for (int i = lane; i < 2 * a.wm; i += 64) {
      const int left = m - 32 * i;
      uint32_t x = left > 0 ? src[i] : 0u;
      if (left > 0 && left < 32) x &= (1u << left) - 1u;
      w[i] = x;
      if (w2) w2[i] = x;
    }
  } else {
    const uint8_t* src = (const uint8_t*)a.syn + hs * (long long)m;
    for (int c0 = 0; c0 < 64 * a.wm; c0 += 64) {
      const int c = c0 + lane;
      const uint64_t b = __ballot(c < m ? (src[c] & 1) : 0);
      store_chunk(w, c0, b, lane);
      if (w2) store_chunk(w2, c0, b, lane);
    }
  }
}

// estimate (original variable order, either format), count and flag of half-shot hs
__device__ __forceinline__ void write_outputs(const HardArgs& a, long long hs, const uint32_t* ew, int count, bool conv,
                                              int lane) {
  if (a.eh_bits) {
    uint64_t* dst = (uint64_t*)a.ehat + hs * a.wn;
    for (int w = lane; w < a.wn; w += 64) dst[w] = (uint64_t)ew[2 * w] | ((uint64_t)ew[2 * w + 1] << 32);
  } else {
    uint8_t* dst = (uint8_t*)a.ehat + hs * (long long)a.n;
    for (int v = lane; v < a.n; v += 64) dst[v] = (uint8_t)bit_of(ew, v);
  }
  if (lane == 0) {
    a.iters[hs] = count;
    if (a.flags) a.flags[hs] = conv ? 1 : 0;
  }
}

// cnt[u] = set bits of `words` over the list of item i = i0 + 64 u + lane
// (u < U); len[u] = the list's length, 0 for i >= count. A list's first 8
// entries come from the ELL table (8 u16 per item, padded with 0): ONE
// coalesced 16-byte load per lane. Gathering them entry by entry from the
// CSR / CSC table cost 5-8 scattered 2-byte loads per item, and the kernels
// were bound by the vector memory pipeline's address rate (measured: loading 8
// instead of 5 entries per variable that way ran 2.1x slower). Entries past 8
// (tab[ptr[i] + 8 ..)) finish in a loop: no shipped code has any.
template <int U>
__device__ __forceinline__ void gather_bits(const uint16_t* ptr, const uint16_t* tab, const uint16_t* ell,
                                            const uint32_t* words, int i0, int count, int lane, int (&cnt)[U],
                                            int (&len)[U]) {
  int kb[U];
  uint4 q[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = i0 + 64 * u + lane;
    const int ic = i < count ? i : 0;
    kb[u] = ptr[ic];
    // (a mask, not a select: the compiler sank the second load into a branch
    // of its own and waited there for both, before the ELL load was issued)
    len[u] = ((int)ptr[ic + 1] - kb[u]) & -(int)(i < count);
    q[u] = ((const uint4*)ell)[ic];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
    uint32_t b[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) b[d] = bit_of(words, (int)((w[d >> 1] >> (16 * (d & 1))) & 0xFFFFu));
    int c = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) c += d < len[u] ? (int)b[d] : 0;
    for (int k = kb[u] + 8; k < kb[u] + len[u]; ++k) c += (int)bit_of(words, tab[k]);
    cnt[u] = c;
  }
}

constexpr int kGatherU = 2;   // 64-item chunks per trip: their loads are in flight together

}  // namespace

// ---------------------------------------------------------------------------
// Bit flipping. e, r and the syndrome are bit words in LDS. Per iteration:
//   lane per variable: nuc = failing checks at v; flip e[v] where 2 nuc > deg
//     (strict: an even degree needs more than half; degree 0 never flips);
//   lane per check:    r[c] = (row c holds a set e bit) XOR syndrome[c] — a
//     non-zero count, not a parity (`s_hat.astype(bool)`, decoders.py:97-98);
//   stop when r is all zero (a wave-wide OR of the chunk ballots).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * kHardMaxWaves) bf_kernel(HardArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, waves = blockDim.x >> 6;
  unsigned char* ws = lds + wid * a.wave_bytes;
  uint32_t* synw = (uint32_t*)ws;
  uint32_t* rw = (uint32_t*)(ws + a.off_res);
  uint32_t* ew = (uint32_t*)(ws + a.off_est);
  const int m = a.m, n = a.n;

  for (HalfShotQueue Q(a.batch, a.queue, waves, wid); Q.hs < a.batch; Q.advance()) {
    const long long hs = Q.hs;
    Q.prefetch(lane);
    load_syndrome(a, hs, synw, rw, lane);
    for (int i = lane; i < 2 * a.wn; i += 64) ew[i] = 0u;
    wave_sync();
    int it = 0;
    bool conv = false;
    while (it < a.max_iter) {
      ++it;
      for (int v0 = 0; v0 < n; v0 += 64 * kGatherU) {
        int nuc[kGatherU], deg[kGatherU];
        gather_bits<kGatherU>(a.col_ptr, a.col_chk, a.col_ell, rw, v0, n, lane, nuc, deg);
#pragma unroll
        for (int u = 0; u < kGatherU; ++u) {
          const uint64_t f = __ballot(2 * nuc[u] > deg[u]);   // (variables past n: 0 > 0)
          if (lane == 0 && v0 + 64 * u < n) {
            ew[(v0 >> 5) + 2 * u] ^= (uint32_t)f;
            ew[(v0 >> 5) + 2 * u + 1] ^= (uint32_t)(f >> 32);
          }
        }
      }
      wave_sync();
      uint64_t any = 0;
      for (int c0 = 0; c0 < m; c0 += 64 * kGatherU) {
        int hit[kGatherU], deg[kGatherU];
        gather_bits<kGatherU>(a.row_ptr, a.row_var, a.row_ell, ew, c0, m, lane, hit, deg);
#pragma unroll
        for (int u = 0; u < kGatherU; ++u) {
          const int c = c0 + 64 * u + lane;
          const uint32_t r = c < m ? (uint32_t)(hit[u] != 0) ^ bit_of(synw, c) : 0u;
          const uint64_t b = __ballot(r);
          if (c0 + 64 * u < m) store_chunk(rw, c0 + 64 * u, b, lane);
          any |= b;
        }
      }
      wave_sync();
      if (any == 0) {
        conv = true;
        break;
      }
    }
    write_outputs(a, hs, ew, it, conv, lane);
    wave_sync();   // the next half-shot reuses this wave's LDS slice
  }
}

// ---------------------------------------------------------------------------
// Naive greedy. score[v] (failing checks at v, u16 in LDS) is built once per
// half-shot and then kept up to date: flipping v* toggles the residual of each
// of its checks c in turn, and the lanes spread over row c add +1 / -1 to the
// row's variables. Check by check, so two checks that share a variable never
// update one score at the same time; inside a row the variables are distinct.
// The argmax packs (score << 16) | (0xFFFF - v): the largest key is the
// largest score at the LOWEST original index (np.argmax). Lanes scan the
// scores two per 32-bit read at stride 64 (consecutive lanes on consecutive
// banks: conflict-free; the key makes the scan order irrelevant), then a DPP
// max-scan reduces the wave with no LDS round trip.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
  // inclusive max-scan inside each row of 16 lanes (row_shr 1, 2, 4, 8: lanes
  // shifted in from outside the row read 0), then lane 15 of rows 0 / 2 into
  // rows 1 / 3 (row_bcast15) and lane 31 into rows 2, 3 (row_bcast31):
  // lane 63 holds the maximum of the wave
#define QLDPC_DPP_MAX(ctrl, rows) \
  x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, ctrl, rows, 0xf, false))
  QLDPC_DPP_MAX(0x111, 0xf);
  QLDPC_DPP_MAX(0x112, 0xf);
  QLDPC_DPP_MAX(0x114, 0xf);
  QLDPC_DPP_MAX(0x118, 0xf);
  QLDPC_DPP_MAX(0x142, 0xa);
  QLDPC_DPP_MAX(0x143, 0xc);
#undef QLDPC_DPP_MAX
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

__device__ __forceinline__ int wave_sum(int x) {
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return __builtin_amdgcn_readfirstlane(x);
}

__global__ void __launch_bounds__(64 * kHardMaxWaves) ng_kernel(HardArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, waves = blockDim.x >> 6;
  unsigned char* ws = lds + wid * a.wave_bytes;
  uint16_t* sc = (uint16_t*)ws;
  const u32a* sc2 = (const u32a*)ws;
  uint32_t* rw = (uint32_t*)(ws + a.off_res);
  uint32_t* ew = (uint32_t*)(ws + a.off_est);
  const int n = a.n, npad = a.npad;
  const int cap = 2 * n;

  for (HalfShotQueue Q(a.batch, a.queue, waves, wid); Q.hs < a.batch; Q.advance()) {
    const long long hs = Q.hs;
    Q.prefetch(lane);
    load_syndrome(a, hs, rw, nullptr, lane);
    for (int i = lane; i < 2 * a.wn; i += 64) ew[i] = 0u;
    wave_sync();
    int failing = 0;                                  // checks with a non-zero residual (wave-uniform)
    for (int i = lane; i < 2 * a.wm; i += 64) failing += __popc(rw[i]);
    failing = wave_sum(failing);
    if (failing > 0) {
      for (int v0 = 0; v0 < npad; v0 += 64 * kGatherU) {   // the padding keeps score 0: never chosen
        int s[kGatherU], deg[kGatherU];
        gather_bits<kGatherU>(a.col_ptr, a.col_chk, a.col_ell, rw, v0, n, lane, s, deg);
#pragma unroll
        for (int u = 0; u < kGatherU; ++u) sc[v0 + 64 * u + lane] = (uint16_t)(v0 + 64 * u + lane < n ? s[u] : 0);
      }
    }
    wave_sync();
    int steps = 0;
    while (failing > 0 && steps < cap) {
      ++steps;
      uint32_t key = 0;
      for (int i = lane; i < (npad >> 1); i += 64) {
        const uint32_t two = sc2[i];                  // scores of variables 2i (low half), 2i + 1
        const uint32_t k0 = (two << 16) | (uint32_t)(0xFFFF - 2 * i);
        const uint32_t k1 = (two & 0xFFFF0000u) | (uint32_t)(0xFFFF - (2 * i + 1));
        key = max(key, max(k0, k1));
      }
      key = wave_max_u32(key);
      if ((key >> 16) == 0) break;                    // no variable touches a failing check (step counted)
      const int v = 0xFFFF - (int)(key & 0xFFFFu);
      if (v >= n) break;                              // (cannot happen: guards the table reads below)
      if (lane == 0) ew[v >> 5] ^= 1u << (v & 31);
      const int kb = ld_const(a.col_ptr, v), ke = ld_const(a.col_ptr, v + 1);
      // the checks of v in groups of 4: lane i < 4 loads check i and its row
      // bounds, then every lane its entry of each of the 4 rows, before the
      // first score changes (one check at a time paid four dependent memory
      // latencies per check)
      for (int k0 = kb; k0 < ke; k0 += 4) {
        int cc = 0, rb = 0, rl = 0;
        if (lane < 4 && k0 + lane < ke) {
          cc = a.col_chk[k0 + lane];
          rb = a.row_ptr[cc];
          rl = (int)a.row_ptr[cc + 1] - rb;
        }
        int c[4], b[4], l[4], u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          c[i] = __builtin_amdgcn_readlane(cc, i);
          b[i] = __builtin_amdgcn_readlane(rb, i);
          l[i] = __builtin_amdgcn_readlane(rl, i);     // 0 past the column's last check
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = lane < l[i] ? (int)a.row_var[b[i] + lane] : -1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (k0 + i < ke) {
            const uint32_t word = rw[c[i] >> 5];
            const int now = __builtin_amdgcn_readfirstlane((int)(((word >> (c[i] & 31)) & 1u) ^ 1u));
            if (lane == 0) rw[c[i] >> 5] = word ^ (1u << (c[i] & 31));
            const int delta = now ? 1 : -1;
            failing += delta;
            if (u[i] >= 0) sc[u[i]] = (uint16_t)(sc[u[i]] + delta);
            for (int j = b[i] + 64 + lane; j < b[i] + l[i]; j += 64) {   // rows longer than 64
              const int w = a.row_var[j];
              sc[w] = (uint16_t)(sc[w] + delta);
            }
            wave_sync();
          }
        }
      }
    }
    write_outputs(a, hs, ew, steps, failing == 0, lane);
    wave_sync();   // the next half-shot reuses this wave's LDS slice
  }
}

const void* select_hard_kernel(int algo, const char** name) {
  if (algo == ALGO_BF) {
    if (name) *name = "bf_kernel";
    return (const void*)&bf_kernel;
  }
  if (algo == ALGO_NG) {
    if (name) *name = "ng_kernel";
    return (const void*)&ng_kernel;
  }
  return nullptr;
}

hipError_t configure_hard_kernel(const void* kernel, int lds_bytes) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
}

hipError_t launch_hard(const void* kernel, const HardArgs& args, int grid, int block, int lds_bytes,
                       hipStream_t stream) {
  void* params[] = {(void*)&args};
  return hipLaunchKernel(kernel, dim3(grid), dim3(block), params, (size_t)lds_bytes, stream);
}

}  // namespace qldpc
