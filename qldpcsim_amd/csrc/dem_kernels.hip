// dem_kernels.hip — shot source and outcome counter of a detector error model
// on the device (gfx950): N independent mechanisms with one probability each,
// column J of H [M, N] the detectors and column J of L [K, N] the observables
// mechanism J flips.
//
// dem_sample_kernel draws column J of shot s from the phenomenological
// sampler's generator,
//     u(s, J) = Philox4x32-10(key = seed, ctr = (J % 64, (J / 64) / 4,
//                             shot_lo, shot_hi))[(J / 64) % 4]
// and fires it iff u < thr[J], thr[J] = floor(p_J 2^32): on a space-time
// matrix with its prior row the fired row is phenom_sample_kernel's, and on
// any matrix channel_sample_vec_kernel's errX with (px, py, pz) = (p, 0, 0).
// It writes per shot the M detectors (bytes or words) and the ceil(K/64)
// observable words, and the fired row only if asked.
//
// dem_count_kernel reads an estimate (bytes or words), forms A ehat and the
// shot's class: 2 decoder failure (H ehat != detectors), else 1 logical error
// (L ehat != observables), else 0. Four int64 counters: failures, logical
// errors, successes, iteration sum. It needs no error vector.
//
// Both: one wavefront per shot (grid-stride), lane l owns bit l of every
// 64-bit word of columns (a ballot makes the fired word). The walk is
// column-major: only the lists of set columns (fired, or 1 in the estimate)
// are read, each entry's bit XORed into the wave's LDS row of 64 (MW + KW)
// bits with an LDS atomic (flip_columns), so the work of a shot follows the
// number of set columns, not the number of edges, and no row degree enters
// (an observable row of a circuit-level model touches hundreds of columns).
// The tables (thresholds, column pointers, lists) are read from global
// memory; LDS holds the waves' rows alone.

#include <cstdio>

#include "dem_kernels.h"
#include "channel_common.h"
#include "wave_common.h"

namespace qldpc {
namespace {

// XOR the lists of the set columns of word w (`bits`, wave-uniform: bit l is
// column 64 w + l) into the wave's row (32-bit words of LDS). Few set columns
// (a fired row; a decoder's estimate): the wave takes them one after the
// other, lane l the entries l, l + 64, ... of the list, so a long list (an
// observable-heavy column) is one step. Many (more than kDemLaneWalk of the
// 64: a dense estimate): every lane walks its own column instead.
constexpr int kDemLaneWalk = 16;

template <typename IT>
__device__ __forceinline__ void flip_columns(const DemTabs& t, uint64_t bits, int w, int lane, uint32_t* row32) {
  if (!bits) return;  // wave-uniform
  const IT* tg = static_cast<const IT*>(t.tg);
  const int J = 64 * w + lane;
  int e0 = 0, e1 = 0;
  if (J < t.N) {
    e0 = t.cp[J];
    e1 = t.cp[J + 1];
  }
  if (__popcll(bits) > kDemLaneWalk) {
    if ((bits >> lane) & 1)
      for (int e = e0; e < e1; ++e) {
        const uint32_t r = tg[e];
        atomicXor(&row32[r >> 5], 1u << (r & 31));
      }
    return;
  }
  while (bits) {
    const int src = __ffsll((unsigned long long)bits) - 1;
    bits &= bits - 1;
    const int b1 = __builtin_amdgcn_readlane(e1, src);
    for (int e = __builtin_amdgcn_readlane(e0, src) + lane; e < b1; e += 64) {
      const uint32_t r = tg[e];
      atomicXor(&row32[r >> 5], 1u << (r & 31));
    }
  }
}

template <typename IT>
__global__ void __launch_bounds__(64 * kDemWaves) dem_sample_kernel(DemSampleArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const DemTabs& t = a.t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NW = t.NW, MW = t.MW, KW = t.KW, RW = MW + KW;
  uint64_t* row = reinterpret_cast<uint64_t*>(smem) + (size_t)wave * RW;
  uint32_t* row32 = reinterpret_cast<uint32_t*>(row);
  for (long long b = (long long)blockIdx.x * kDemWaves + wave; b < a.batch; b += (long long)gridDim.x * kDemWaves) {
    const uint64_t shot = a.shot0 + (uint64_t)b;
    for (int w = lane; w < RW; w += 64) row[w] = 0;
    wave_sync();
    for (int wq = 0; 4 * wq < NW; ++wq) {
      const uint4 r = philox4x32_10((uint32_t)lane, (uint32_t)wq, (uint32_t)shot, (uint32_t)(shot >> 32), a.key0,
                                    a.key1);
      const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int w = 4 * wq + i;
        if (w >= NW) break;  // wave-uniform
        const int J = 64 * w + lane;
        const bool f = J < t.N && rr[i] < t.thr[J < t.N ? J : 0];
        const uint64_t bits = ballot_b(f);
        if (a.fired && lane == 0) a.fired[b * NW + w] = bits;
        flip_columns<IT>(t, bits, w, lane, row32);
      }
    }
    wave_sync();
    if (a.det_bits) {
      uint64_t* out = reinterpret_cast<uint64_t*>(a.det) + b * MW;
      for (int w = lane; w < MW; w += 64) out[w] = row[w];
    } else {
      uint8_t* out = a.det + b * t.M;
      for (int d = lane; d < t.M; d += 64) out[d] = (uint8_t)((row[d >> 6] >> (d & 63)) & 1);
    }
    for (int w = lane; w < KW; w += 64) a.obs[b * KW + w] = row[MW + w];
    wave_sync();  // the next shot clears the row
  }
}

template <typename IT>
__global__ void __launch_bounds__(64 * kDemWaves) dem_count_kernel(DemCountArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const DemTabs& t = a.t;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NW = t.NW, MW = t.MW, KW = t.KW, RW = MW + KW;
  constexpr int NC = kDemCounters;
  unsigned long long* part = reinterpret_cast<unsigned long long*>(smem);          // [waves][NC]
  uint64_t* row = reinterpret_cast<uint64_t*>(part + NC * kDemWaves) + (size_t)wave * RW;
  uint32_t* row32 = reinterpret_cast<uint32_t*>(row);
  unsigned long long cnt[NC] = {0, 0, 0, 0};
  for (long long b = (long long)blockIdx.x * kDemWaves + wave; b < a.batch; b += (long long)gridDim.x * kDemWaves) {
    const int it = a.iters[b];
    for (int w = lane; w < RW; w += 64) row[w] = 0;
    wave_sync();
    if (a.eh_bits) {
      const uint64_t* eh = reinterpret_cast<const uint64_t*>(a.ehat) + b * NW;
      for (int w0 = 0; w0 < NW; w0 += 64) {       // 64 words in one read, then lane i's word broadcast
        const uint64_t mine = w0 + lane < NW ? eh[w0 + lane] : 0;
        const int nw = NW - w0 < 64 ? NW - w0 : 64;
        for (int i = 0; i < nw; ++i) {
          const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(mine >> 32), i) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)mine, i);
          const int left = t.N - 64 * (w0 + i);  // the last word's padding bits do not count
          flip_columns<IT>(t, left >= 64 ? word : word & ((1ull << left) - 1), w0 + i, lane, row32);
        }
      }
    } else {                                     // one byte per column: a ballot per word
      const uint8_t* eh = a.ehat + b * t.N;
      for (int w = 0; w < NW; ++w) {
        const int J = 64 * w + lane;
        flip_columns<IT>(t, ballot_b(J < t.N && (eh[J < t.N ? J : 0] & 1)), w, lane, row32);
      }
    }
    wave_sync();
    bool bad = false;
    if (a.det_bits) {
      const uint64_t* d = reinterpret_cast<const uint64_t*>(a.det) + b * MW;
      for (int w = lane; w < MW; w += 64) {
        const int left = t.M - 64 * w;           // the last word's padding bits do not count
        const uint64_t mask = left >= 64 ? ~0ull : (1ull << left) - 1;
        bad |= ((row[w] ^ d[w]) & mask) != 0;
      }
    } else {
      const uint8_t* d = a.det + b * t.M;
      for (int i = lane; i < t.M; i += 64) bad |= ((row[i >> 6] >> (i & 63)) & 1) != (uint64_t)(d[i] & 1);
    }
    bool lg = false;
    for (int w = lane; w < KW; w += 64) {
      const uint64_t fl = row[MW + w] ^ a.obs[b * KW + w];
      lg |= fl != 0;
      if (a.flips) a.flips[b * KW + w] = fl;
    }
    const bool fail = ballot_b(bad) != 0, logical = ballot_b(lg) != 0;
    if (lane == 0) {
      const int c = fail ? 2 : (logical ? 1 : 0);
      if (a.cls) a.cls[b] = (uint8_t)c;
      cnt[0] += c == 2;
      cnt[1] += c == 1;
      cnt[2] += c == 0;
      cnt[3] += (unsigned long long)(long long)it;
    }
    wave_sync();  // the next shot clears the row
  }
  if (lane == 0)
    for (int k = 0; k < NC; ++k) part[wave * NC + k] = cnt[k];
  __syncthreads();
  if (threadIdx.x < NC) {
    unsigned long long s = 0;
    for (int w = 0; w < kDemWaves; ++w) s += part[w * NC + threadIdx.x];
    if (s) atomicAdd(&a.acc[threadIdx.x], s);
  }
}

template <typename K>
hipError_t launch(K kernel, const void* args, int grid, long long lds, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  void* params[] = {const_cast<void*>(args)};
  return hipLaunchKernel((const void*)kernel, dim3(grid), dim3(64 * kDemWaves), params, (size_t)lds, stream);
}

}  // namespace

bool dem_kernel_name(int kind, bool wide, char* buf, int len) {
  if (kind != kDemSample && kind != kDemCount) return false;
  snprintf(buf, len, "%s<%d>", kind == kDemSample ? "dem_sample_kernel" : "dem_count_kernel", wide ? 32 : 16);
  return true;
}

long long dem_lds_bytes(const DemTabs& t) {
  return 8ll * kDemCounters * kDemWaves + (long long)kDemWaves * 8 * (t.MW + t.KW);
}

hipError_t launch_dem_sample(const DemSampleArgs& a, int grid, hipStream_t stream) {
  const long long lds = dem_lds_bytes(a.t);
  return a.t.wide ? launch(dem_sample_kernel<uint32_t>, &a, grid, lds, stream)
                  : launch(dem_sample_kernel<uint16_t>, &a, grid, lds, stream);
}

hipError_t launch_dem_count(const DemCountArgs& a, int grid, hipStream_t stream) {
  const long long lds = dem_lds_bytes(a.t);
  return a.t.wide ? launch(dem_count_kernel<uint32_t>, &a, grid, lds, stream)
                  : launch(dem_count_kernel<uint16_t>, &a, grid, lds, stream);
}

}  // namespace qldpc
