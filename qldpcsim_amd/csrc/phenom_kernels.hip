// phenom_kernels.hip — shot source and outcome counter of the phenomenological
// noise model on the device (gfx950): T rounds of syndrome extraction of one
// CSS half (H [m, n], logical table L [k, n]) with data error probability
// p_data per qubit and round and measurement error probability q per check
// and round, the last round measured perfectly.
//
// Space-time columns, round-major (N = T n + (T-1) m): round t owns data
// columns t (n+m) + j and, for t < T-1, measurement columns t (n+m) + n + c.
// Detector row t m + c:  d_t[c] = (H e_t)[c] ^ u_t[c] ^ u_{t-1}[c], with
// u_{-1} = u_{T-1} = 0. Neither kernel materialises the space-time matrix:
// both walk H's own CSR at the round's bit offset.
//
// phenom_sample_kernel draws column J of shot s from channel_sample_kernel's
// generator with j := J,
//     u(s, J) = Philox4x32-10(key = seed, ctr = (J % 64, (J / 64) / 4,
//                             shot_lo, shot_hi))[(J / 64) % 4]
// and fires it iff u < thr (thr_data on data columns, thr_meas on measurement
// columns), so the fired row is channel_sample_vec_kernel's errX on the
// materialised matrix with (px, py, pz) = (prior, 0, 0). It keeps the N-bit
// fired row in the wave's LDS slice and writes per shot the T m detectors
// (bytes or words), E = XOR_t e_t ([ceil(n/64)] words) and, if asked, the
// fired row.
//
// phenom_count_kernel reads the space-time estimate (bytes or words), forms
// H_st ehat round by round, folds Ehat = XOR_t ehat_t, r = E ^ Ehat, L r, and
// the shot's class: 2 decoder failure (H_st ehat != d), 1 logical error (not
// 2, L r != 0), 0 success. Four int64 counters: failures, logical errors,
// successes, iteration sum.
//
// phenom_window_kernel is the step between two windows of sliding-window
// decoding: it copies the decoded window's committed columns
// into the shot's full estimate row at bit offset a (n+m), adds the window's
// iteration count, and cuts the next window's syndrome from bit offset a' m of
// the detector row, its first m entries XORed with the committed measurement
// estimate. Each of the four rows is bytes or words on its own; in words
// either offset may or may not be a multiple of 64 (it is one at every step
// when n + m is), so reads are funnel shifts that fall back to the plain word
// at shift 0, and the first and last destination word of a commit are merged
// with the row's unless the commit starts or ends on a word boundary.
//
// Sampler and counter: one wavefront per shot (grid-stride), H's CSR staged once per
// workgroup into LDS as 16-bit column indices (and, for the counter, L's
// word-major table) — neither depends on T; lane l owns bit l of every 64-bit
// word (ballots assemble the words); detectors are lane-parallel over checks.

#include <cstdio>

#include "phenom_kernels.h"
#include "channel_common.h"
#include "wave_common.h"

namespace qldpc {
namespace {

struct HTabs {
  const int* rp;
  const uint16_t* ci;
  unsigned char* tail;  // 8-byte aligned, after the tables
};

__host__ __device__ __forceinline__ int csr_bytes(int m, int e) { return (4 * (m + 1) + 2 * e + 7) & ~7; }

// stage H's CSR into LDS (whole workgroup; caller syncs)
__device__ HTabs stage_h(const PhenomTabs& t, unsigned char* smem) {
  int* rp = reinterpret_cast<int*>(smem);
  uint16_t* ci = reinterpret_cast<uint16_t*>(rp + (t.m + 1));
  for (int i = threadIdx.x; i <= t.m; i += blockDim.x) rp[i] = t.rp[i];
  for (int i = threadIdx.x; i < t.e; i += blockDim.x) ci[i] = (uint16_t)t.ci[i];
  return HTabs{rp, ci, smem + csr_bytes(t.m, t.e)};
}

// bit `pos` of the packed vector `w` (LDS, 32-bit words)
__device__ __forceinline__ uint32_t bit_at(const uint32_t* w, int pos) { return (w[pos >> 5] >> (pos & 31)) & 1u; }

// Parity of row c of H over the bits off + j of the packed vector `w` (a
// round's data block starts at any bit offset). DC > 0: every row has DC
// entries (the reads are unrolled and issued together).
template <int DC>
__device__ __forceinline__ uint32_t row_parity_at(const int* rp, const uint16_t* ci, int c, const uint32_t* w,
                                                  int off) {
  uint32_t par = 0;
  if constexpr (DC > 0) {
    uint32_t j[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) j[k] = off + ci[c * DC + k];
#pragma unroll
    for (int k = 0; k < DC; ++k) par ^= w[j[k] >> 5] >> (j[k] & 31);
  } else {
    const int e1 = rp[c + 1];
    for (int e = rp[c]; e < e1; ++e) {
      const uint32_t j = off + ci[e];
      par ^= w[j >> 5] >> (j & 31);
    }
  }
  return par & 1u;
}

// Detector t m + c (round rt, check c) of the N-bit vector `w` (fired row or
// estimate): (H x_t)[c] ^ u_t[c] ^ u_{t-1}[c].
template <int DC>
__device__ __forceinline__ uint32_t detector_bit(const PhenomTabs& t, const HTabs& tb, int rt, int c,
                                                 const uint32_t* w) {
  const int off = rt * (t.n + t.m);
  uint32_t x = row_parity_at<DC>(tb.rp, tb.ci, c, w, off);
  if (rt < t.rounds - 1) x ^= bit_at(w, off + t.n + c);
  if (rt >= 1) x ^= bit_at(w, off - t.m + c);
  return x;
}

// (quotient, remainder) of 64 w + lane by a divisor fixed for the kernel,
// stepped from word to word without a division: start at w = 0, next() moves
// to w + 1.
struct LaneDiv {
  int q, r, dq, dr, div;
  __device__ __forceinline__ LaneDiv(int lane, int divisor)
      : q(lane / divisor), r(lane % divisor), dq(64 / divisor), dr(64 % divisor), div(divisor) {}
  __device__ __forceinline__ void next() {
    q += dq;
    r += dr;
    if (r >= div) {
      r -= div;
      ++q;
    }
  }
};

// Word k (< W) of the XOR of the T data blocks of the N-bit vector `v`
// (64-bit words, one zero word behind the last: a block starts at any bit).
__device__ __forceinline__ uint64_t fold_word(const PhenomTabs& t, const uint64_t* v, int k) {
  uint64_t x = 0;
  for (int rt = 0; rt < t.rounds; ++rt) {
    const int b = rt * (t.n + t.m) + 64 * k;
    const int sh = b & 63;
    const uint64_t lo = v[b >> 6], hi = v[(b >> 6) + 1];
    x ^= sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
  }
  const int left = t.n - 64 * k;  // bits of this word that lie in the block
  return left >= 64 ? x : x & ((1ull << left) - 1);
}

template <int DC>
__global__ void __launch_bounds__(64 * kPhenomWaves) phenom_sample_kernel(PhenomSampleArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const PhenomTabs& t = a.t;
  const HTabs tb = stage_h(t, smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NW = t.NW, W = t.W, nm = t.n + t.m;
  uint64_t* fired = reinterpret_cast<uint64_t*>(tb.tail) + (size_t)wave * (NW + 1);  // + one zero word
  const uint32_t* f32 = reinterpret_cast<const uint32_t*>(fired);
  if (lane == 0) fired[NW] = 0;
  const LaneDiv col0(lane, nm > 0 ? nm : 1), det0(lane, t.m > 0 ? t.m : 1);
  __syncthreads();
  for (long long b = (long long)blockIdx.x * kPhenomWaves + wave; b < a.batch;
       b += (long long)gridDim.x * kPhenomWaves) {
    const uint64_t shot = a.shot0 + (uint64_t)b;
    LaneDiv col = col0;                         // J = 64 w + lane by n + m: the remainder names the column's kind
    for (int wq = 0; 4 * wq < NW; ++wq) {
      const uint4 r = philox4x32_10((uint32_t)lane, (uint32_t)wq, (uint32_t)shot, (uint32_t)(shot >> 32), a.key0,
                                    a.key1);
      const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int w = 4 * wq + i;
        if (w >= NW) break;  // wave-uniform
        const int J = 64 * w + lane;
        const uint64_t thr = col.r < t.n ? a.thr_data : a.thr_meas;
        const uint64_t bits = __ballot(J < t.N && (uint64_t)rr[i] < thr);
        if (lane == 0) fired[w] = bits;
        col.next();
      }
    }
    wave_sync();
    if (a.fired)
      for (int w = lane; w < NW; w += 64) a.fired[b * NW + w] = fired[w];
    if (lane < W) a.E[b * W + lane] = fold_word(t, fired, lane);
    LaneDiv dd = det0;                          // d = 64 w + lane by m: (round, check)
    for (int d0 = 0; d0 < t.M; d0 += 64, dd.next()) {
      const int d = d0 + lane;
      const uint32_t x = d < t.M ? detector_bit<DC>(t, tb, dd.q, dd.r, f32) : 0u;
      if (a.det_bits) {
        const uint64_t bits = __ballot(x);
        if (lane == 0) reinterpret_cast<uint64_t*>(a.det)[b * t.MW + (d0 >> 6)] = bits;
      } else if (d < t.M) {
        a.det[b * t.M + d] = (uint8_t)x;
      }
    }
    wave_sync();  // the next shot overwrites the fired row
  }
}

template <int DC>
__global__ void __launch_bounds__(64 * kPhenomWaves) phenom_count_kernel(PhenomCountArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const PhenomTabs& t = a.t;
  const HTabs tb = stage_h(t, smem);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NW = t.NW, W = t.W, kp = a.kp, kw = a.kp >> 6;
  constexpr int NC = kPhenomCounters;
  unsigned long long* part = reinterpret_cast<unsigned long long*>(tb.tail);  // [waves][NC]
  uint64_t* ltab = reinterpret_cast<uint64_t*>(part + NC * kPhenomWaves);     // tab_lds: L, [W][kp]
  const size_t tab_words = a.tab_lds ? (size_t)W * kp : 0;
  uint64_t* est = ltab + tab_words + (size_t)wave * (NW + 1 + W);  // the estimate, + one zero word
  uint64_t* res = est + NW + 1;                                    // residual words E ^ fold(ehat)
  const uint32_t* e32 = reinterpret_cast<const uint32_t*>(est);
  for (size_t i = threadIdx.x; i < tab_words; i += blockDim.x) ltab[i] = a.tab[i];
  if (lane == 0) est[NW] = 0;
  const LaneDiv det0(lane, t.m > 0 ? t.m : 1);
  __syncthreads();
  const uint64_t* lt = a.tab_lds ? ltab : a.tab;
  unsigned long long cnt[NC] = {0, 0, 0, 0};
  for (long long b = (long long)blockIdx.x * kPhenomWaves + wave; b < a.batch;
       b += (long long)gridDim.x * kPhenomWaves) {
    const uint64_t tE = lane < W ? a.E[b * W + lane] : 0;
    const int it = a.iters[b];
    if (a.eh_bits) {                            // already words
      const uint64_t* row = reinterpret_cast<const uint64_t*>(a.ehat) + b * NW;
      for (int w = lane; w < NW; w += 64) est[w] = row[w];
    } else {                                    // one byte per column: a ballot per word
      const uint8_t* row = a.ehat + b * t.N;
      for (int w = 0; w < NW; ++w) {
        const int J = 64 * w + lane;
        const uint64_t bits = __ballot(J < t.N && (row[J < t.N ? J : 0] & 1));
        if (lane == 0) est[w] = bits;
      }
    }
    wave_sync();
    if (lane < W) res[lane] = tE ^ fold_word(t, est, lane);
    bool bad = false;
    LaneDiv dd = det0;                          // d = 64 w + lane by m: (round, check)
    for (int d0 = 0; d0 < t.M; d0 += 64, dd.next()) {
      const int d = d0 + lane;
      if (d < t.M) {
        const uint32_t s = a.det_bits
                               ? (uint32_t)(reinterpret_cast<const uint64_t*>(a.det)[b * t.MW + (d >> 6)] >> (d & 63)) & 1u
                               : (uint32_t)(a.det[b * t.M + d] & 1);
        bad |= detector_bit<DC>(t, tb, dd.q, dd.r, e32) != s;
      }
    }
    const bool fail = __ballot(bad) != 0;
    wave_sync();  // res is read by every lane below
    bool lg = false;
    const uint64_t fl = logical_flips(lt, res, W, kp, lane, &lg);
    if (a.flips && lane < kw) a.flips[b * kw + lane] = fl;
    if (a.resid && lane < W) a.resid[b * W + lane] = res[lane];
    if (lane == 0) {
      const int c = fail ? 2 : (lg ? 1 : 0);
      if (a.cls) a.cls[b] = (uint8_t)c;
      cnt[0] += c == 2;
      cnt[1] += c == 1;
      cnt[2] += c == 0;
      cnt[3] += (unsigned long long)(long long)it;
    }
    wave_sync();  // the next shot overwrites the wave's slot
  }
  if (lane == 0)
    for (int k = 0; k < NC; ++k) part[wave * NC + k] = cnt[k];
  __syncthreads();
  if (threadIdx.x < NC) {
    unsigned long long s = 0;
    for (int w = 0; w < kPhenomWaves; ++w) s += part[w * NC + threadIdx.x];
    if (s) atomicAdd(&a.acc[threadIdx.x], s);
  }
}

// One shot's row of a 0/1 vector in either wire format: one byte per entry
// (`bytes`), else 64-bit words. Entries outside [0, len) read as zero, the
// words' padding bits included.
struct BitRow {
  const uint8_t* bytes;
  const uint64_t* words;
  int len;
  __device__ __forceinline__ uint32_t bit(int pos) const {
    if (pos < 0 || pos >= len) return 0u;
    return bytes ? (uint32_t)(bytes[pos] & 1) : (uint32_t)(words[pos >> 6] >> (pos & 63)) & 1u;
  }
  // entries [pos, pos + 64) of a words row (pos at any bit, negative too): a
  // funnel shift of two adjacent words
  __device__ __forceinline__ uint64_t word(int pos) const {
    const int nw = (len + 63) >> 6, w0 = pos >> 6, sh = pos & 63;  // pos >> 6 floors
    const uint64_t lo = (w0 >= 0 && w0 < nw) ? words[w0] : 0;
    const uint64_t hi = (sh && w0 + 1 >= 0 && w0 + 1 < nw) ? words[w0 + 1] : 0;
    const uint64_t x = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    const int left = len - pos;  // entries of this word that lie in the row
    return left >= 64 ? x : (left <= 0 ? 0 : x & ((1ull << left) - 1));
  }
};

__device__ __forceinline__ BitRow bit_row(const uint8_t* base, int bits, long long b, int len) {
  if (bits) return BitRow{nullptr, reinterpret_cast<const uint64_t*>(base) + b * ((len + 63) >> 6), len};
  return BitRow{base + b * len, nullptr, len};
}

// dst[dst_off + j] = a[a_off + j] ^ x[x_off + j] for j < len (> 0), by one
// wave; `x` is clipped by its len (len 0: none). dst is a shot's row, bytes
// or (dst_bits) words. Words: entries below dst_off in the first word keep
// what the row holds, and so do those above the end in the last word unless
// zero_tail, which clears them (the row's padding). The wave owns the row, so
// the merge is a plain read and write.
__device__ __forceinline__ void copy_bits(const BitRow& a, int a_off, const BitRow& x, int x_off, uint8_t* dst,
                                          int dst_bits, int dst_off, int len, bool zero_tail, int lane) {
  if (!dst_bits) {
    for (int j = lane; j < len; j += 64) dst[dst_off + j] = (uint8_t)(a.bit(a_off + j) ^ x.bit(x_off + j));
    return;
  }
  uint64_t* dw = reinterpret_cast<uint64_t*>(dst);
  const int end = dst_off + len, w0 = dst_off >> 6, w1 = (end - 1) >> 6;
  const bool words = !a.bytes && !x.bytes;           // every source is words: a lane per destination word
  // word w of the row from `val`, whose bit 0 is source entry j0 = 64 w - dst_off
  auto store = [&](int w, uint64_t val) {
    const int j0 = 64 * w - dst_off, left = end - 64 * w;
    uint64_t in = ~0ull, keep = 0;                   // bits inside [dst_off, end); bits left as the row holds them
    if (j0 < 0) {
      in = ~0ull << -j0;
      keep = ~in;
    }
    if (left < 64) {
      const uint64_t above = ~0ull << left;
      in &= ~above;
      if (!zero_tail) keep |= above;
    }
    dw[w] = keep ? (dw[w] & keep) | (val & in) : val & in;
  };
  if (words) {
    for (int w = w0 + lane; w <= w1; w += 64) {
      const int j0 = 64 * w - dst_off;               // negative in the first word
      store(w, a.word(a_off + j0) ^ x.word(x_off + j0));
    }
  } else {                                           // a byte source: a ballot per word
    for (int w = w0; w <= w1; ++w) {
      const int j = 64 * w - dst_off + lane;
      const uint64_t val = __ballot(a.bit(a_off + j) ^ x.bit(x_off + j));
      if (lane == 0) store(w, val);
    }
  }
}

// Sliding-window step: one wavefront per shot (grid-stride). No tables and no
// LDS: a lane owns 64-bit words of the shot's rows.
__global__ void __launch_bounds__(64 * kPhenomWaves) phenom_window_kernel(PhenomWindowArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const BitRow none{nullptr, nullptr, 0};
  for (long long b = (long long)blockIdx.x * kPhenomWaves + wave; b < a.batch;
       b += (long long)gridDim.x * kPhenomWaves) {
    BitRow corr = none;
    if (a.has_done) {
      const BitRow west = bit_row(a.west, a.west_bits, b, a.west_len);
      uint8_t* row = a.eh_bits ? a.ehat + 8 * b * ((a.N + 63) >> 6) : a.ehat + b * a.N;
      copy_bits(west, 0, none, 0, row, a.eh_bits, a.commit_off, a.commit_len, a.commit_off + a.commit_len == a.N,
                lane);
      if (lane == 0) a.iters[b] += a.witers[b];
      corr = west;
      corr.len = a.corr_off + a.m;                   // u_{a'-1}: m entries from corr_off
    }
    if (a.has_next) {
      const BitRow det = bit_row(a.det, a.det_bits, b, a.M);
      uint8_t* row = a.syn_bits ? a.syn + 8 * b * ((a.syn_len + 63) >> 6) : a.syn + b * a.syn_len;
      copy_bits(det, a.syn_off, corr, a.corr_off, row, a.syn_bits, 0, a.syn_len, true, lane);
    }
  }
}

template <typename K>
hipError_t launch(K kernel, const void* args, int grid, long long lds, hipStream_t stream) {
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  void* params[] = {const_cast<void*>(args)};
  return hipLaunchKernel((const void*)kernel, dim3(grid), dim3(64 * kPhenomWaves), params, (size_t)lds, stream);
}

}  // namespace

int phenom_choice(const PhenomTabs& t) { return (t.udeg == 6 || t.udeg == 7 || t.udeg == 8) ? t.udeg : 0; }

bool phenom_kernel_name(int kind, int deg, char* buf, int len) {
  if (kind != kPhenomSample && kind != kPhenomCount) return false;
  snprintf(buf, len, "%s<%d>", kind == kPhenomSample ? "phenom_sample_kernel" : "phenom_count_kernel", deg);
  return true;
}

long long phenom_sample_lds_bytes(const PhenomTabs& t) {
  return csr_bytes(t.m, t.e) + (long long)kPhenomWaves * 8 * (t.NW + 1);
}

long long phenom_count_lds_bytes(const PhenomTabs& t, int kp, bool tab_lds) {
  long long b = csr_bytes(t.m, t.e) + 8ll * kPhenomCounters * kPhenomWaves;
  if (tab_lds) b += 8ll * t.W * kp;
  return b + (long long)kPhenomWaves * 8 * (t.NW + 1 + t.W);
}

hipError_t launch_phenom_sample(const PhenomSampleArgs& a, int grid, hipStream_t stream) {
  const long long lds = phenom_sample_lds_bytes(a.t);
  switch (phenom_choice(a.t)) {
    case 6: return launch(phenom_sample_kernel<6>, &a, grid, lds, stream);
    case 7: return launch(phenom_sample_kernel<7>, &a, grid, lds, stream);
    case 8: return launch(phenom_sample_kernel<8>, &a, grid, lds, stream);
    default: return launch(phenom_sample_kernel<0>, &a, grid, lds, stream);
  }
}

hipError_t launch_phenom_count(const PhenomCountArgs& a, int grid, hipStream_t stream) {
  const long long lds = phenom_count_lds_bytes(a.t, a.kp, a.tab_lds != 0);
  switch (phenom_choice(a.t)) {
    case 6: return launch(phenom_count_kernel<6>, &a, grid, lds, stream);
    case 7: return launch(phenom_count_kernel<7>, &a, grid, lds, stream);
    case 8: return launch(phenom_count_kernel<8>, &a, grid, lds, stream);
    default: return launch(phenom_count_kernel<0>, &a, grid, lds, stream);
  }
}

hipError_t launch_phenom_window(const PhenomWindowArgs& a, int grid, hipStream_t stream) {
  return launch(phenom_window_kernel, &a, grid, 0, stream);
}

}  // namespace qldpc
