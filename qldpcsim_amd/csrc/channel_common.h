// channel_common.h — device helpers the shot sources and outcome counters
// share (channel_kernels.hip, phenom_kernels.hip): the counter-based
// generator and the logical-operator product.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qldpc {

// Philox4x32-10 (Salmon et al., SC'11), counter (c0..c3), key (k0, k1).
__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                               uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one v_mad_u64_u32 per product (hi and lo together)
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// Lz·rX (or Lx·rZ) mod 2 for one shot: lane l owns logical rows l, l + 64, ...
// of the word-major table `tab` ([W][kp]: consecutive lanes read consecutive
// 8-byte words, so a 32-lane half covers all 64 banks once; r[w] is one
// broadcast read), XOR-accumulates tab[w][i] & r[w] over the W residual words
// and takes the popcount parity; a ballot makes each flip word. Padding rows
// of the table are zero, so bits above k are. Lane g returns word g.
__device__ __forceinline__ uint64_t logical_flips(const uint64_t* tab, const uint64_t* r, int W, int kp, int lane,
                                                  bool* any) {
  uint64_t mine = 0;
  bool nz = false;
  for (int i0 = 0; i0 < kp; i0 += 64) {
    const uint64_t* col = tab + i0 + lane;
    uint64_t x = 0;
#pragma unroll 4
    for (int w = 0; w < W; ++w) x ^= col[(size_t)w * kp] & r[w];
    const uint64_t bits = __ballot(__popcll(x) & 1);
    nz |= bits != 0;
    if (lane == (i0 >> 6)) mine = bits;
  }
  *any = nz;
  return mine;
}

}  // namespace qldpc
