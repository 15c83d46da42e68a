// wave_common.h — device primitives every kernel file shares, free of any
// kernel's argument struct: the wave-level phase barrier, ballots, LDS and
// constant-address-space access and the persistent half-shot queue
// (DESIGN.md §3.6).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qldpc {

// Kernel selectors: the pointer, and the kernel's name as rocprofv3 reports it
// (bench.py matches profiles by name).
#define QLDPC_NAMED(ptr, str) do { if (name) *name = str; return (const void*)ptr; } while (0)

__device__ __forceinline__ void wave_sync() {
  // Lanes of one wave exchange data through LDS between phases. DS
  // instructions of a wave complete in order; the fences only stop the
  // compiler from moving LDS accesses across the phase boundary.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t ballot(int pred) { return __ballot(pred); }
// the same from a bool: the wave's compare mask itself (s_and with exec). The
// int form above materialises the predicate (v_cndmask) and compares it again
// (v_cmp_ne) — two VALU ops per ballot, kept where the code is profiled as is.
__device__ __forceinline__ uint64_t ballot_b(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }

// LDS (address space 3) access through a 32-bit byte address held in a VGPR
// (ds_read / ds_write directly; a generic pointer would become flat_load).
#define QLDPC_LDS(T, addr) ((__attribute__((address_space(3))) T*)(uintptr_t)(uint32_t)(addr))
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)p;
}

// Read-only kernel inputs through the constant address space: with a
// wave-uniform index the compiler issues scalar loads (through a generic
// pointer it must assume the kernel's own stores alias them).
template <typename T>
__device__ __forceinline__ T ld_const(const T* p, long long i) {
  return ((const __attribute__((address_space(4))) T*)p)[i];
}

// Persistent half-shot loop. Each wave starts with one static half-shot;
// with a queue, further work comes from a global ticket counter in guided
// chunks (about remaining / (4 * waves) consecutive half-shots, at most 64,
// at least 1), claimed with one atomic when the last half-shot of the current
// chunk starts, so its latency is hidden. Early-terminating decodes (channel
// syndromes: most stop after 1-3 iterations, a few run max_iter) then
// balance across waves instead of leaving a long tail, and the counter sees
// O(waves * log) atomics rather than one per half-shot.
// A wave-uniform 64-bit value the compiler may not prove uniform: pinning it
// to scalar registers keeps the queue state out of VGPRs (the headline kernel
// had spilled it to scratch memory at its 168-VGPR budget).
__device__ __forceinline__ long long uniform64(long long x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)x);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (long long)(((uint64_t)hi << 32) | lo);
}

struct HalfShotQueue {
  long long hs, end, stride, batch;
  uint32_t* q;
  uint32_t tk, tlen, seen;
  __device__ __forceinline__ HalfShotQueue(long long batch_, uint32_t* queue, int waves, int wid)
      : hs(uniform64((long long)blockIdx.x * waves + wid)), end(0), stride((long long)gridDim.x * waves),
        batch(batch_), q(queue), tk(0), tlen(1), seen(0) {
    end = hs + 1;
  }
  __device__ __forceinline__ void prefetch(int lane) {
    if (q && hs + 1 == end) {                       // last of this chunk: claim the next
      const long long rem = batch - stride - (long long)seen;
      long long len = rem / (4 * stride);
      len = len < 1 ? 1 : (len > 64 ? 64 : len);
      tlen = (uint32_t)len;
      if (lane == 0) tk = atomicAdd(q, tlen);
    }
  }
  __device__ __forceinline__ void advance() {
    if (!q) {
      hs = uniform64(hs + stride);
      return;
    }
    hs = uniform64(hs + 1);
    if (hs < end) return;
    const uint32_t t = __builtin_amdgcn_readfirstlane(tk);
    seen = t + tlen;
    hs = uniform64(stride + (long long)t);
    end = uniform64(hs + tlen);
  }
};

}  // namespace qldpc
