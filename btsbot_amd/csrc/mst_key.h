// (w, j) of a mutual-reachability offer as one 64-bit key, and its minimum over the W lanes that hold a row of a list:
// what csrc/mst.hip (a row of the bank among the others) and csrc/hdbscan_predict.hip (a new row against the bank) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace offer {

constexpr unsigned long long NO_KEY = ~0ull;

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o, int w) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(v & 0xffffffffull), o, w);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, w);
  return ((unsigned long long)hi << 32) | lo;
}

template <int W>
__device__ __forceinline__ unsigned long long group_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) {
    const unsigned long long t = shfl_xor_u64(v, o, W);
    v = t < v ? t : v;
  }
  return v;
}

// (w, j) as one key: the bits of a float >= 0 (+inf included) order like the value
__device__ __forceinline__ unsigned long long offer_key(float d, float core_row, float core_j, long j) {
  float w = fmaxf(d, fmaxf(core_row, core_j));
  w = w > 0.0f ? w : 0.0f;   // (1 - cos may round below 0; -0 would not order by its bits)
  return ((unsigned long long)__float_as_uint(w) << 32) | (unsigned)j;
}

}  // namespace offer
