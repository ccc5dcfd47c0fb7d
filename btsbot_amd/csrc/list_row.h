// W lanes hold a row of a neighbour list, lane c its column c: W = 16, 32 or 64, the smallest that holds k, so that at the
// usual k a wave carries four or two rows and not one.  What the kernels over such lists share -- csrc/lof.hip (sums over a
// row), csrc/mr_offer.hip (the lightest mutual-reachability offer of a row) -- and the host checks of the entry points
// around them: where a row stands, the launch by lane width, the reductions over a row's lanes, and the (w, j) key of an
// offer.
#pragma once
#include <type_traits>

#include "common.h"

namespace list_row {

constexpr int WG = 256;

// ---- where a row stands: WG / W rows per workgroup; a whole group of lanes leaves together at row >= rows
template <int W>
__device__ __forceinline__ int lane_col() {
  return threadIdx.x % W;
}
template <int W>
__device__ __forceinline__ long lane_row() {
  return (long)blockIdx.x * (WG / W) + threadIdx.x / W;
}

inline int lanes_for(int k) { return k <= 16 ? 16 : k <= 32 ? 32 : 64; }
inline dim3 row_grid(long rows, int W) { return dim3((unsigned)((rows + WG / W - 1) / (WG / W))); }

// f(std::integral_constant<int, W>) for W = lanes: for_lanes(lanes_for(k), [&](auto w) { launch<decltype(w)::value>(...); })
template <typename F>
void for_lanes(int lanes, F&& f) {
  switch (lanes) {
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
  }
}

// ---- reductions over the W lanes of a row.  The butterfly o = W/2, W/4, ..., 1 -- v[c] <- v[c] + v[c ^ o] for every c at
// once -- is the order of a row's float64 sum that tests/lof_ref.py (tree_sum) copies: it stays as it is.
template <int W>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, W);
  return v;
}
template <int W>
__device__ __forceinline__ int group_sum_i(int v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, W);
  return v;
}
template <int W>
__device__ __forceinline__ int group_max_i(int v) {
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, W));
  return v;
}

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

// ---- (w, j) of a mutual-reachability offer as one 64-bit key: the bits of a float >= 0 (+inf included) order like the
// value, so the smallest key is the smallest (w, j)
constexpr unsigned long long NO_KEY = ~0ull;

__device__ __forceinline__ unsigned long long offer_key(float d, float core_row, float core_j, long j) {
  float w = fmaxf(d, fmaxf(core_row, core_j));
  w = w > 0.0f ? w : 0.0f;   // (1 - cos may round below 0; -0 would not order by its bits)
  return ((unsigned long long)__float_as_uint(w) << 32) | (unsigned)j;
}

// ---- host checks of the entry points
inline int check_count(const char* who, const char* name, int64_t n) {
  if (n < 0 || n > 0x7fffffffLL) {
    btsbot_set_error("%s: %s=%lld must be in 0 .. 2^31 - 1", who, name, (long long)n);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace list_row
