// btsbot_mst_merge: one Boruvka round of the minimum spanning tree of the mutual-reachability graph (gfx950), DESIGN.md
// section 4v.  The searches of a round are the existing grouped k-nearest and radius kernels with the rows' current
// components as groups, and the offers between them -- per row the lightest entry of its lists by (w, index), best_w and
// best_j -- are csrc/mr_offer.hip's (btsbot_mst_offer_knn, btsbot_mst_offer_csr).  What is here is the merge of a round:
//
//   init    the components' slots
//   reduce  two steps: a 32-bit atomicMin on the weight's bits (weights are >= 0, so the bits order like the values),
//           then a 64-bit atomicMin on (lo << 32 | hi) among the rows that offer that weight
//   hook    per component, its edge: lock-free union on int32 parents (csrc/components.hip's rule: a root is only ever
//           hooked under a SMALLER root, so every chain ends); the thread whose compare-and-swap joined two trees appends
//           the edge through an atomic cursor, an edge whose ends are joined already (tied choices can close a cycle, all
//           of one weight) is dropped
//   relabel comp[i] = the root of i, then parent[i] = comp[i]: the smallest row of the component
// Plain C++ atomics only.
#include "list_row.h"

namespace {

using list_row::NO_KEY;
using list_row::WG;
using list_row::check_count;

__global__ __launch_bounds__(WG) void mst_init_kernel(long n, unsigned* __restrict__ comp_w,
                                                     unsigned long long* __restrict__ comp_edge) {
  const long i = (long)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  comp_w[i] = 0xffffffffu;
  comp_edge[i] = NO_KEY;
}

__device__ __forceinline__ bool offers(const int32_t* best_j, const int64_t* comp, long i, long n, long* c) {
  const int32_t j = best_j[i];
  *c = (long)comp[i];
  return j >= 0 && j < n && *c >= 0 && *c < n;
}

__global__ __launch_bounds__(WG) void mst_reduce_w_kernel(const float* __restrict__ best_w, const int32_t* __restrict__ best_j,
                                                         const int64_t* __restrict__ comp, long n, unsigned* comp_w) {
  const long i = (long)blockIdx.x * WG + threadIdx.x;
  long c;
  if (i >= n || !offers(best_j, comp, i, n, &c)) return;
  atomicMin(comp_w + c, __float_as_uint(best_w[i]));
}

__global__ __launch_bounds__(WG) void mst_reduce_edge_kernel(const float* __restrict__ best_w,
                                                            const int32_t* __restrict__ best_j,
                                                            const int64_t* __restrict__ comp, long n,
                                                            const unsigned* __restrict__ comp_w,
                                                            unsigned long long* comp_edge) {
  const long i = (long)blockIdx.x * WG + threadIdx.x;
  long c;
  if (i >= n || !offers(best_j, comp, i, n, &c)) return;
  if (__float_as_uint(best_w[i]) != comp_w[c]) return;
  const unsigned a = (unsigned)i, b = (unsigned)best_j[i];
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  atomicMin(comp_edge + c, ((unsigned long long)lo << 32) | hi);
}

__device__ __forceinline__ int find_root(const int* parent, int x) {
  for (;;) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}

__global__ __launch_bounds__(WG) void mst_hook_kernel(const unsigned* __restrict__ comp_w,
                                                     const unsigned long long* __restrict__ comp_edge, long n, int* parent,
                                                     int64_t* __restrict__ edges, float* __restrict__ weights,
                                                     long capacity, int* cursor) {
  const long c = (long)blockIdx.x * WG + threadIdx.x;
  if (c >= n) return;
  const unsigned long long key = comp_edge[c];
  if (key == NO_KEY) return;
  const long lo = (long)(key >> 32), hi = (long)(key & 0xffffffffull);
  if (lo >= n || hi >= n) return;
  int a = (int)lo, b = (int)hi;
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;   // joined already: the edge would close a cycle
    const int big = a > b ? a : b, small = a > b ? b : a;
    if (atomicCAS(parent + big, big, small) == big) break;
    // (big is no root any more: somebody hooked it; both finds continue from where they stand)
  }
  const int slot = atomicAdd(cursor, 1);
  if (slot < 0 || slot >= capacity) return;   // (a forest of n rows holds fewer than n edges: it cannot happen)
  edges[2 * (long)slot] = lo;
  edges[2 * (long)slot + 1] = hi;
  weights[slot] = __uint_as_float(comp_w[c]);
}

__global__ __launch_bounds__(WG) void mst_relabel_kernel(const int* __restrict__ parent, long n, int64_t* __restrict__ comp) {
  const long i = (long)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  int x = parent[i];
  for (int p = parent[x]; p != x; p = parent[x]) x = p;
  comp[i] = x;
}

__global__ __launch_bounds__(WG) void mst_flatten_kernel(const int64_t* __restrict__ comp, long n, int* __restrict__ parent) {
  const long i = (long)blockIdx.x * WG + threadIdx.x;
  if (i < n) parent[i] = (int)comp[i];
}

}  // namespace

extern "C" int btsbot_mst_merge(const float* best_w, const int32_t* best_j, int64_t n, int64_t* comp, int32_t* parent,
                                uint32_t* comp_w, uint64_t* comp_edge, int64_t* edges, float* weights,
                                int64_t edge_capacity, int32_t* cursor, void* stream) {
  TRY(check_count("btsbot_mst_merge", "n", n));
  if (n == 0) return BTSBOT_OK;
  if (best_w == nullptr || best_j == nullptr || comp == nullptr || parent == nullptr || comp_w == nullptr ||
      comp_edge == nullptr || edges == nullptr || weights == nullptr || cursor == nullptr || edge_capacity < 0) {
    btsbot_set_error("btsbot_mst_merge: NULL argument, or a negative edge_capacity");
    return BTSBOT_ERR_INVALID_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n + WG - 1) / WG)), block(WG);
  unsigned long long* ce = reinterpret_cast<unsigned long long*>(comp_edge);
  hipLaunchKernelGGL(mst_init_kernel, grid, block, 0, s, (long)n, comp_w, ce);
  hipLaunchKernelGGL(mst_reduce_w_kernel, grid, block, 0, s, best_w, best_j, (const int64_t*)comp, (long)n, comp_w);
  hipLaunchKernelGGL(mst_reduce_edge_kernel, grid, block, 0, s, best_w, best_j, (const int64_t*)comp, (long)n,
                     (const unsigned*)comp_w, ce);
  hipLaunchKernelGGL(mst_hook_kernel, grid, block, 0, s, (const unsigned*)comp_w, (const unsigned long long*)ce, (long)n,
                     parent, edges, weights, (long)edge_capacity, cursor);
  hipLaunchKernelGGL(mst_relabel_kernel, grid, block, 0, s, (const int*)parent, (long)n, comp);
  hipLaunchKernelGGL(mst_flatten_kernel, grid, block, 0, s, (const int64_t*)comp, (long)n, parent);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
