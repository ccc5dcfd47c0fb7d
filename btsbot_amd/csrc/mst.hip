// btsbot_mst_*: one Boruvka round of the minimum spanning tree of the mutual-reachability graph (gfx950), DESIGN.md
// section 4v.  The searches of a round are the existing grouped k-nearest and radius kernels with the rows' current
// components as groups; what is new here is what stands between them:
//
//   offer_knn   per row, the lightest entry of its list of the search_k nearest rows of OTHER components by (w, index),
//               w = max(dist, core(row), core(entry)), and whether the list proves it the lightest of all: the list is
//               not full (it holds every eligible row), or w_best <= max(floor, core(row)) where floor bounds the distance
//               of every row the list does not hold from below (the last entry's distance, less the slack of a search
//               that ranks its candidates by another form).  Otherwise the row is UNRESOLVED and w_best is a radius that
//               contains the lightest.
//   offer_csr   the same minimum over the radius lists of the unresolved rows
//   merge       init    the components' slots
//               reduce  two steps: a 32-bit atomicMin on the weight's bits (weights are >= 0, so the bits order like the
//                       values), then a 64-bit atomicMin on (lo << 32 | hi) among the rows that offer that weight
//               hook    per component, its edge: lock-free union on int32 parents (csrc/components.hip's rule: a root is
//                       only ever hooked under a SMALLER root, so every chain ends); the thread whose compare-and-swap
//                       joined two trees appends the edge through an atomic cursor, an edge whose ends are joined already
//                       (tied choices can close a cycle, all of one weight) is dropped
//               relabel comp[i] = the root of i, then parent[i] = comp[i]: the smallest row of the component
// W lanes hold a row of a list, as in csrc/lof.hip.  Plain C++ atomics only.
#include "common.h"
#include "mst_key.h"

namespace {

constexpr int MST_MAX_K = 64;
constexpr int WG = 256;
using offer::NO_KEY;
using offer::group_min_u64;
using offer::offer_key;

template <int W>
__global__ __launch_bounds__(WG) void mst_offer_knn_kernel(const int64_t* __restrict__ idx, const float* __restrict__ dist,
                                                          long n, int k, const float* __restrict__ core,
                                                          const float* __restrict__ slack, int squared, float rel,
                                                          float* __restrict__ best_w, int32_t* __restrict__ best_j,
                                                          uint8_t* __restrict__ unresolved) {
  const int c = threadIdx.x % W;
  const long row = (long)blockIdx.x * (WG / W) + threadIdx.x / W;
  if (row >= n) return;   // (a whole group leaves together)
  const long j = c < k ? (long)idx[row * k + c] : -1;
  const bool present = j >= 0 && j < n;
  const float d = c < k ? dist[row * k + c] : 0.0f;
  const float core_row = core[row];
  unsigned long long key = NO_KEY;
  if (present && d == d) key = offer_key(d, core_row, core[j], j);
  key = group_min_u64<W>(key);
  // the list is full when its last column is present; its distance is the largest of the list
  const long j_last = (long)idx[row * k + k - 1];
  const bool full = j_last >= 0 && j_last < n;
  if (c != 0) return;
  if (key == NO_KEY) {
    best_w[row] = __uint_as_float(0x7f800000u);
    best_j[row] = -1;
    unresolved[row] = 0;
    return;
  }
  const float w = __uint_as_float((unsigned)(key >> 32));
  best_w[row] = w;
  best_j[row] = (int32_t)(unsigned)(key & 0xffffffffull);
  bool open = false;
  if (full) {
    const double d_last = (double)dist[row * k + k - 1];
    double floor_d = d_last;
    if (slack != nullptr) {
      const double s = (double)slack[row];
      floor_d = squared ? sqrt(fmax(d_last * d_last - s, 0.0)) : d_last - s;
    }
    floor_d *= 1.0 - (double)rel;   // the direct form's own error on both distances (0: the search ranks by it)
    open = !((double)w <= fmax(floor_d, (double)core_row));
  }
  unresolved[row] = open ? 1 : 0;
}

__global__ __launch_bounds__(WG) void mst_offer_csr_kernel(const int64_t* __restrict__ indptr,
                                                          const int64_t* __restrict__ indices,
                                                          const float* __restrict__ dist, const int64_t* __restrict__ rows,
                                                          long m, long n, const float* __restrict__ core,
                                                          float* __restrict__ best_w, int32_t* __restrict__ best_j) {
  const int lane = threadIdx.x & 63;
  const long u = (long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
  if (u >= m) return;
  const long row = (long)rows[u];
  if (row < 0 || row >= n) return;
  const float core_row = core[row];
  unsigned long long key = NO_KEY;
  const long long e1 = indptr[u + 1];
  for (long long e = indptr[u] + lane; e < e1; e += 64) {
    const long j = (long)indices[e];
    const float d = dist[e];
    if (j < 0 || j >= n || d != d) continue;
    const unsigned long long t = offer_key(d, core_row, core[j], j);
    key = t < key ? t : key;
  }
  key = group_min_u64<64>(key);
  if (lane != 0 || key == NO_KEY) return;
  const int32_t old_j = best_j[row];
  const unsigned long long old =
      old_j < 0 ? NO_KEY : (((unsigned long long)__float_as_uint(best_w[row]) << 32) | (unsigned)old_j);
  if (key < old) {
    best_w[row] = __uint_as_float((unsigned)(key >> 32));
    best_j[row] = (int32_t)(unsigned)(key & 0xffffffffull);
  }
}

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

int check_rows(const char* who, int64_t n) {
  if (n < 0 || n > 0x7fffffffLL) {
    btsbot_set_error("%s: n=%lld must be in 0 .. 2^31 - 1", who, (long long)n);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

template <int W>
void launch_offer_knn(const int64_t* idx, const float* dist, long n, int k, const float* core, const float* slack,
                      int squared, float rel, float* best_w, int32_t* best_j, uint8_t* unresolved, hipStream_t s) {
  hipLaunchKernelGGL(mst_offer_knn_kernel<W>, dim3((unsigned)((n + WG / W - 1) / (WG / W))), dim3(WG), 0, s, idx, dist, n,
                     k, core, slack, squared, rel, best_w, best_j, unresolved);
}

}  // namespace

extern "C" int btsbot_mst_offer_knn(const int64_t* idx, const float* dist, int64_t n, int k, const float* core,
                                    const float* slack, int slack_is_squared, float rel, float* best_w, int32_t* best_j,
                                    uint8_t* unresolved, void* stream) {
  TRY(check_rows("btsbot_mst_offer_knn", n));
  if (k < 1 || k > MST_MAX_K || !(rel >= 0.0f && rel < 1.0f)) {
    btsbot_set_error("btsbot_mst_offer_knn: k=%d must be in 1..%d and rel=%g in [0, 1)", k, MST_MAX_K, (double)rel);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n == 0) return BTSBOT_OK;
  if (idx == nullptr || dist == nullptr || core == nullptr || best_w == nullptr || best_j == nullptr ||
      unresolved == nullptr) {
    btsbot_set_error("btsbot_mst_offer_knn: NULL argument (only slack may be NULL)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  if (k <= 16)
    launch_offer_knn<16>(idx, dist, (long)n, k, core, slack, slack_is_squared, rel, best_w, best_j, unresolved, s);
  else if (k <= 32)
    launch_offer_knn<32>(idx, dist, (long)n, k, core, slack, slack_is_squared, rel, best_w, best_j, unresolved, s);
  else
    launch_offer_knn<64>(idx, dist, (long)n, k, core, slack, slack_is_squared, rel, best_w, best_j, unresolved, s);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_mst_offer_csr(const int64_t* indptr, const int64_t* indices, const float* dist, const int64_t* rows,
                                    int64_t m, int64_t n, const float* core, float* best_w, int32_t* best_j,
                                    void* stream) {
  TRY(check_rows("btsbot_mst_offer_csr", n));
  TRY(check_rows("btsbot_mst_offer_csr", m));
  if (m == 0 || n == 0) return BTSBOT_OK;
  if (indptr == nullptr || rows == nullptr || core == nullptr || best_w == nullptr || best_j == nullptr) {
    btsbot_set_error("btsbot_mst_offer_csr: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(mst_offer_csr_kernel, dim3((unsigned)((m + WG / 64 - 1) / (WG / 64))), dim3(WG), 0,
                     (hipStream_t)stream, indptr, indices, dist, rows, (long)m, (long)n, core, best_w, best_j);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_mst_merge(const float* best_w, const int32_t* best_j, int64_t n, int64_t* comp, int32_t* parent,
                                uint32_t* comp_w, uint64_t* comp_edge, int64_t* edges, float* weights,
                                int64_t edge_capacity, int32_t* cursor, void* stream) {
  TRY(check_rows("btsbot_mst_merge", n));
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
