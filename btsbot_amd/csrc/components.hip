// btsbot_graph_components / btsbot_dbscan_labels: connected components of a CSR graph and the DBSCAN labelling rule
// (gfx950), DESIGN.md section 4p.
//
// Components: lock-free union-find on int32 parents.  parent[i] <= i always holds -- a root is only ever hooked under a
// SMALLER root -- so the chains end, every find terminates whatever the other threads do, and the root a component ends
// with is its smallest row index: a function of the graph alone, not of the schedule.
//   init     parent[i] = i (a row the mask passes) or -1
//   hook     one wave per row, the lanes stride over its neighbours: for an edge (u, v) whose both ends pass the mask,
//            find both roots; equal: done; else atomicCAS(parent[larger], larger, smaller).  The CAS fails only when
//            another thread hooked that root meanwhile; then the roots are looked up again.  Nothing waits for another
//            workgroup: every retry follows somebody else's progress (the parent of `larger` went down).
//   flatten  root[i] = the end of i's chain (into the int64 output: the parents are not written while they are read)
// An edge joins its ends whichever row's list holds it.
//
// Labels: one wave per row.  A core row takes its component's number; any other row the smallest number among its core
// neighbours (clusters are numbered in the order of their smallest core row, so that is the component with the smallest
// root), or -1 -- sklearn.cluster.DBSCAN's labels, made independent of the visiting order.
#include "list_row.h"

namespace {

__device__ __forceinline__ int find_root(const int* parent, int x) {
  for (;;) {
    const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}

__global__ __launch_bounds__(256) void cc_init_kernel(const unsigned char* __restrict__ mask, long n,
                                                      int* __restrict__ parent) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) parent[i] = mask == nullptr || mask[i] != 0 ? (int)i : -1;
}

__global__ __launch_bounds__(256) void cc_hook_kernel(const long long* __restrict__ indptr,
                                                      const long long* __restrict__ indices,
                                                      const unsigned char* __restrict__ mask, long n, int* parent) {
  const int lane = threadIdx.x & 63;
  const long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n || (mask != nullptr && mask[u] == 0)) return;
  const long long e1 = indptr[u + 1];
  for (long long e = indptr[u] + lane; e < e1; e += 64) {
    const long long v = indices[e];
    if (v < 0 || v >= n || v == u || (mask != nullptr && mask[v] == 0)) continue;
    int a = (int)u, b = (int)v;
    for (;;) {
      a = find_root(parent, a);
      b = find_root(parent, b);
      if (a == b) break;
      const int hi = a > b ? a : b, lo = a > b ? b : a;
      if (atomicCAS(parent + hi, hi, lo) == hi) break;
      // (hi is no root any more: somebody hooked it; both finds continue from where they stand)
    }
  }
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, long n,
                                                         long long* __restrict__ root) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int x = parent[i];
  if (x >= 0) {
    for (int p = parent[x]; p != x; p = parent[x]) x = p;
  }
  root[i] = x;
}

__global__ __launch_bounds__(256) void dbscan_label_kernel(const long long* __restrict__ indptr,
                                                           const long long* __restrict__ indices,
                                                           const unsigned char* __restrict__ core,
                                                           const long long* __restrict__ root,
                                                           const long long* __restrict__ cluster, long n,
                                                           long long* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= n) return;
  if (core[u] != 0) {
    const long long r = root[u];
    if (lane == 0) labels[u] = r >= 0 && r < n ? cluster[r] : -1;
    return;
  }
  long long best = 0x7fffffffffffffffLL;
  const long long e1 = indptr[u + 1];
  for (long long e = indptr[u] + lane; e < e1; e += 64) {
    const long long v = indices[e];
    if (v < 0 || v >= n || core[v] == 0) continue;
    const long long r = root[v];
    if (r >= 0 && r < n) best = min(best, cluster[r]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int lo = __shfl_xor((int)(best & 0xffffffffLL), o), hi = __shfl_xor((int)(best >> 32), o);
    best = min(best, (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
  }
  if (lane == 0) labels[u] = best == 0x7fffffffffffffffLL ? -1 : best;
}

using list_row::check_count;

}  // namespace

extern "C" int btsbot_graph_components(const int64_t* indptr, const int64_t* indices, const uint8_t* mask, int64_t n,
                                       int32_t* parent, int64_t* root, void* stream) {
  TRY(check_count("btsbot_graph_components", "n", n));
  if (n == 0) return BTSBOT_OK;
  if (indptr == nullptr || parent == nullptr || root == nullptr) {
    btsbot_set_error("btsbot_graph_components: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const unsigned flat = (unsigned)((n + 255) / 256), waves = (unsigned)((n + 3) / 4);
  hipLaunchKernelGGL(cc_init_kernel, dim3(flat), dim3(256), 0, st, mask, (long)n, parent);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_hook_kernel, dim3(waves), dim3(256), 0, st, reinterpret_cast<const long long*>(indptr),
                     reinterpret_cast<const long long*>(indices), mask, (long)n, parent);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(flat), dim3(256), 0, st, (const int*)parent, (long)n,
                     reinterpret_cast<long long*>(root));
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_dbscan_labels(const int64_t* indptr, const int64_t* indices, const uint8_t* core,
                                    const int64_t* root, const int64_t* cluster, int64_t n, int64_t* labels,
                                    void* stream) {
  TRY(check_count("btsbot_dbscan_labels", "n", n));
  if (n == 0) return BTSBOT_OK;
  if (indptr == nullptr || core == nullptr || root == nullptr || cluster == nullptr || labels == nullptr) {
    btsbot_set_error("btsbot_dbscan_labels: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(dbscan_label_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(indptr), reinterpret_cast<const long long*>(indices), core,
                     reinterpret_cast<const long long*>(root), reinterpret_cast<const long long*>(cluster), (long)n, reinterpret_cast<long long*>(labels));
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
