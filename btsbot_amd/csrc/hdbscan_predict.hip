// btsbot_cluster_*: which cluster of a fitted HDBSCAN tree a NEW row belongs to (gfx950), DESIGN.md section 4w.  The
// searches are the existing k-nearest and radius kernels against the bank; what is new here is what follows them:
//
//   offer_knn   per query row, its core distance -- the distance of its (min_samples - 1)-th nearest eligible bank row,
//               column core_col of its list, 0 for core_col < 0, +inf where that column is absent --, the lightest entry
//               of its list by (w, index), w = max(dist, core(q), core(b)), and whether the list proves it the smallest
//               (w, index) of ALL eligible bank rows: the list is not full (it holds every eligible row), or w_best <
//               floor, where floor bounds the distance of every row the list does not hold from below (the last entry's
//               distance, less the slack of a search that ranks its candidates by another form).  The comparison is
//               STRICT, unlike csrc/mst.hip's: a spanning tree may take any of several equally light edges, a prediction
//               may not -- two bank rows at one weight can lie in different clusters --, and a row the list does not hold
//               may tie the weight at a smaller index.  Otherwise the row is UNRESOLVED and w_best is a radius that
//               contains the answer.
//   offer_csr   the same minimum over the radius lists of the unresolved rows
//   assign      lambda_q = 1 / w_best (lam_zero at 0), the walk from the neighbour's cluster up to the cluster alive at
//               lambda_q, its label, the membership strength and the GLOSH score
// Every float operation of assign is one correctly rounded IEEE operation (max, 1 / x, min, one division, one
// subtraction; contraction is off), so the lists' fp32 distances determine the answer bit for bit.
// W lanes hold a row of a list, as in csrc/lof.hip and csrc/mst.hip.  Plain C++ and vector stores only.
#include "common.h"
#include "mst_key.h"

#pragma clang fp contract(off)

namespace {

using offer::NO_KEY;
using offer::group_min_u64;
using offer::offer_key;

constexpr int CLUSTER_MAX_K = 64;
constexpr int WG = 256;
constexpr unsigned INF_BITS = 0x7f800000u, NAN_BITS = 0x7fc00000u;

template <int W>
__global__ __launch_bounds__(WG) void cluster_offer_knn_kernel(const int64_t* __restrict__ idx, const float* __restrict__ dist,
                                                              long nq, int k, long n, int core_col,
                                                              const float* __restrict__ core, const float* __restrict__ slack,
                                                              int squared, float rel, float* __restrict__ core_q,
                                                              float* __restrict__ best_w, int32_t* __restrict__ best_j,
                                                              uint8_t* __restrict__ unresolved) {
  const int c = threadIdx.x % W;
  const long row = (long)blockIdx.x * (WG / W) + threadIdx.x / W;
  if (row >= nq) return;   // (a whole group leaves together)
  const long j = c < k ? (long)idx[row * k + c] : -1;
  const bool present = j >= 0 && j < n;
  const float d = c < k ? dist[row * k + c] : 0.0f;
  const float d_first = dist[row * k];
  float core_row = 0.0f;
  if (core_col >= 0) {
    const long j_core = (long)idx[row * k + core_col];
    core_row = j_core >= 0 && j_core < n ? dist[row * k + core_col] : __uint_as_float(INF_BITS);
  }
  unsigned long long key = NO_KEY;
  if (present && d == d) key = offer_key(d, core_row, core[j], j);
  key = group_min_u64<W>(key);
  // the list is full when its last column is present; its distance is the largest of the list
  const long j_last = (long)idx[row * k + k - 1];
  const bool full = j_last >= 0 && j_last < n;
  if (c != 0) return;
  unresolved[row] = 0;
  if (d_first != d_first) {   // a non-finite query row: the search answers -1 / NaN throughout
    core_q[row] = best_w[row] = __uint_as_float(NAN_BITS);
    best_j[row] = -1;
    return;
  }
  core_q[row] = core_row;
  if (key == NO_KEY || !(core_row < __uint_as_float(INF_BITS))) {   // no eligible row, or fewer than min_samples - 1
    best_w[row] = __uint_as_float(INF_BITS);
    best_j[row] = -1;
    return;
  }
  const float w = __uint_as_float((unsigned)(key >> 32));
  best_w[row] = w;
  best_j[row] = (int32_t)(unsigned)(key & 0xffffffffull);
  if (!full) return;
  const double d_last = (double)dist[row * k + k - 1];
  double floor_d = d_last;
  if (slack != nullptr) {
    const double s = (double)slack[row];
    floor_d = squared ? sqrt(fmax(d_last * d_last - s, 0.0)) : d_last - s;
  }
  floor_d *= 1.0 - (double)rel;   // the direct form's own error on both distances (0: the search ranks by it)
  unresolved[row] = (double)w < floor_d ? 0 : 1;
}

__global__ __launch_bounds__(WG) void cluster_offer_csr_kernel(const int64_t* __restrict__ indptr,
                                                              const int64_t* __restrict__ indices,
                                                              const float* __restrict__ dist, const int64_t* __restrict__ rows,
                                                              long m, long nq, long n, const float* __restrict__ core,
                                                              const float* __restrict__ core_q, float* __restrict__ best_w,
                                                              int32_t* __restrict__ best_j) {
  const int lane = threadIdx.x & 63;
  const long u = (long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
  if (u >= m) return;
  const long row = (long)rows[u];
  if (row < 0 || row >= nq) return;
  const float core_row = core_q[row];
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

__global__ __launch_bounds__(WG) void cluster_assign_kernel(
    const float* __restrict__ best_w, const int32_t* __restrict__ best_j, long nq, long n,
    const int32_t* __restrict__ row_cluster, const double* __restrict__ row_lambda, int nc,
    const int32_t* __restrict__ parent, const double* __restrict__ birth, const int32_t* __restrict__ label,
    const double* __restrict__ max_lambda, const double* __restrict__ death, double lam_zero,
    int64_t* __restrict__ out_label, double* __restrict__ out_prob, double* __restrict__ out_outlier,
    double* __restrict__ out_lambda, int64_t* __restrict__ out_cluster, int64_t* __restrict__ out_neighbor) {
  const long i = (long)blockIdx.x * WG + threadIdx.x;
  if (i >= nq) return;
  const float w = best_w[i];
  const long b = (long)best_j[i];
  int c = b >= 0 && b < n ? row_cluster[b] : -1;
  if (w != w || c < 0 || c >= nc) {   // a non-finite row (NaN), or a row without a neighbour (w = +inf)
    const bool bad = w != w;
    out_label[i] = -1;
    out_prob[i] = 0.0;
    out_outlier[i] = bad ? (double)w : 1.0;
    out_lambda[i] = bad ? (double)w : 0.0;
    out_cluster[i] = -1;
    out_neighbor[i] = -1;
    return;
  }
  const double lam = w == 0.0f ? lam_zero : 1.0 / (double)w;
  if (row_lambda[b] > lam) {
    for (int step = 0; step < nc; ++step) {   // (a parent stands before its children: at most nc - 1 steps)
      const int p = parent[c];
      if (p < 0 || p >= c || !(birth[c] >= lam)) break;
      c = p;
    }
  }
  const int lab = label[c];
  const double m = max_lambda[c], dth = death[c];
  out_label[i] = lab;
  out_prob[i] = lab < 0 ? 0.0 : (m == 0.0 ? 1.0 : fmin(lam, m) / m);
  out_outlier[i] = dth == 0.0 ? 0.0 : 1.0 - fmin(lam, dth) / dth;
  out_lambda[i] = lam;
  out_cluster[i] = c;
  out_neighbor[i] = b;
}

int check_rows(const char* who, const char* name, int64_t n) {
  if (n < 0 || n > 0x7fffffffLL) {
    btsbot_set_error("%s: %s=%lld must be in 0 .. 2^31 - 1", who, name, (long long)n);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

template <int W>
void launch_offer_knn(const int64_t* idx, const float* dist, long nq, int k, long n, int core_col, const float* core,
                      const float* slack, int squared, float rel, float* core_q, float* best_w, int32_t* best_j,
                      uint8_t* unresolved, hipStream_t s) {
  hipLaunchKernelGGL(cluster_offer_knn_kernel<W>, dim3((unsigned)((nq + WG / W - 1) / (WG / W))), dim3(WG), 0, s, idx, dist,
                     nq, k, n, core_col, core, slack, squared, rel, core_q, best_w, best_j, unresolved);
}

}  // namespace

extern "C" int btsbot_cluster_offer_knn(const int64_t* idx, const float* dist, int64_t n_query, int k, int64_t n,
                                        int min_samples, const float* core, const float* slack, int slack_is_squared,
                                        float rel, float* core_q, float* best_w, int32_t* best_j, uint8_t* unresolved,
                                        void* stream) {
  const char* who = "btsbot_cluster_offer_knn";
  TRY(check_rows(who, "n_query", n_query));
  TRY(check_rows(who, "n", n));
  if (k < 1 || k > CLUSTER_MAX_K || min_samples < 1 || min_samples - 1 > k || !(rel >= 0.0f && rel < 1.0f)) {
    btsbot_set_error("%s: k=%d must be in 1..%d, min_samples=%d in 1..k + 1 and rel=%g in [0, 1)", who, k, CLUSTER_MAX_K,
                     min_samples, (double)rel);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query == 0) return BTSBOT_OK;
  if (idx == nullptr || dist == nullptr || (n > 0 && core == nullptr) || core_q == nullptr || best_w == nullptr ||
      best_j == nullptr || unresolved == nullptr) {
    btsbot_set_error("%s: NULL argument (only slack may be NULL)", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  const int col = min_samples - 2;   // -1: min_samples = 1, a core distance of 0
  if (k <= 16)
    launch_offer_knn<16>(idx, dist, (long)n_query, k, (long)n, col, core, slack, slack_is_squared, rel, core_q, best_w,
                         best_j, unresolved, s);
  else if (k <= 32)
    launch_offer_knn<32>(idx, dist, (long)n_query, k, (long)n, col, core, slack, slack_is_squared, rel, core_q, best_w,
                         best_j, unresolved, s);
  else
    launch_offer_knn<64>(idx, dist, (long)n_query, k, (long)n, col, core, slack, slack_is_squared, rel, core_q, best_w,
                         best_j, unresolved, s);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_cluster_offer_csr(const int64_t* indptr, const int64_t* indices, const float* dist,
                                        const int64_t* rows, int64_t m, int64_t n_query, int64_t n, const float* core,
                                        const float* core_q, float* best_w, int32_t* best_j, void* stream) {
  const char* who = "btsbot_cluster_offer_csr";
  TRY(check_rows(who, "m", m));
  TRY(check_rows(who, "n_query", n_query));
  TRY(check_rows(who, "n", n));
  if (m == 0 || n_query == 0 || n == 0) return BTSBOT_OK;
  if (indptr == nullptr || rows == nullptr || core == nullptr || core_q == nullptr || best_w == nullptr ||
      best_j == nullptr) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(cluster_offer_csr_kernel, dim3((unsigned)((m + WG / 64 - 1) / (WG / 64))), dim3(WG), 0,
                     (hipStream_t)stream, indptr, indices, dist, rows, (long)m, (long)n_query, (long)n, core, core_q,
                     best_w, best_j);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_cluster_assign(const float* best_w, const int32_t* best_j, int64_t n_query, int64_t n,
                                     const int32_t* row_cluster, const double* row_lambda, int64_t n_clusters,
                                     const int32_t* parent, const double* birth, const int32_t* label,
                                     const double* max_lambda, const double* death, double lam_zero, int64_t* out_label,
                                     double* out_prob, double* out_outlier, double* out_lambda, int64_t* out_cluster,
                                     int64_t* out_neighbor, void* stream) {
  const char* who = "btsbot_cluster_assign";
  TRY(check_rows(who, "n_query", n_query));
  TRY(check_rows(who, "n", n));
  TRY(check_rows(who, "n_clusters", n_clusters));
  if (!(lam_zero > 0.0)) {
    btsbot_set_error("%s: lam_zero=%g must be > 0", who, lam_zero);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query == 0) return BTSBOT_OK;
  if (best_w == nullptr || best_j == nullptr || out_label == nullptr || out_prob == nullptr || out_outlier == nullptr ||
      out_lambda == nullptr || out_cluster == nullptr || out_neighbor == nullptr ||
      (n > 0 && (row_cluster == nullptr || row_lambda == nullptr)) ||
      (n_clusters > 0 && (parent == nullptr || birth == nullptr || label == nullptr || max_lambda == nullptr ||
                          death == nullptr))) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(cluster_assign_kernel, dim3((unsigned)((n_query + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream,
                     best_w, best_j, (long)n_query, (long)n, row_cluster, row_lambda, (int)n_clusters, parent, birth, label,
                     max_lambda, death, lam_zero, out_label, out_prob, out_outlier, out_lambda, out_cluster, out_neighbor);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
