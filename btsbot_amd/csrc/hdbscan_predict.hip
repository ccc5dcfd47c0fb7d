// btsbot_cluster_assign: which cluster of a fitted HDBSCAN tree a NEW row belongs to (gfx950), DESIGN.md section 4w.  The
// searches are the existing k-nearest and radius kernels against the bank, and the offers that follow them -- per query
// row its core distance and its nearest mutual-reachability neighbour, best_w and best_j, the smallest (w, index) of ALL
// eligible bank rows -- are csrc/mr_offer.hip's (btsbot_cluster_offer_knn, btsbot_cluster_offer_csr).  What is here:
//
//   assign      lambda_q = 1 / w_best (lam_zero at 0), the walk from the neighbour's cluster up to the cluster alive at
//               lambda_q, its label, the membership strength and the GLOSH score
// Every float operation of assign is one correctly rounded IEEE operation (max, 1 / x, min, one division, one
// subtraction; contraction is off), so the lists' fp32 distances determine the answer bit for bit.
// Plain C++ and vector stores only.
#include "list_row.h"

#pragma clang fp contract(off)

namespace {

using list_row::WG;
using list_row::check_count;

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

}  // namespace

extern "C" int btsbot_cluster_assign(const float* best_w, const int32_t* best_j, int64_t n_query, int64_t n,
                                     const int32_t* row_cluster, const double* row_lambda, int64_t n_clusters,
                                     const int32_t* parent, const double* birth, const int32_t* label,
                                     const double* max_lambda, const double* death, double lam_zero, int64_t* out_label,
                                     double* out_prob, double* out_outlier, double* out_lambda, int64_t* out_cluster,
                                     int64_t* out_neighbor, void* stream) {
  const char* who = "btsbot_cluster_assign";
  TRY(check_count(who, "n_query", n_query));
  TRY(check_count(who, "n", n));
  TRY(check_count(who, "n_clusters", n_clusters));
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
