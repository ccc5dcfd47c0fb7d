// btsbot_mst_offer_* / btsbot_cluster_offer_*: the lightest mutual-reachability offer of a row, from its list (gfx950),
// DESIGN.md sections 4v and 4w.  Two callers, one kernel pair:
//
//   the spanning tree (csrc/mst.hip)       a row of the bank among the rows of OTHER components; its core distance is
//                                          core[row]
//   prediction (csrc/hdbscan_predict.hip)  a NEW row against the bank; its core distance is the distance of its
//                                          (min_samples - 1)-th nearest eligible bank row, column core_col of its own list,
//                                          0 for core_col < 0, +inf where that column is absent, and an output (core_q)
//
//   offer_knn   per row, the lightest entry of its list by (w, index), w = max(dist, core(row), core(entry)), and whether
//               the list proves it the lightest of all: the list is not full (it holds every eligible row), or w_best lies
//               within floor, which bounds the distance of every row the list does not hold from below (the last entry's
//               distance, less the slack of a search that ranks its candidates by another form).  Otherwise the row is
//               UNRESOLVED and w_best is a radius that contains the answer.
//   offer_csr   the same minimum over the radius lists of the unresolved rows
//
// The floor is float64 on the list's fp32 values with the contraction off (prediction's rule, which
// tests/hdbscan_predict_ref.py restates): d * d - s is two roundings.  No answer of the tree depends on it (4v).
// W lanes hold a row of a list (csrc/list_row.h).  Plain C++ and vector stores only.
#include "list_row.h"

#pragma clang fp contract(off)

namespace {

using namespace list_row;

constexpr int OFFER_MAX_K = 64;
constexpr unsigned INF_BITS = 0x7f800000u, NAN_BITS = 0x7fc00000u;

template <int W, bool PREDICT>
__global__ __launch_bounds__(WG) void offer_knn_kernel(const int64_t* __restrict__ idx, const float* __restrict__ dist,
                                                      long rows, int k, long n, int core_col,
                                                      const float* __restrict__ core, const float* __restrict__ slack,
                                                      int squared, float rel, float* __restrict__ core_q,
                                                      float* __restrict__ best_w, int32_t* __restrict__ best_j,
                                                      uint8_t* __restrict__ unresolved) {
  const int c = lane_col<W>();
  const long row = lane_row<W>();
  if (row >= rows) return;   // (a whole group leaves together)
  const long j = c < k ? (long)idx[row * k + c] : -1;
  const bool present = j >= 0 && j < n;
  const float d = c < k ? dist[row * k + c] : 0.0f;
  float core_row, d_first = 0.0f;
  if constexpr (PREDICT) {
    d_first = dist[row * k];
    core_row = 0.0f;
    if (core_col >= 0) {
      const long j_core = (long)idx[row * k + core_col];
      core_row = j_core >= 0 && j_core < n ? dist[row * k + core_col] : __uint_as_float(INF_BITS);
    }
  } else {
    core_row = core[row];
  }
  unsigned long long key = NO_KEY;
  if (present && d == d) key = offer_key(d, core_row, core[j], j);
  key = group_min_u64<W>(key);
  // the list is full when its last column is present; its distance is the largest of the list
  const long j_last = (long)idx[row * k + k - 1];
  const bool full = j_last >= 0 && j_last < n;
  if (c != 0) return;
  bool none = key == NO_KEY;   // no eligible row
  if constexpr (PREDICT) {
    if (d_first != d_first) {   // a non-finite query row: the search answers -1 / NaN throughout
      core_q[row] = best_w[row] = __uint_as_float(NAN_BITS);
      best_j[row] = -1;
      unresolved[row] = 0;
      return;
    }
    core_q[row] = core_row;
    none = none || !(core_row < __uint_as_float(INF_BITS));   // fewer than min_samples - 1 eligible rows
  }
  if (none) {
    best_w[row] = __uint_as_float(INF_BITS);
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
    if constexpr (PREDICT) {
      // the list proves the smallest (w, index) of ALL eligible bank rows only where w_best < floor.  The comparison is
      // STRICT, unlike the tree's: a spanning tree may take any of several equally light edges, a prediction may not --
      // two bank rows at one weight can lie in different clusters --, and a row the list does not hold may tie the
      // weight at a smaller index.
      open = !((double)w < floor_d);
    } else {
      // the list proves the lightest of all where w_best <= max(floor, core(row)): no row weighs less than core(row),
      // and of several equally light edges the tree may take any (its sorted weights do not depend on which).
      open = !((double)w <= fmax(floor_d, (double)core_row));
    }
  }
  unresolved[row] = open ? 1 : 0;
}

// row_core / n_rows: the rows the lists belong to -- the bank's own (core, n) for the tree, (core_q, n_query) for new rows
__global__ __launch_bounds__(WG) void offer_csr_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ indices,
                                                      const float* __restrict__ dist, const int64_t* __restrict__ rows,
                                                      long m, long n_rows, long n, const float* __restrict__ core,
                                                      const float* __restrict__ row_core, float* __restrict__ best_w,
                                                      int32_t* __restrict__ best_j) {
  const int lane = lane_col<64>();
  const long u = lane_row<64>();
  if (u >= m) return;
  const long row = (long)rows[u];
  if (row < 0 || row >= n_rows) return;
  const float core_row = row_core[row];
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

template <bool PREDICT>
void launch_offer_knn(const int64_t* idx, const float* dist, long rows, int k, long n, int core_col, const float* core,
                      const float* slack, int squared, float rel, float* core_q, float* best_w, int32_t* best_j,
                      uint8_t* unresolved, hipStream_t s) {
  for_lanes(lanes_for(k), [&](auto w) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL((offer_knn_kernel<W, PREDICT>), row_grid(rows, W), dim3(WG), 0, s, idx, dist, rows, k, n, core_col,
                       core, slack, squared, rel, core_q, best_w, best_j, unresolved);
  });
}

void launch_offer_csr(const int64_t* indptr, const int64_t* indices, const float* dist, const int64_t* rows, long m,
                      long n_rows, long n, const float* core, const float* row_core, float* best_w, int32_t* best_j,
                      hipStream_t s) {
  hipLaunchKernelGGL(offer_csr_kernel, row_grid(m, 64), dim3(WG), 0, s, indptr, indices, dist, rows, m, n_rows, n, core,
                     row_core, best_w, best_j);
}

}  // namespace

extern "C" int btsbot_mst_offer_knn(const int64_t* idx, const float* dist, int64_t n, int k, const float* core,
                                    const float* slack, int slack_is_squared, float rel, float* best_w, int32_t* best_j,
                                    uint8_t* unresolved, void* stream) {
  TRY(check_count("btsbot_mst_offer_knn", "n", n));
  if (k < 1 || k > OFFER_MAX_K || !(rel >= 0.0f && rel < 1.0f)) {
    btsbot_set_error("btsbot_mst_offer_knn: k=%d must be in 1..%d and rel=%g in [0, 1)", k, OFFER_MAX_K, (double)rel);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n == 0) return BTSBOT_OK;
  if (idx == nullptr || dist == nullptr || core == nullptr || best_w == nullptr || best_j == nullptr ||
      unresolved == nullptr) {
    btsbot_set_error("btsbot_mst_offer_knn: NULL argument (only slack may be NULL)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  launch_offer_knn<false>(idx, dist, (long)n, k, (long)n, -1, core, slack, slack_is_squared, rel, nullptr, best_w, best_j,
                          unresolved, (hipStream_t)stream);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_mst_offer_csr(const int64_t* indptr, const int64_t* indices, const float* dist, const int64_t* rows,
                                    int64_t m, int64_t n, const float* core, float* best_w, int32_t* best_j,
                                    void* stream) {
  TRY(check_count("btsbot_mst_offer_csr", "n", n));
  TRY(check_count("btsbot_mst_offer_csr", "m", m));
  if (m == 0 || n == 0) return BTSBOT_OK;
  if (indptr == nullptr || rows == nullptr || core == nullptr || best_w == nullptr || best_j == nullptr) {
    btsbot_set_error("btsbot_mst_offer_csr: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  launch_offer_csr(indptr, indices, dist, rows, (long)m, (long)n, (long)n, core, core, best_w, best_j, (hipStream_t)stream);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_cluster_offer_knn(const int64_t* idx, const float* dist, int64_t n_query, int k, int64_t n,
                                        int min_samples, const float* core, const float* slack, int slack_is_squared,
                                        float rel, float* core_q, float* best_w, int32_t* best_j, uint8_t* unresolved,
                                        void* stream) {
  const char* who = "btsbot_cluster_offer_knn";
  TRY(check_count(who, "n_query", n_query));
  TRY(check_count(who, "n", n));
  if (k < 1 || k > OFFER_MAX_K || min_samples < 1 || min_samples - 1 > k || !(rel >= 0.0f && rel < 1.0f)) {
    btsbot_set_error("%s: k=%d must be in 1..%d, min_samples=%d in 1..k + 1 and rel=%g in [0, 1)", who, k, OFFER_MAX_K,
                     min_samples, (double)rel);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query == 0) return BTSBOT_OK;
  if (idx == nullptr || dist == nullptr || (n > 0 && core == nullptr) || core_q == nullptr || best_w == nullptr ||
      best_j == nullptr || unresolved == nullptr) {
    btsbot_set_error("%s: NULL argument (only slack may be NULL)", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  // (core_col = -1: min_samples = 1, a core distance of 0)
  launch_offer_knn<true>(idx, dist, (long)n_query, k, (long)n, min_samples - 2, core, slack, slack_is_squared, rel, core_q,
                         best_w, best_j, unresolved, (hipStream_t)stream);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_cluster_offer_csr(const int64_t* indptr, const int64_t* indices, const float* dist,
                                        const int64_t* rows, int64_t m, int64_t n_query, int64_t n, const float* core,
                                        const float* core_q, float* best_w, int32_t* best_j, void* stream) {
  const char* who = "btsbot_cluster_offer_csr";
  TRY(check_count(who, "m", m));
  TRY(check_count(who, "n_query", n_query));
  TRY(check_count(who, "n", n));
  if (m == 0 || n_query == 0 || n == 0) return BTSBOT_OK;
  if (indptr == nullptr || rows == nullptr || core == nullptr || core_q == nullptr || best_w == nullptr ||
      best_j == nullptr) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  launch_offer_csr(indptr, indices, dist, rows, (long)m, (long)n_query, (long)n, core, core_q, best_w, best_j,
                   (hipStream_t)stream);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
