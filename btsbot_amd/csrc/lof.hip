// btsbot_lof_*: the local outlier factor on a kNN graph (gfx950), DESIGN.md section 4u.
//
//   bank among itself (btsbot_knn_query, self masked) -> kdist [n] -> lrd [n] -> lof [n]      three launches
//   new rows against a fitted bank (no self)          -> lrd [q], lof [q]                      one launch
//
// An entry (row, c) is PRESENT when 0 <= idx[row][c] < n (n: the rows kdist / lrd are held for); a -1 tail is no entry and
// an index out of range is treated the same (the rule of layout_smooth_knn_kernel).  m(row) = the present entries.
// Everything is float64 on the fp32 distances converted once.
//   kdist(i)     dist of row i's last present column                                           NaN when m = 0
//   reach(i, c)  fmax(dist[i][c], kdist(idx[i][c]))          (fmax: a NaN kdist leaves dist)
//   lrd(i)       1 / (sum_c reach(i, c) / m + 1e-10)         (scikit-learn's constant)         NaN when m = 0
//   lof(i)       (sum_c lrd(idx[i][c]) / lrd(i)) / m         (each quotient formed first)      NaN when m = 0
//
// Lanes.  A row is held by a group of W lanes, lane c its column c (csrc/list_row.h): W = 16, 32 or 64, the smallest that
// holds k, so that at the usual k = 15..20 a wave carries four or two rows and not one (4u has the times of both forms).
//
// The order of a row's sum (list_row::group_sum) -- the one thing a float64 restatement has to copy (tests/lof_ref.py,
// tree_sum):
//   slots v[0..W), v[c] = the term of column c where the entry is present, +0.0 everywhere else (c >= k, absent);
//   for o = W/2, W/4, ..., 1:  v[c] <- v[c] + v[c ^ o] for every c at once;   the sum is v[0].
// It depends on the row's own columns and on k (through W) alone: not on the grid, the run, the other rows of the call or
// where the row stands in its workgroup.  (A slot of +0.0 adds exactly, so W = 64 gives the bits of the smaller W for every
// sum that is not a zero; BTSBOT_LOF_LANES=64 at compile time is the one-wave-per-row form, kept to time it.)
// Nothing here is a product followed by a sum, and the contraction is switched off all the same; the divisions are IEEE.
#include "list_row.h"

#pragma clang fp contract(off)

namespace {

using namespace list_row;

constexpr int LOF_MAX_K = 64;

// what lane c of a row's group holds: its entry, whether it is present, and m
struct Entry {
  long j;
  double d;
  bool present;
  int m;
};
template <int W>
__device__ __forceinline__ Entry load_entry(const int64_t* __restrict__ idx, const float* __restrict__ dist, long row, int k,
                                            int c, long n) {
  Entry e;
  const bool in_row = c < k;
  e.j = in_row ? (long)idx[row * k + c] : -1;
  e.present = e.j >= 0 && e.j < n;
  e.d = in_row ? (double)dist[row * k + c] : 0.0;
  e.m = group_sum_i<W>(e.present ? 1 : 0);
  return e;
}

template <int W>
__global__ __launch_bounds__(WG) void lof_kdist_kernel(const int64_t* __restrict__ idx, const float* __restrict__ dist, long n,
                                                      int k, double* __restrict__ kdist) {
  const int c = lane_col<W>();
  const long row = lane_row<W>();
  if (row >= n) return;   // (a whole group leaves together)
  const Entry e = load_entry<W>(idx, dist, row, k, c, n);
  const int last = group_max_i<W>(e.present ? c : -1);
  if (c == (last < 0 ? 0 : last)) kdist[row] = last < 0 ? __builtin_nan("") : e.d;
}

// STAGE 0: lrd of bank rows from kdist.  STAGE 1: lof of bank rows from lrd (own = the row's own lrd).
// STAGE 2: the query side, both at once from the bank's arrays.
template <int W, int STAGE>
__global__ __launch_bounds__(WG) void lof_kernel(const int64_t* __restrict__ idx, const float* __restrict__ dist, long rows,
                                                int k, const double* __restrict__ bank_kdist,
                                                const double* __restrict__ bank_lrd, long n, double* __restrict__ lrd,
                                                double* __restrict__ lof) {
  const int c = lane_col<W>();
  const long row = lane_row<W>();
  if (row >= rows) return;
  const Entry e = load_entry<W>(idx, dist, row, k, c, n);
  const double nan = __builtin_nan("");
  // both gathers leave before either sum waits
  const double kd = (STAGE != 1 && e.present) ? bank_kdist[e.j] : 0.0;
  const double lj = (STAGE != 0 && e.present) ? bank_lrd[e.j] : 0.0;
  double own;
  if (STAGE == 1) {
    own = bank_lrd[row];
  } else {
    const double sum = group_sum<W>(e.present ? fmax(e.d, kd) : 0.0);
    own = e.m > 0 ? 1.0 / (sum / (double)e.m + 1e-10) : nan;
    if (c == 0 && lrd != nullptr) lrd[row] = own;
  }
  if (STAGE != 0) {
    const double sum = group_sum<W>(e.present ? lj / own : 0.0);
    if (c == 0) lof[row] = e.m > 0 ? sum / (double)e.m : nan;
  }
}

// (BTSBOT_LOF_LANES=64 at compile time: one wave per row at every k, the form 4u times this one against)
int lof_lanes(int k) {
#ifdef BTSBOT_LOF_LANES
  static_assert(BTSBOT_LOF_LANES == 64, "only the whole wave holds every k");
  return BTSBOT_LOF_LANES;
#else
  return lanes_for(k);
#endif
}

int check_lof_shape(const char* who, int64_t rows, int k, int64_t n) {
  if (rows < 0 || rows > 0x7fffffffLL || n < 0 || n > 0x7fffffffLL || k < 1 || k > LOF_MAX_K) {
    btsbot_set_error("%s: need 0 <= rows, n < 2^31 and 1 <= k <= %d (rows=%lld n=%lld k=%d)", who, LOF_MAX_K, (long long)rows,
                     (long long)n, k);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

template <int W>
void launch_fit(const int64_t* idx, const float* dist, long n, int k, double* kdist, double* lrd, double* lof,
                hipStream_t s) {
  const dim3 grid = row_grid(n, W);
  hipLaunchKernelGGL(lof_kdist_kernel<W>, grid, dim3(WG), 0, s, idx, dist, n, k, kdist);
  hipLaunchKernelGGL((lof_kernel<W, 0>), grid, dim3(WG), 0, s, idx, dist, n, k, (const double*)kdist, (const double*)nullptr, n,
                     lrd, (double*)nullptr);
  if (lof != nullptr)
    hipLaunchKernelGGL((lof_kernel<W, 1>), grid, dim3(WG), 0, s, idx, dist, n, k, (const double*)nullptr, (const double*)lrd, n,
                       (double*)nullptr, lof);
}

template <int W>
void launch_score(const int64_t* idx, const float* dist, long q, int k, const double* bank_kdist, const double* bank_lrd,
                  long n, double* lrd, double* lof, hipStream_t s) {
  hipLaunchKernelGGL((lof_kernel<W, 2>), row_grid(q, W), dim3(WG), 0, s, idx, dist, q, k, bank_kdist, bank_lrd, n, lrd, lof);
}

}  // namespace

extern "C" int btsbot_lof_fit(const int64_t* idx, const float* dist, int64_t n, int k, double* kdist, double* lrd, double* lof,
                              void* stream) {
  TRY(check_lof_shape("btsbot_lof_fit", n, k, n));
  if (n == 0) return BTSBOT_OK;
  if (idx == nullptr || dist == nullptr || kdist == nullptr || lrd == nullptr) {
    btsbot_set_error("btsbot_lof_fit: NULL argument (only lof may be NULL)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (misaligned(idx, 8) || misaligned(dist, 4) || misaligned(kdist, 8) || misaligned(lrd, 8) || misaligned(lof, 8)) {
    btsbot_set_error("btsbot_lof_fit: misaligned argument (idx and the float64 arrays: 8 bytes, dist: 4)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  for_lanes(lof_lanes(k), [&](auto w) { launch_fit<decltype(w)::value>(idx, dist, (long)n, k, kdist, lrd, lof, s); });
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_lof_score(const int64_t* idx, const float* dist, int64_t q, int k, const double* bank_kdist,
                                const double* bank_lrd, int64_t n, double* lrd, double* lof, void* stream) {
  TRY(check_lof_shape("btsbot_lof_score", q, k, n));
  if (q == 0) return BTSBOT_OK;
  // (an empty bank has no arrays to name: no entry is present and every row scores NaN)
  if (idx == nullptr || dist == nullptr || lof == nullptr || (n > 0 && (bank_kdist == nullptr || bank_lrd == nullptr))) {
    btsbot_set_error("btsbot_lof_score: NULL argument (only lrd may be NULL)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (misaligned(idx, 8) || misaligned(dist, 4) || misaligned(bank_kdist, 8) || misaligned(bank_lrd, 8) ||
      misaligned(lrd, 8) || misaligned(lof, 8)) {
    btsbot_set_error("btsbot_lof_score: misaligned argument (idx and the float64 arrays: 8 bytes, dist: 4)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  for_lanes(lof_lanes(k), [&](auto w) {
    launch_score<decltype(w)::value>(idx, dist, (long)q, k, bank_kdist, bank_lrd, (long)n, lrd, lof, s);
  });
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
