// btsbot_alert_histograms: every alert-level count of the reference's diagnostic figure (val.py:185-379 inside
// diagnostic_fig) in one pass over a split's alerts -- the score / magnitude density (ax4.hist2d) with its two marginal
// histograms, the TP / FP / TN / FN counts per magnitude bin (np.histogram per class, the stacked bars) and the four
// totals of the confusion matrix.
//
// Bin rule (numpy's, which the figure goes through): bin i of edges e[0..nb] holds e[i] <= x < e[i+1], the last bin also
// x == e[nb]; anything else, NaN included, is in no bin.  The edges come from the caller as float64 and are compared as
// they are (never recomputed as lo + i * step); a score is its float32 value widened to float64.  pred = score > 0.5
// (np.rint takes 0.5 to 0; a NaN score predicts 0 and is in no score bin), label != 0 is a positive.
//
// One workgroup of 1024 threads (16 waves) per CU at most, grid-stride over the alerts.  The three edge tables (kernel
// arguments: they are host data, validated before the launch) are copied to LDS, a bin is found by binary search over its
// table (at most seven probes for 64 bins; every lane probes its own address, float64 LDS reads).  The workgroup counts
// into int32 counters of its own in LDS -- n_mag * n_score + n_mag + n_score + 4 * n_class + 4 of them, 892 for the
// figure's shape, 4484 (17.5 KB) for the largest -- and adds the non-zero ones to `out` once, with 64-bit global atomics:
// integer sums, so the result does not depend on the order.  No workgroup waits for another.
//
// Three build-time choices, each made from a measurement on 1,000,000 alerts (DESIGN.md section 4l has the tables; the
// macros stay so that it can be repeated, tools/build_variant.sh):
//   ALERT_HIST_WG      threads per workgroup.  The loop is latency-bound (a load, a dependent search, LDS atomics), so the
//                      waves a CU holds decide: 256 threads took 0.029 ms, 512 0.019 ms, 1024 0.015 ms.
//   ALERT_HIST_GRID    most workgroups.  Every workgroup flushes up to 892 counters, so more of them cost more atomics:
//                      at 1024 threads, 256 workgroups took 0.015 ms, 512 0.018 ms, 1024 0.027 ms (at 8,000,000 alerts
//                      512 win, 0.047 against 0.062 ms; the grid does not follow n).
//   ALERT_HIST_LAYOUT  how the hot counters are kept -- a trained model's scores pile into the first and the last score
//                      bin, and every alert lands in one of the four totals:
//                        0  every count is one LDS atomic add on the workgroup's counters
//                        1  the four totals and the first / last score bin are wave sums: one ballot + popcount per wave
//                           and trip, kept in wave-uniform registers and added to LDS once per wave; the interior score
//                           bins stay LDS atomics
//                      With 4 waves per workgroup layout 1 was 3-5 % slower on every distribution.  With 16 waves adding to
//                      the same counters it is the one that does not care about the distribution: trained-like scores
//                      cost layout 0 8 % at 1,000,000 alerts (0.0160 against 0.0148 ms) and 16 % at 8,000,000, layout 1
//                      nothing (0.0148 / 0.0146 ms), and on uniform scores the two are equal.  Layout 1 is built.
#include "common.h"

#include <cmath>

#ifndef ALERT_HIST_LAYOUT
#define ALERT_HIST_LAYOUT 1
#endif
#ifndef ALERT_HIST_WG
#define ALERT_HIST_WG 1024
#endif
#ifndef ALERT_HIST_GRID
#define ALERT_HIST_GRID 256
#endif

namespace {

constexpr int WG = ALERT_HIST_WG;
constexpr int MAXB = 64;                                          // bins per table
constexpr int MAXJOINT = 4096;                                    // n_mag * n_score
constexpr int MAXCOUNT = MAXJOINT + 2 * MAXB + 4 * MAXB + 4;      // 4484 counters
constexpr int GRID_CAP = ALERT_HIST_GRID;                         // workgroups: one per CU of an MI355X
static_assert(WG > MAXB && WG % 64 == 0 && WG <= 1024, "a thread per edge, whole waves");
constexpr int64_t MAX_ALERTS = (int64_t)1 << 38;                  // a workgroup's share stays below 2^31: int32 counters

struct Edges {
  double mag[MAXB + 1], score[MAXB + 1], cls[MAXB + 1];
  int n_mag, n_score, n_class;
};

// the bin of x over e[0..nb], -1 when it has none.  Invariant of the search: e[lo] <= x < e[hi] (e[nb + 1] = +inf)
__device__ __forceinline__ int find_bin(const double* e, int nb, double x) {
  if (!(x >= e[0] && x <= e[nb])) return -1;
  int lo = 0, hi = nb + 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;                               // 1..nb
    if (e[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo < nb ? lo : nb - 1;                                   // x == e[nb]: the last bin
}

template <int LAYOUT>
__global__ __launch_bounds__(WG) void alert_hist_kernel(const double* __restrict__ mag, const float* __restrict__ raw,
                                                        const int32_t* __restrict__ label, long n, Edges ed,
                                                        unsigned long long* __restrict__ out) {
  __shared__ double s_me[MAXB + 1], s_se[MAXB + 1], s_ce[MAXB + 1];
  __shared__ int s_cnt[MAXCOUNT];
  const int tid = threadIdx.x;
  const int nm = ed.n_mag, ns = ed.n_score, nc = ed.n_class;
  const int o_mag = nm * ns, o_score = o_mag + nm, o_cls = o_score + ns, o_tot = o_cls + 4 * nc, ncount = o_tot + 4;
  for (int i = tid; i < ncount; i += WG) s_cnt[i] = 0;
  if (tid <= nm) s_me[tid] = ed.mag[tid];
  if (tid <= ns) s_se[tid] = ed.score[tid];
  if (tid <= nc) s_ce[tid] = ed.cls[tid];
  __syncthreads();

  int w_tot[4] = {0, 0, 0, 0}, w_first = 0, w_last = 0;           // LAYOUT 1: wave sums, the same in every lane
  const long stride = (long)gridDim.x * WG;
  for (long base = (long)blockIdx.x * WG; base < n; base += stride) {   // (the trip count is uniform over the workgroup)
    const long i = base + tid;
    int cls = -1, sb = -1;
    if (i < n) {
      const double m = mag[i];
      const double s = (double)raw[i];
      const bool pred = s > 0.5, pos = label[i] != 0;
      cls = pos ? (pred ? 0 : 3) : (pred ? 1 : 2);                // TP, FP, TN, FN
      const int mb = find_bin(s_me, nm, m), cb = find_bin(s_ce, nc, m);
      sb = find_bin(s_se, ns, s);
      if (mb >= 0) atomicAdd(&s_cnt[o_mag + mb], 1);
      if (mb >= 0 && sb >= 0) atomicAdd(&s_cnt[mb * ns + sb], 1);
      if (cb >= 0) atomicAdd(&s_cnt[o_cls + cls * nc + cb], 1);
      if (LAYOUT == 0) {
        if (sb >= 0) atomicAdd(&s_cnt[o_score + sb], 1);
        atomicAdd(&s_cnt[o_tot + cls], 1);
      } else if (sb > 0 && sb < ns - 1) {
        atomicAdd(&s_cnt[o_score + sb], 1);
      }
    }
    if (LAYOUT == 1) {                                            // every lane of the wave is here (cls = sb = -1: no alert)
#pragma unroll
      for (int c = 0; c < 4; ++c) w_tot[c] += __popcll(__ballot(cls == c));
      w_first += __popcll(__ballot(sb == 0));
      w_last += __popcll(__ballot(sb == ns - 1 && ns > 1));
    }
  }
  if (LAYOUT == 1 && (tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (w_tot[c]) atomicAdd(&s_cnt[o_tot + c], w_tot[c]);
    if (w_first) atomicAdd(&s_cnt[o_score], w_first);
    if (w_last) atomicAdd(&s_cnt[o_score + ns - 1], w_last);
  }
  __syncthreads();
  for (int i = tid; i < ncount; i += WG) {
    const int v = s_cnt[i];
    if (v != 0) atomicAdd(out + i, (unsigned long long)v);
  }
}

// n + 1 finite, strictly increasing edges, n in 1..MAXB
int check_edges(const char* name, const double* e, int n) {
  if (e == nullptr) {
    btsbot_set_error("alert_histograms: %s_edges is NULL", name);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n < 1 || n > MAXB) {
    btsbot_set_error("alert_histograms: n_%s must be 1..%d, got %d", name, MAXB, n);
    return BTSBOT_ERR_INVALID_ARG;
  }
  for (int i = 0; i <= n; ++i) {
    if (!std::isfinite(e[i]) || (i > 0 && !(e[i] > e[i - 1]))) {
      btsbot_set_error("alert_histograms: %s_edges must be finite and strictly increasing (edge %d = %g)", name, i, e[i]);
      return BTSBOT_ERR_INVALID_ARG;
    }
  }
  return BTSBOT_OK;
}

}  // namespace

extern "C" int btsbot_alert_histograms(const double* magpsf, const float* raw, const int32_t* label, int64_t n,
                                       const double* mag_edges, int n_mag, const double* score_edges, int n_score,
                                       const double* class_edges, int n_class, int64_t* out, void* stream) {
  int rc;
  if ((rc = check_edges("mag", mag_edges, n_mag)) != BTSBOT_OK) return rc;
  if ((rc = check_edges("score", score_edges, n_score)) != BTSBOT_OK) return rc;
  if ((rc = check_edges("class", class_edges, n_class)) != BTSBOT_OK) return rc;
  if (n_mag * n_score > MAXJOINT) {
    btsbot_set_error("alert_histograms: n_mag * n_score must be <= %d, got %d x %d", MAXJOINT, n_mag, n_score);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n < 0 || n > MAX_ALERTS) {
    btsbot_set_error("alert_histograms: n must be 0..2^38, got %lld", (long long)n);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n == 0) return BTSBOT_OK;
  if (magpsf == nullptr || raw == nullptr || label == nullptr || out == nullptr) {
    btsbot_set_error("alert_histograms: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  Edges ed = {};
  for (int i = 0; i <= n_mag; ++i) ed.mag[i] = mag_edges[i];
  for (int i = 0; i <= n_score; ++i) ed.score[i] = score_edges[i];
  for (int i = 0; i <= n_class; ++i) ed.cls[i] = class_edges[i];
  ed.n_mag = n_mag;
  ed.n_score = n_score;
  ed.n_class = n_class;
  const int64_t want = (n + WG - 1) / WG;
  const unsigned blocks = (unsigned)(want < GRID_CAP ? want : GRID_CAP);
  hipLaunchKernelGGL(alert_hist_kernel<ALERT_HIST_LAYOUT>, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, magpsf, raw,
                     label, (long)n, ed, (unsigned long long*)out);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
