// btsbot_policy_eval: the per-object half of the reference's policy metrics (val.py:454-500 inside diagnostic_fig) for a
// whole validation split in one launch -- does a scanning policy fire on an object, and at which alert first.
//
// The caller has grouped the alerts by object (perm: alert indices, input order inside an object; seg_offsets: where
// each object's run starts).  A policy is (thr, cut, k, gate).  With
//   O(i) = the alerts of i's object,   P(i) = { j in O(i) : (jd[j], j) <= (jd[i], i) }     (equal jd: input order)
//   valid(j) = (double)raw_pred[j] > thr  and  magpsf[j] < cut                             (NaN magpsf: never valid)
// the policy fires at alert i when  #{ j in P(i) : valid(j) } >= k  and (no gate, or min magpsf over P(i) <= gate; NaN
// skipped).  Both conditions are monotone along the light curve, so the object's pred is "fires anywhere" and its
// trigger is the (jd, index)-earliest alert it fires at: (jd, magpsf) of that alert, (-1, -1) when there is none.
// obj_info keeps what the object filter and the peak-magnitude bins need: the number of alerts, the label of the
// first alert in input order, min magpsf over O (NaN: no magnitude at all).
//
// Every alert counts over the alerts of its own object in the three forms of object_walk.h (one wave; the object
// resident in LDS; the object streamed through the LDS tile), the valid bits of up to 16 policies riding along as the
// walk's payload word: one mask per alert.  The result is per object, so the walk runs with a reducer: the earliest
// firing alert is a (jd, index) min-reduction -- per thread over its own alerts, across lanes with shuffles, across the
// four waves through LDS -- beside a running min magpsf over the object.
//
// LDS per workgroup: 1024 x (8 + 8 + 4 + 4) B tile + 4 x 16 x (8 + 4) B of wave minima = 25,344 B, so six workgroups
// (24 waves) fit the 160 KiB of a CU.
#include "object_walk.h"

#include <climits>
#include <cmath>

namespace {

using object_walk::OBJ_PER_WG;
using object_walk::WG;
constexpr int MAXP = 16;     // policies per launch

struct Policies {
  double thr[MAXP], cut[MAXP], gate[MAXP];
  int k[MAXP];
  int n;
};

struct Args {
  const int32_t* perm;
  const double* jd;
  const double* mag;
  const float* raw;
  const int32_t* label;
  int32_t* pred;
  double* trig;
  double* info;
  int n_alerts;
  Policies pol;
};

// the walk's inputs for a kernel of up to NP policies: every alert carries the mask of the policies it is valid for (an
// invalid slot: 0, it changes no count and never fires)
template <int NP>
struct Inputs : Args {
  using Word = unsigned;
  __device__ __forceinline__ Word word(int a, double amag) const {
    const double score = (double)raw[a];
    Word mask = 0;
#pragma unroll
    for (int q = 0; q < NP; ++q) mask |= (unsigned)(q < pol.n && score > pol.thr[q] && amag < pol.cut[q]) << q;
    return mask;
  }
};

// what one alert knows about the alerts of its object up to and including itself
template <int NP>
struct Acc {
  double sp;     // min magpsf over P(i)
  int cnt[NP];   // valid alerts in P(i), per policy
  __device__ void init() {
    sp = __builtin_nan("");
#pragma unroll
    for (int q = 0; q < NP; ++q) cnt[q] = 0;
  }
  // alert (kjd, kmag, ka, kmask) of the same object seen from alert (myjd, mya)
  __device__ __forceinline__ void take(double kjd, double kmag, int ka, unsigned kmask, double myjd, int mya) {
    if (kjd < myjd || (kjd == myjd && ka <= mya)) {
      sp = (kmag == kmag && !(sp <= kmag)) ? kmag : sp;   // (a NaN running value is replaced)
#pragma unroll
      for (int q = 0; q < NP; ++q) cnt[q] += (int)((kmask >> q) & 1u);
    }
  }
};

__device__ __forceinline__ void store_policy(const Args& in, long obj, int q, double bjd, int ba) {
  const bool fired = ba != INT_MAX;
  const long e = obj * in.pol.n + q;
  in.pred[e] = fired ? 1 : 0;
  in.trig[2 * e] = fired ? bjd : -1.0;
  in.trig[2 * e + 1] = fired ? in.mag[ba] : -1.0;
}

// n alerts starting at grouped position s: (n, label of the first alert in input order, min magpsf)
__device__ __forceinline__ void store_info(const Args& in, long obj, int s, int n, double lo) {
  double lab = -1.0;
  if (n > 0) {
    const int a = in.perm[s];   // the stable grouping keeps input order: the run's head is the first alert
    if ((unsigned)a < (unsigned)in.n_alerts) lab = (double)in.label[a];
  }
  in.info[3 * obj] = (double)n;
  in.info[3 * obj + 1] = lab;
  in.info[3 * obj + 2] = lo;
}

// the walk's reducer: the (jd, index)-earliest alert seen firing so far, per policy (a == INT_MAX: none), and min
// magpsf over the object
template <int NP>
struct Best {
  double jd[NP];
  int a[NP];
  double lo;
  __device__ void init() {
    lo = __builtin_nan("");
    // lo stays in vector registers: in the one-wave form it is uniform, and for a scalar pair hipcc 7.2 can emit the NaN
    // as one s_mov_b64 with a 64-bit literal, which gfx950 cannot encode -- the object file then holds its low half, 0
    asm volatile("" : "+v"(lo));
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      jd[q] = __builtin_inf();
      a[q] = INT_MAX;
    }
  }
  __device__ __forceinline__ void slot(double, double kmag, int) { lo = (kmag == kmag && !(lo <= kmag)) ? kmag : lo; }
  __device__ __forceinline__ void offer(int q, double ojd, int oa) {
    if (oa != INT_MAX && (a[q] == INT_MAX || ojd < jd[q] || (ojd == jd[q] && oa < a[q]))) {
      jd[q] = ojd;
      a[q] = oa;
    }
  }
  __device__ __forceinline__ void alert_done(const Inputs<NP>& in, const Acc<NP>& c, double myjd, int mya) {
    if (mya < 0) return;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const double g = in.pol.gate[q];
      if (q < in.pol.n && c.cnt[q] >= in.pol.k[q] && (g != g || c.sp <= g)) offer(q, myjd, mya);
    }
  }
  __device__ __forceinline__ void wave_min() {   // afterwards every lane holds the wave's earliest
#pragma unroll
    for (int q = 0; q < NP; ++q) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) {
        const double ojd = __shfl_xor(jd[q], d);
        const int oa = __shfl_xor(a[q], d);
        offer(q, ojd, oa);
      }
    }
  }
  __device__ __forceinline__ void finish_wave(const Inputs<NP>& in, long obj, int s, int n) {
    wave_min();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int q = 0; q < NP; ++q)
        if (q < in.pol.n) store_policy(in, obj, q, jd[q], a[q]);
      store_info(in, obj, s, n, lo);
    }
  }
  // lanes, then the four waves through LDS, policy p written by thread p.  Nothing writes s_bjd / s_ba again before the
  // next object's first barrier (object_walk.h).
  __device__ __forceinline__ void finish_workgroup(const Inputs<NP>& in, long obj, int s, int n) {
    __shared__ double s_bjd[OBJ_PER_WG][MAXP];
    __shared__ int s_ba[OBJ_PER_WG][MAXP];
    const int wave = threadIdx.x >> 6;
    wave_min();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        s_bjd[wave][p] = jd[p];
        s_ba[wave][p] = a[p];
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < in.pol.n) {
      const int p = threadIdx.x;
      double bjd = s_bjd[0][p];
      int ba = s_ba[0][p];
      for (int w = 1; w < OBJ_PER_WG; ++w) {
        const double ojd = s_bjd[w][p];
        const int oa = s_ba[w][p];
        if (oa != INT_MAX && (ba == INT_MAX || ojd < bjd || (ojd == bjd && oa < ba))) {
          bjd = ojd;
          ba = oa;
        }
      }
      store_policy(in, obj, p, bjd, ba);
    }
    if (threadIdx.x == 0) store_info(in, obj, s, n, lo);
  }
};

template <int NP>
__global__ __launch_bounds__(WG) void policy_eval_kernel(Inputs<NP> in, const int32_t* __restrict__ seg_offsets,
                                                         int n_objects) {
  object_walk::walk<Acc<NP>, Best<NP>>(in, seg_offsets, n_objects);
}

}  // namespace

extern "C" int btsbot_policy_eval(const int32_t* perm, const int32_t* seg_offsets, int n_alerts, int n_objects,
                                  const double* jd, const double* magpsf, const float* raw_pred, const int32_t* label,
                                  const double* policies, int n_policies, int32_t* obj_pred, double* obj_trigger,
                                  double* obj_info, void* stream) {
  TRY(object_walk::check_args("policy_eval",
                              perm != nullptr && seg_offsets != nullptr && jd != nullptr && magpsf != nullptr &&
                                  raw_pred != nullptr && label != nullptr && policies != nullptr && obj_pred != nullptr &&
                                  obj_trigger != nullptr && obj_info != nullptr,
                              n_alerts, n_objects));
  if (n_policies < 1 || n_policies > MAXP) {
    btsbot_set_error("policy_eval: n_policies must be 1..%d per launch, got %d", MAXP, n_policies);
    return BTSBOT_ERR_INVALID_ARG;
  }
  Args in{perm, jd, magpsf, raw_pred, label, obj_pred, obj_trigger, obj_info, n_alerts, {}};
  Policies& pol = in.pol;
  pol.n = n_policies;
  for (int q = 0; q < MAXP; ++q) {
    const bool used = q < n_policies;
    const double k = used ? policies[4 * q + 2] : 1.0;
    if (!(k >= 1.0) || k != std::floor(k)) {
      btsbot_set_error("policy_eval: policy %d: k must be an integer >= 1, got %g", q, k);
      return BTSBOT_ERR_INVALID_ARG;
    }
    pol.thr[q] = used ? policies[4 * q] : 0.0;
    pol.cut[q] = used ? policies[4 * q + 1] : 0.0;
    pol.gate[q] = used ? policies[4 * q + 3] : 0.0;
    pol.k[q] = k > (double)INT_MAX ? INT_MAX : (int)k;   // (more than any object can hold: never fires)
  }
  unsigned blocks;
  TRY(object_walk::grid("policy_eval", n_alerts, n_objects, &blocks));
  if (blocks == 0) return BTSBOT_OK;
  if (n_policies <= 4)
    hipLaunchKernelGGL(policy_eval_kernel<4>, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, Inputs<4>{in}, seg_offsets,
                       n_objects);
  else
    hipLaunchKernelGGL(policy_eval_kernel<MAXP>, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, Inputs<MAXP>{in},
                       seg_offsets, n_objects);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
