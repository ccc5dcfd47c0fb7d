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
// Every alert counts over the alerts of its own object -- n^2 compare-and-selects per object, the valid bits of up to
// 16 policies riding along as one mask per alert; no sort, no atomics, one writer per output element.  The earliest
// firing alert is a (jd, index) min-reduction: per thread over its own alerts, across lanes with shuffles, across the
// four waves through LDS.  A workgroup of four waves owns four consecutive objects and picks a form per object:
//   n <= 64         one wave, one alert per lane; the object's (jd, magpsf, index, mask) go round as readlane broadcasts
//   n <= TILE       the workgroup stages the object in LDS once; each thread counts its alerts over the tile (every lane
//                   reads the same LDS address: a broadcast, no bank conflicts)
//   n >  TILE       the same inner loop, 256 alerts at a time, the object streamed through the LDS tile once per batch
// The three forms run the same take() on the same (jd, index) order, so they give identical results.
//
// LDS per workgroup: 1024 x (8 + 8 + 4 + 4) B tile + 4 x 16 x (8 + 4) B of wave minima = 25,344 B, so six workgroups
// (24 waves) fit the 160 KiB of a CU.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int TILE = 1024;   // alerts per LDS tile (val.POLICY_TILE)
constexpr int WG = 256, OBJ_PER_WG = WG / 64;
constexpr int MAXP = 16;     // policies per launch

struct Policies {
  double thr[MAXP], cut[MAXP], gate[MAXP];
  int k[MAXP];
  int n;
};

struct Inputs {
  const int32_t* perm;
  const double* jd;
  const double* mag;
  const float* raw;
  const int32_t* label;
  int32_t* pred;
  double* trig;
  double* info;
  int n_alerts;
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

// the (jd, index)-earliest alert seen firing so far, per policy; a == INT_MAX: none
template <int NP>
struct Best {
  double jd[NP];
  int a[NP];
  __device__ void init() {
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      jd[q] = __builtin_inf();
      a[q] = INT_MAX;
    }
  }
  __device__ __forceinline__ void offer(int q, double ojd, int oa) {
    if (oa != INT_MAX && (a[q] == INT_MAX || ojd < jd[q] || (ojd == jd[q] && oa < a[q]))) {
      jd[q] = ojd;
      a[q] = oa;
    }
  }
  // an own alert whose counts are complete
  __device__ __forceinline__ void alert_done(const Policies& pol, const Acc<NP>& c, double myjd, int mya) {
    if (mya < 0) return;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      const double g = pol.gate[q];
      if (q < pol.n && c.cnt[q] >= pol.k[q] && (g != g || c.sp <= g)) offer(q, myjd, mya);
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
};

__device__ __forceinline__ void store_policy(const Inputs& in, const Policies& pol, long obj, int q, double bjd, int ba) {
  const bool fired = ba != INT_MAX;
  const long e = obj * pol.n + q;
  in.pred[e] = fired ? 1 : 0;
  in.trig[2 * e] = fired ? bjd : -1.0;
  in.trig[2 * e + 1] = fired ? in.mag[ba] : -1.0;
}

// n alerts starting at grouped position s: (n, label of the first alert in input order, min magpsf)
__device__ __forceinline__ void store_info(const Inputs& in, long obj, int s, int n, double lo) {
  double lab = -1.0;
  if (n > 0) {
    const int a = in.perm[s];   // the stable grouping keeps input order: the run's head is the first alert
    if ((unsigned)a < (unsigned)in.n_alerts) lab = (double)in.label[a];
  }
  in.info[3 * obj] = (double)n;
  in.info[3 * obj + 1] = lab;
  in.info[3 * obj + 2] = lo;
}

// alert p of the grouped order: its index (-1: p is outside the object, or perm holds no valid alert there), jd, magpsf
// and the mask of the policies it is valid for.  An invalid slot reads as (jd = +inf, magpsf = NaN, mask = 0): it changes
// no count and never fires.
template <int NP>
__device__ __forceinline__ int load_alert(const Inputs& in, const Policies& pol, int p, bool inside, double& jd,
                                          double& mag, unsigned& mask) {
  int a = -1;
  jd = __builtin_inf();
  mag = __builtin_nan("");
  mask = 0;
  if (inside) {
    a = in.perm[p];
    if ((unsigned)a < (unsigned)in.n_alerts) {
      jd = in.jd[a];
      mag = in.mag[a];
      const double score = (double)in.raw[a];
#pragma unroll
      for (int q = 0; q < NP; ++q)
        mask |= (unsigned)(q < pol.n && score > pol.thr[q] && mag < pol.cut[q]) << q;
    } else {
      a = -1;
    }
  }
  return a;
}

template <int NP>
__global__ __launch_bounds__(WG) void policy_eval_kernel(Inputs in, Policies pol, const int32_t* __restrict__ seg_offsets,
                                                         int n_objects) {
  __shared__ double s_jd[TILE], s_mag[TILE];
  __shared__ int s_a[TILE];
  __shared__ unsigned s_mask[TILE];
  __shared__ double s_bjd[OBJ_PER_WG][MAXP];
  __shared__ int s_ba[OBJ_PER_WG][MAXP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long obj0 = (long)blockIdx.x * OBJ_PER_WG;

  // the five offsets of this workgroup's objects (objects past n_objects: empty), clamped to the batch
  int off[OBJ_PER_WG + 1];
#pragma unroll
  for (int q = 0; q <= OBJ_PER_WG; ++q) {
    const long o = obj0 + q < n_objects ? obj0 + q : n_objects;
    const int v = seg_offsets[o];
    off[q] = v < 0 ? 0 : v > in.n_alerts ? in.n_alerts : v;
  }

  // ---- one wave per object, n <= 64 (n == 0: an empty object still gets its "never" row)
  {
    int s = off[0], e = off[1];
#pragma unroll
    for (int q = 1; q < OBJ_PER_WG; ++q)
      if (wave == q) { s = off[q]; e = off[q + 1]; }
    const int n = e - s;
    if (obj0 + wave < n_objects && n >= 0 && n <= 64) {
      double myjd, mymag;
      unsigned mymask;
      const int mya = load_alert<NP>(in, pol, s + lane, lane < n, myjd, mymag, mymask);
      Acc<NP> c;
      c.init();
      double lo = __builtin_nan("");
      for (int k = 0; k < n; ++k) {
        const double kmag = lane_bcast(mymag, k);
        lo = (kmag == kmag && !(lo <= kmag)) ? kmag : lo;
        c.take(lane_bcast(myjd, k), kmag, __builtin_amdgcn_readlane(mya, k),
               (unsigned)__builtin_amdgcn_readlane((int)mymask, k), myjd, mya);
      }
      Best<NP> b;
      b.init();
      b.alert_done(pol, c, myjd, mya);
      b.wave_min();
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NP; ++q)
          if (q < pol.n) store_policy(in, pol, obj0 + wave, q, b.jd[q], b.a[q]);
        store_info(in, obj0 + wave, s, n, lo);
      }
    }
  }

  // ---- one workgroup per object, n > 64 (every condition below is uniform over the workgroup)
  for (int q = 0; q < OBJ_PER_WG; ++q) {
    const int s = off[q], n = off[q + 1] - s;
    if (n <= 64) continue;
    Best<NP> b;
    b.init();
    double lo = __builtin_nan("");                                  // complete after any one pass over the object
    for (int b0 = 0; b0 < n; b0 += (n <= TILE ? n : WG)) {          // n <= TILE: one pass, the tile staged once
      const int bn = n <= TILE ? n : (n - b0 < WG ? n - b0 : WG);   // this pass's own alerts: [b0, b0 + bn)
      constexpr int OWN = TILE / WG;                                // own alerts per thread in the one-pass form
      double myjd[OWN];
      int mya[OWN];
      Acc<NP> c[OWN];
#pragma unroll
      for (int r = 0; r < OWN; ++r) c[r].init();
      for (int t0 = 0; t0 < n; t0 += TILE) {
        const int tn = n - t0 < TILE ? n - t0 : TILE;
        __syncthreads();                                            // the tile's previous readers are done
        for (int i = threadIdx.x; i < tn; i += WG) {
          double jd, mag;
          unsigned mask;
          s_a[i] = load_alert<NP>(in, pol, s + t0 + i, true, jd, mag, mask);
          s_jd[i] = jd;
          s_mag[i] = mag;
          s_mask[i] = mask;
        }
        __syncthreads();
        if (n <= TILE) {
          // own alerts threadIdx.x + r * WG: they are in the tile already
#pragma unroll
          for (int r = 0; r < OWN; ++r) {
            const int i = threadIdx.x + r * WG;
            mya[r] = i < n ? s_a[i] : -1;
            myjd[r] = i < n ? s_jd[i] : __builtin_inf();
          }
          for (int k = 0; k < tn; ++k) {
            const double kjd = s_jd[k], kmag = s_mag[k];
            const int ka = s_a[k];
            const unsigned km = s_mask[k];
            lo = (kmag == kmag && !(lo <= kmag)) ? kmag : lo;
#pragma unroll
            for (int r = 0; r < OWN; ++r) c[r].take(kjd, kmag, ka, km, myjd[r], mya[r]);
          }
        } else {
          if (t0 == 0) {
            double mag;
            unsigned mask;
            mya[0] = load_alert<NP>(in, pol, s + b0 + threadIdx.x, (int)threadIdx.x < bn, myjd[0], mag, mask);
          }
          for (int k = 0; k < tn; ++k) {
            const double kmag = s_mag[k];
            if (b0 == 0) lo = (kmag == kmag && !(lo <= kmag)) ? kmag : lo;
            c[0].take(s_jd[k], kmag, s_a[k], s_mask[k], myjd[0], mya[0]);
          }
        }
      }
      if (n <= TILE) {
#pragma unroll
        for (int r = 0; r < OWN; ++r) b.alert_done(pol, c[r], myjd[r], mya[r]);
      } else {
        b.alert_done(pol, c[0], myjd[0], mya[0]);
      }
    }
    // the object's earliest firing alert: lanes, then the four waves through LDS, policy p written by thread p
    b.wave_min();
    if (lane == 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        s_bjd[wave][p] = b.jd[p];
        s_ba[wave][p] = b.a[p];
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < pol.n) {
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
      store_policy(in, pol, obj0 + q, p, bjd, ba);
    }
    if (threadIdx.x == 0) store_info(in, obj0 + q, s, n, lo);
    // (the next object's first barrier comes before anything writes s_bjd / s_ba again)
  }
}

}  // namespace

extern "C" int btsbot_policy_eval(const int32_t* perm, const int32_t* seg_offsets, int n_alerts, int n_objects,
                                  const double* jd, const double* magpsf, const float* raw_pred, const int32_t* label,
                                  const double* policies, int n_policies, int32_t* obj_pred, double* obj_trigger,
                                  double* obj_info, void* stream) {
  if (perm == nullptr || seg_offsets == nullptr || jd == nullptr || magpsf == nullptr || raw_pred == nullptr ||
      label == nullptr || policies == nullptr || obj_pred == nullptr || obj_trigger == nullptr || obj_info == nullptr ||
      n_alerts < 0 || n_objects < 0) {
    btsbot_set_error("policy_eval: NULL argument or negative n_alerts / n_objects");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_policies < 1 || n_policies > MAXP) {
    btsbot_set_error("policy_eval: n_policies must be 1..%d per launch, got %d", MAXP, n_policies);
    return BTSBOT_ERR_INVALID_ARG;
  }
  Policies pol;
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
  if (n_alerts == 0) return BTSBOT_OK;
  if (n_objects == 0) {
    btsbot_set_error("policy_eval: %d alerts in 0 objects", n_alerts);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const Inputs in{perm, jd, magpsf, raw_pred, label, obj_pred, obj_trigger, obj_info, n_alerts};
  const unsigned blocks = (unsigned)(((long)n_objects + OBJ_PER_WG - 1) / OBJ_PER_WG);
  if (n_policies <= 4)
    hipLaunchKernelGGL(policy_eval_kernel<4>, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, in, pol, seg_offsets,
                       n_objects);
  else
    hipLaunchKernelGGL(policy_eval_kernel<MAXP>, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, in, pol, seg_offsets,
                       n_objects);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
