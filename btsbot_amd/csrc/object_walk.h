// The per-object walk of btsbot_alert_features and btsbot_split_labels: every alert reduces over the alerts of its own
// object -- n^2 compare-and-selects per object, no sort, no atomics, one writer per output element.
//
// The caller has grouped the alerts by object (perm: alert indices, input order inside an object; seg_offsets: where
// each object's run starts).  A workgroup of four waves owns four consecutive objects and picks a form per object:
//   n <= 64         one wave, one alert per lane; the object's (jd, magpsf, index) go round as readlane broadcasts
//   n <= TILE       the workgroup stages the object in LDS once; each thread reduces its alerts over the tile (every lane
//                   reads the same LDS address: a broadcast, no bank conflicts)
//   n >  TILE       the same inner loop, 256 alerts at a time, the object streamed through the LDS tile once per batch
//
// A kernel supplies its inputs In { const int32_t* perm; const double* jd; const double* mag; int n_alerts; ... } and an
// accumulator Acc: what one alert knows about its object so far, with
//   init()                               the empty object
//   take(kjd, kmag, ka, myjd, mya)       alert (kjd, kmag, ka) of the same object seen from alert (myjd, mya); called in
//                                        grouped order, once per slot of the object, invalid slots (ka = -1) included
//   store(in, mya, myjd)                 write alert mya's row (only called with mya >= 0)
#pragma once
#include "common.h"

namespace object_walk {

constexpr int TILE = 1024;   // alerts per LDS tile (alert_utils.FEATURE_TILE): 20 KB of LDS, 8 workgroups per CU
constexpr int WG = 256, OBJ_PER_WG = WG / 64;

// alert p of the grouped order: its index (-1: p is outside the object, or perm holds no valid alert there), jd, magpsf.
// An invalid slot reads as (jd = +inf, magpsf = NaN).
template <class In>
__device__ __forceinline__ int load_alert(const In& in, int p, bool inside, double& jd, double& mag) {
  int a = -1;
  jd = __builtin_inf();
  mag = __builtin_nan("");
  if (inside) {
    a = in.perm[p];
    if ((unsigned)a < (unsigned)in.n_alerts) {
      jd = in.jd[a];
      mag = in.mag[a];
    } else {
      a = -1;
    }
  }
  return a;
}

// the body of a kernel launched with WG threads and ceil(n_objects / OBJ_PER_WG) workgroups
template <class Acc, class In>
__device__ __forceinline__ void walk(const In& in, const int32_t* __restrict__ seg_offsets, int n_objects) {
  __shared__ double s_jd[TILE], s_mag[TILE];
  __shared__ int s_a[TILE];
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

  // ---- one wave per object, n <= 64
  {
    int s = off[0], e = off[1];
#pragma unroll
    for (int q = 1; q < OBJ_PER_WG; ++q)
      if (wave == q) { s = off[q]; e = off[q + 1]; }
    const int n = e - s;
    if (n > 0 && n <= 64) {
      double myjd, mymag;
      const int mya = load_alert(in, s + lane, lane < n, myjd, mymag);
      Acc c;
      c.init();
      for (int k = 0; k < n; ++k)
        c.take(lane_bcast(myjd, k), lane_bcast(mymag, k), __builtin_amdgcn_readlane(mya, k), myjd, mya);
      if (mya >= 0) c.store(in, mya, myjd);
    }
  }

  // ---- one workgroup per object, n > 64 (every condition below is uniform over the workgroup)
  for (int q = 0; q < OBJ_PER_WG; ++q) {
    const int s = off[q], n = off[q + 1] - s;
    if (n <= 64) continue;
    for (int b0 = 0; b0 < n; b0 += (n <= TILE ? n : WG)) {        // n <= TILE: one pass, the tile staged once
      const int bn = n <= TILE ? n : (n - b0 < WG ? n - b0 : WG);   // this pass's own alerts: [b0, b0 + bn)
      constexpr int OWN = TILE / WG;                                // own alerts per thread in the one-pass form
      double myjd[OWN];
      int mya[OWN];
      Acc c[OWN];
#pragma unroll
      for (int r = 0; r < OWN; ++r) c[r].init();
      for (int t0 = 0; t0 < n; t0 += TILE) {
        const int tn = n - t0 < TILE ? n - t0 : TILE;
        __syncthreads();                                            // the tile's previous readers are done
        for (int i = threadIdx.x; i < tn; i += WG) {
          double jd, mag;
          s_a[i] = load_alert(in, s + t0 + i, true, jd, mag);
          s_jd[i] = jd;
          s_mag[i] = mag;
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
#pragma unroll
            for (int r = 0; r < OWN; ++r) c[r].take(kjd, kmag, ka, myjd[r], mya[r]);
          }
        } else {
          if (t0 == 0) {
            double mag;
            mya[0] = load_alert(in, s + b0 + threadIdx.x, (int)threadIdx.x < bn, myjd[0], mag);
          }
          for (int k = 0; k < tn; ++k) c[0].take(s_jd[k], s_mag[k], s_a[k], myjd[0], mya[0]);
        }
      }
      if (n <= TILE) {
#pragma unroll
        for (int r = 0; r < OWN; ++r)
          if (mya[r] >= 0) c[r].store(in, mya[r], myjd[r]);
      } else if (mya[0] >= 0) {
        c[0].store(in, mya[0], myjd[0]);
      }
    }
  }
}

}  // namespace object_walk
