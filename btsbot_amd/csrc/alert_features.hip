// btsbot_alert_features: the per-object light-curve columns of prep_alerts (alert_utils.py:333-441 of the reference)
// for a whole batch of alerts in one launch -- peakmag, maxmag, peakmag_so_far, maxmag_so_far, age, days_since_peak,
// days_to_peak, nnotdet, as float32 [N][8] in input order.
//
// The caller has grouped the alerts by object (perm: alert indices, input order inside an object; seg_offsets: where
// each object's run starts).  With
//   O(i) = the alerts of i's object,   P(i) = { j in O(i) : (jd[j], j) <= (jd[i], i) }     (equal jd: input order)
// every output is a selection or one float64 subtraction, rounded to float32 once at the store:
//   0 min magpsf over O(i)    2 min magpsf over P(i)    4 jd[i] - first(i)      first(i) = min(jdstarthist[i], min jd over O(i))
//   1 max magpsf over O(i)    3 max magpsf over P(i)    5 jd[i] - jdpk(i)       jdpk(i)  = jd of the (jd, j)-earliest alert of
//   7 ncovhist[i] - ndethist[i]                         6 jdpk(i) - first(i)               P(i) whose magpsf is column 2
// NaN magnitudes are skipped (pandas); a set without any leaves NaN in columns 0-3, 5, 6.  A NaN jdstarthist makes
// first(i) NaN (np.min), so the minimum below is a compare-and-select, never fmin.
//
// Every alert reduces over the alerts of its own object -- n^2 compare-and-selects per object, no sort, no atomics, one
// writer per output element.  A workgroup of four waves owns four consecutive objects and picks a form per object:
//   n <= 64         one wave, one alert per lane; the object's (jd, magpsf, index) go round as readlane broadcasts
//   n <= TILE       the workgroup stages the object in LDS once; each thread reduces its alerts over the tile (every lane
//                   reads the same LDS address: a broadcast, no bank conflicts)
//   n >  TILE       the same inner loop, 256 alerts at a time, the object streamed through the LDS tile once per batch
#include "common.h"

namespace {

constexpr int TILE = 1024;   // alerts per LDS tile (alert_utils.FEATURE_TILE): 20 KB of LDS, 8 workgroups per CU
constexpr int WG = 256, OBJ_PER_WG = WG / 64;

struct Inputs {
  const int32_t* perm;
  const double* jd;
  const double* mag;
  const double* jsh;
  const int32_t* ncov;
  const int32_t* ndet;
  float* out;
  int n_alerts;
};

// what one alert knows about its object so far
struct Acc {
  double lo, hi;     // min / max magpsf over O(i)
  double sp, spjd;   // min magpsf over P(i) and the jd it was first (by (jd, j)) reached at
  double sm;         // max magpsf over P(i)
  double minjd;      // min jd over O(i)
  int spa;           // alert index of that epoch
  __device__ void init() {
    lo = hi = sp = sm = spjd = __builtin_nan("");
    minjd = __builtin_inf();
    spa = 0;
  }
  // alert (kjd, kmag, ka) of the same object seen from alert (myjd, mya)
  __device__ __forceinline__ void take(double kjd, double kmag, int ka, double myjd, int mya) {
    minjd = kjd < minjd ? kjd : minjd;
    if (kmag == kmag) {
      lo = !(lo <= kmag) ? kmag : lo;   // (a NaN running value is replaced)
      hi = !(hi >= kmag) ? kmag : hi;
      if (kjd < myjd || (kjd == myjd && ka <= mya)) {
        sm = !(sm >= kmag) ? kmag : sm;
        if (!(sp <= kmag) || (kmag == sp && (kjd < spjd || (kjd == spjd && ka < spa)))) {
          sp = kmag;
          spjd = kjd;
          spa = ka;
        }
      }
    }
  }
};

__device__ __forceinline__ void store_row(const Inputs& in, int a, double myjd, const Acc& c) {
  const double jsh = in.jsh[a];
  const double first = jsh != jsh ? jsh : (jsh < c.minjd ? jsh : c.minjd);
  const double jdpk = c.sp == c.sp ? c.spjd : __builtin_nan("");
  float4* o = reinterpret_cast<float4*>(in.out + (long)a * 8);
  o[0] = make_float4((float)c.lo, (float)c.hi, (float)c.sp, (float)c.sm);
  o[1] = make_float4((float)(myjd - first), (float)(myjd - jdpk), (float)(jdpk - first),
                     (float)((double)in.ncov[a] - (double)in.ndet[a]));
}

// alert p of the grouped order: its index (-1: p is outside the object, or perm holds no valid alert there), jd, magpsf.
// An invalid slot reads as (jd = +inf, magpsf = NaN): it changes no reduction and nothing is stored for it.
__device__ __forceinline__ int load_alert(const Inputs& in, int p, bool inside, double& jd, double& mag) {
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

__device__ __forceinline__ double lane_bcast(double v, int k) {   // k wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(WG) void alert_features_kernel(Inputs in, const int32_t* __restrict__ seg_offsets,
                                                            int n_objects) {
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
      if (mya >= 0) store_row(in, mya, myjd, c);
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
          if (mya[r] >= 0) store_row(in, mya[r], myjd[r], c[r]);
      } else if (mya[0] >= 0) {
        store_row(in, mya[0], myjd[0], c[0]);
      }
    }
  }
}

}  // namespace

extern "C" int btsbot_alert_features(const int32_t* perm, const int32_t* seg_offsets, int n_alerts, int n_objects,
                                     const double* jd, const double* magpsf, const double* jdstarthist,
                                     const int32_t* ncovhist, const int32_t* ndethist, float* out8, void* stream) {
  if (perm == nullptr || seg_offsets == nullptr || jd == nullptr || magpsf == nullptr || jdstarthist == nullptr ||
      ncovhist == nullptr || ndethist == nullptr || out8 == nullptr || n_alerts < 0 || n_objects < 0) {
    btsbot_set_error("alert_features: NULL argument or negative n_alerts / n_objects");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_alerts == 0) return BTSBOT_OK;
  if (((uintptr_t)out8 & 15) != 0) {
    btsbot_set_error("alert_features: out8 must be 16-byte aligned");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_objects == 0) {
    btsbot_set_error("alert_features: %d alerts in 0 objects", n_alerts);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const Inputs in{perm, jd, magpsf, jdstarthist, ncovhist, ndethist, out8, n_alerts};
  const unsigned blocks = (unsigned)(((long)n_objects + OBJ_PER_WG - 1) / OBJ_PER_WG);
  hipLaunchKernelGGL(alert_features_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, in, seg_offsets,
                     n_objects);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
