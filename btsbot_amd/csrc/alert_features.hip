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
// Every alert reduces over the alerts of its own object, in the three forms of object_walk.h (one wave; the object
// resident in LDS; the object streamed through the LDS tile).
#include "object_walk.h"

namespace {

using object_walk::WG;

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
  // alert (kjd, kmag, ka) of the same object seen from alert (myjd, mya); an invalid slot (jd = +inf, magpsf = NaN)
  // changes no reduction
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
  __device__ __forceinline__ void store(const Inputs& in, int a, double myjd) const {
    const double jsh = in.jsh[a];
    const double first = jsh != jsh ? jsh : (jsh < minjd ? jsh : minjd);
    const double jdpk = sp == sp ? spjd : __builtin_nan("");
    float4* o = reinterpret_cast<float4*>(in.out + (long)a * 8);
    o[0] = make_float4((float)lo, (float)hi, (float)sp, (float)sm);
    o[1] = make_float4((float)(myjd - first), (float)(myjd - jdpk), (float)(jdpk - first),
                       (float)((double)in.ncov[a] - (double)in.ndet[a]));
  }
};

__global__ __launch_bounds__(WG) void alert_features_kernel(Inputs in, const int32_t* __restrict__ seg_offsets,
                                                            int n_objects) {
  object_walk::walk<Acc>(in, seg_offsets, n_objects);
}

}  // namespace

extern "C" int btsbot_alert_features(const int32_t* perm, const int32_t* seg_offsets, int n_alerts, int n_objects,
                                     const double* jd, const double* magpsf, const double* jdstarthist,
                                     const int32_t* ncovhist, const int32_t* ndethist, float* out8, void* stream) {
  TRY(object_walk::check_args("alert_features",
                              perm != nullptr && seg_offsets != nullptr && jd != nullptr && magpsf != nullptr &&
                                  jdstarthist != nullptr && ncovhist != nullptr && ndethist != nullptr && out8 != nullptr,
                              n_alerts, n_objects));
  if (n_alerts > 0 && ((uintptr_t)out8 & 15) != 0) {   // (an empty batch returns BTSBOT_OK whatever out8 is)
    btsbot_set_error("alert_features: out8 must be 16-byte aligned");
    return BTSBOT_ERR_INVALID_ARG;
  }
  unsigned blocks;
  TRY(object_walk::grid("alert_features", n_alerts, n_objects, &blocks));
  if (blocks == 0) return BTSBOT_OK;
  const Inputs in{perm, jd, magpsf, jdstarthist, ncovhist, ndethist, out8, n_alerts};
  hipLaunchKernelGGL(alert_features_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, in, seg_offsets,
                     n_objects);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
