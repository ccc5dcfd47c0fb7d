// btsbot_split_labels: what the per-object loops of cut_set_and_assign_splits and create_subset
// (query_data/train_val_test_split.py:123-140, 211-231 of the reference) need to know about each alert's object, for a
// whole table in one launch.  Those loops scan the table once per object; here every alert reduces over the alerts of
// its own object in the three forms of object_walk.h.
//
// With O(i) the alerts of i's object (grouped by the caller: perm, seg_offsets), per alert, in input order:
//   pos        |{ j in O(i) : j < i }|         the alert's position in the object in table order: with size it picks the
//   size       |O(i)|                          alert's N label out of RandomState(seed).permutation(size)
//   first_row  min O(i)                        the row of the object's first appearance: its rank orders the split draw
//   later      |{ j in O(i) : (jd[j], j) > (jd[i], i) }|      "one of the k latest alerts" is later < k
//   is_rise    jd[i] <= jd[m],  m = the lowest row of O(i) at the minimum non-NaN magpsf of O(i) (np.argmin: ties of
//              the minimum go to the lowest row, not the lowest jd)
//   peakmag    magpsf[m]; NaN when every magpsf of the object is NaN, and is_rise is then 0 on all of it
// later orders a NaN jd after every finite jd, and NaN jd among themselves by index, so that the counts of an object
// are always a permutation of 0 .. size - 1.  A NaN jd is never <= anything: is_rise is 0 for that alert, and for the
// whole object when jd[m] is NaN.  Every comparison is a float64 compare-and-select, never fmin.  perm entries outside
// [0, n_alerts) are skipped: they count nowhere and nothing is stored for them.
#include "object_walk.h"

#include <climits>

namespace {

using object_walk::WG;

struct Inputs {
  const int32_t* perm;
  const double* jd;
  const double* mag;
  int32_t* pos;
  int32_t* size;
  int32_t* first_row;
  int32_t* later;
  uint8_t* is_rise;
  double* peakmag;
  int n_alerts;
};

// what one alert knows about its object so far
struct Acc {
  double pm, pjd;   // min magpsf over O(i) and the jd of its lowest row
  int pa;           // that row
  int pos, size, first, later;
  __device__ void init() {
    pm = pjd = __builtin_nan("");
    pa = first = INT_MAX;
    pos = size = later = 0;
  }
  // alert (kjd, kmag, ka) of the same object seen from alert (myjd, mya); ka < 0: no alert in this slot
  __device__ __forceinline__ void take(double kjd, double kmag, int ka, double myjd, int mya) {
    if (ka < 0) return;
    size += 1;
    pos += ka < mya;
    first = ka < first ? ka : first;
    const bool knan = kjd != kjd, mynan = myjd != myjd;
    later += knan ? (!mynan || ka > mya) : (!mynan && (kjd > myjd || (kjd == myjd && ka > mya)));
    if (kmag == kmag && (!(pm <= kmag) || (kmag == pm && ka < pa))) {   // (a NaN running value is replaced)
      pm = kmag;
      pjd = kjd;
      pa = ka;
    }
  }
  __device__ __forceinline__ void store(const Inputs& in, int a, double myjd) const {
    in.pos[a] = pos;
    in.size[a] = size;
    in.first_row[a] = first;
    in.later[a] = later;
    in.is_rise[a] = pm == pm && myjd <= pjd;
    in.peakmag[a] = pm;
  }
};

__global__ __launch_bounds__(WG) void split_labels_kernel(Inputs in, const int32_t* __restrict__ seg_offsets,
                                                          int n_objects) {
  object_walk::walk<Acc>(in, seg_offsets, n_objects);
}

}  // namespace

extern "C" int btsbot_split_labels(const int32_t* perm, const int32_t* seg_offsets, int n_alerts, int n_objects,
                                   const double* jd, const double* magpsf, int32_t* pos, int32_t* size,
                                   int32_t* first_row, int32_t* later, uint8_t* is_rise, double* peakmag,
                                   void* stream) {
  TRY(object_walk::check_args("split_labels",
                              perm != nullptr && seg_offsets != nullptr && jd != nullptr && magpsf != nullptr &&
                                  pos != nullptr && size != nullptr && first_row != nullptr && later != nullptr &&
                                  is_rise != nullptr && peakmag != nullptr,
                              n_alerts, n_objects));
  unsigned blocks;
  TRY(object_walk::grid("split_labels", n_alerts, n_objects, &blocks));
  if (blocks == 0) return BTSBOT_OK;
  const Inputs in{perm, jd, magpsf, pos, size, first_row, later, is_rise, peakmag, n_alerts};
  hipLaunchKernelGGL(split_labels_kernel, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, in, seg_offsets, n_objects);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
