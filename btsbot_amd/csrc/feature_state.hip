// btsbot_feature_update / _reset / _load / _rehash: the light-curve columns of alert_features.hip for a live stream.
// alert_features answers "what are peakmag_so_far, maxmag_so_far, age, days_since_peak, days_to_peak of this alert" from
// the alerts of its object that are in the same call; here the object's history is a record in a hash table on the
// device, and one launch per batch advances the records and writes the batch's rows.  The six columns a model reads are
// causal (they depend on the object's alerts up to and including the current one), so the record is a complete summary:
// a time-ordered stream cut into batches anywhere gives columns 2-7 of alert_features over the whole, bit for bit -- every
// output is a selection or one float64 subtraction rounded to float32 once at the store.
//
// Record of one object (struct btsbot_feature_table: one array per field, `capacity` slots, capacity a power of two):
//   key       int64   the object id; BTSBOT_TRIGGER_FREE (INT64_MIN) = free slot, which is why that id is reserved
//   n_alerts  int32   alerts taken
//   first_jd  double  the smallest jd seen; +inf before
//   last_jd   double  the largest jd seen; -inf before
//   peak_mag  double  the smallest magpsf seen, NaN skipped; NaN until a magnitude is seen
//   peak_jd   double  the jd peak_mag was first reached at: the (magpsf, jd, taking order) minimum; NaN with peak_mag
//   max_mag   double  the largest magpsf seen, NaN skipped; NaN until a magnitude is seen
//
// The table, the walk over a grouped batch (one wave per run, one alert per lane, 64 alerts per step), the dropped runs,
// the late scan, the counters and the load protocol are object_table.h's, shared with trigger_state.hip.  A dropped run's
// alerts get all-NaN rows.
//
// Update, what is particular to light curves: what the rule needs at alert l is the record after the alerts of lanes
// <= l: an inclusive prefix minimum of jd, an inclusive prefix maximum of magpsf and the inclusive prefix (magpsf, jd,
// lane) minimum, NaN magnitudes skipped -- shuffle scans of six steps each (the lower lane wins a tie, which is the taking
// order), then combined with the carry, which is older than every lane.  From step to step lane 63's prefix is the
// step's total: lanes past the run's end hold the neutral element.  Every row is written by its own alert's lane, once,
// as two float4 stores.
#include "common.h"
#include "object_table.h"

namespace {

using namespace object_table;

struct Batch {
  const int32_t* perm;
  const int64_t* id;
  const double* jd;
  const double* mag;
  const double* jsh;
  const int32_t* ncov;
  const int32_t* ndet;
  float* out;
  uint8_t* dropped;
  int n_alerts;
};

// the older maximum `o` against the younger `v`, NaN = none: v replaces o when it is higher
__device__ __forceinline__ double keep_max(double o, double v) { return (o == o && !(v > o)) ? o : v; }

// the older peak (om, oj) against the younger (m, j), NaN magnitude = none: the younger replaces the older when it is
// lower, or equal with a lower jd
__device__ __forceinline__ void keep_peak(double om, double oj, double& m, double& j) {
  if (om == om && !(m < om || (m == om && j < oj))) {
    m = om;
    j = oj;
  }
}

__global__ __launch_bounds__(WG) void feature_update_kernel(btsbot_feature_table t, Batch in,
                                                            const int32_t* __restrict__ seg_offsets, int n_runs) {
  const int lane = threadIdx.x & 63;
  const long run = (long)blockIdx.x * RUNS_PER_WG + (threadIdx.x >> 6);
  if (run >= n_runs) return;
  const Run r = open_run(seg_offsets, run, in.perm, in.id, in.n_alerts, t.key, t.capacity, t.counters);
  if (r.e <= r.s) return;
  const int slot = r.slot;
  if (slot < 0) {   // table full, or the reserved id
    drop_run(r.s, r.e, in.perm, in.n_alerts, in.dropped, t.counters, [out = in.out](int a) {
      const float nan = __builtin_nanf("");
      float4* o = reinterpret_cast<float4*>(out + (long)a * 8);
      o[0] = make_float4(nan, nan, nan, nan);
      o[1] = make_float4(nan, nan, nan, nan);
    });
    return;
  }

  // ---- the record so far (wave-uniform)
  const int n_seen = t.n_alerts[slot];
  double first = t.first_jd[slot], last = t.last_jd[slot];
  double pk = t.peak_mag[slot], pkjd = t.peak_jd[slot], mx = t.max_mag[slot];
  int n_late = 0, n_taken = 0;

  for (int b0 = r.s; b0 < r.e; b0 += 64) {
    bool on;
    const int a = step_alert(in.perm, b0, r.e, in.n_alerts, on, n_taken);
    const double jd = on ? in.jd[a] : 0.0;
    const double mag = on ? in.mag[a] : __builtin_nan("");
    n_late += late_step(on, jd, last);

    // the record after this lane's alert: three inclusive prefixes, then the carry
    double lo = on ? jd : __builtin_inf();      // first_jd
    double hi = mag;                            // max_mag
    double pm = mag, pj = mag == mag ? jd : __builtin_nan("");   // (peak_mag, peak_jd)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double olo = __shfl_up(lo, d), ohi = __shfl_up(hi, d), om = __shfl_up(pm, d), oj = __shfl_up(pj, d);
      if (lane >= d) {
        lo = olo < lo ? olo : lo;
        hi = keep_max(ohi, hi);
        keep_peak(om, oj, pm, pj);
      }
    }
    lo = first < lo ? first : lo;
    hi = keep_max(mx, hi);
    keep_peak(pk, pkjd, pm, pj);

    if (on) {
      const double jsh = in.jsh[a];
      const double fst = jsh != jsh ? jsh : (jsh < lo ? jsh : lo);   // (compare-and-select: a NaN jdstarthist stays NaN)
      float4* o = reinterpret_cast<float4*>(in.out + (long)a * 8);
      o[0] = make_float4((float)pm, (float)hi, (float)pm, (float)hi);
      o[1] = make_float4((float)(jd - fst), (float)(jd - pj), (float)(pj - fst),
                         (float)((double)in.ncov[a] - (double)in.ndet[a]));
      in.dropped[a] = 0;
    }

    // lane 63's record is the record after the step
    first = __shfl(lo, 63);
    mx = __shfl(hi, 63);
    pk = __shfl(pm, 63);
    pkjd = __shfl(pj, 63);
  }

  if (lane == 0) {
    t.n_alerts[slot] = n_seen + n_taken;
    t.first_jd[slot] = first;
    t.last_jd[slot] = last;
    t.peak_mag[slot] = pk;
    t.peak_jd[slot] = pkjd;
    t.max_mag[slot] = mx;
    count(t.counters, C_TAKEN, n_taken);
    count(t.counters, C_LATE, n_late);
  }
}

__global__ __launch_bounds__(WG) void feature_reset_kernel(btsbot_feature_table t) {
  const long stride = (long)gridDim.x * WG;
  const long i0 = (long)blockIdx.x * WG + threadIdx.x;
  for (long i = i0; i < t.capacity; i += stride) {
    t.key[i] = FREE_KEY;
    t.n_alerts[i] = 0;
    t.first_jd[i] = __builtin_inf();
    t.last_jd[i] = -__builtin_inf();
    t.peak_mag[i] = __builtin_nan("");
    t.peak_jd[i] = __builtin_nan("");
    t.max_mag[i] = __builtin_nan("");
  }
  if (i0 < C_ROWS * C_STRIDE) t.counters[i0] = 0;
}

struct Records {
  const int64_t* id;
  const int32_t* n_alerts;
  const double* first_jd;
  const double* last_jd;
  const double* peak_mag;
  const double* peak_jd;
  const double* max_mag;
};

__global__ __launch_bounds__(WG) void feature_load_kernel(btsbot_feature_table t, int m, Records rec) {
  const long r = (long)blockIdx.x * WG + threadIdx.x;
  if (r >= m) return;
  const int slot = load_claim(t.key, t.capacity, t.counters, rec.id[r]);
  if (slot < 0) return;
  t.n_alerts[slot] = rec.n_alerts[r];
  t.first_jd[slot] = rec.first_jd[r];
  t.last_jd[slot] = rec.last_jd[r];
  t.peak_mag[slot] = rec.peak_mag[r];
  t.peak_jd[slot] = rec.peak_jd[r];
  t.max_mag[slot] = rec.max_mag[r];
}

// The survivors of src (last_jd >= keep_from, or NaN) into the freshly reset dst: object_table.h's rehash_walk.
__global__ __launch_bounds__(WG) void feature_rehash_kernel(btsbot_feature_table src, btsbot_feature_table dst,
                                                            double keep_from) {
  rehash_walk(src.key, src.last_jd, src.capacity, src.counters, dst.key, dst.capacity, dst.counters, keep_from,
              [src, dst](long i, int slot) {
                dst.n_alerts[slot] = src.n_alerts[i];
                dst.first_jd[slot] = src.first_jd[i];
                dst.last_jd[slot] = src.last_jd[i];
                dst.peak_mag[slot] = src.peak_mag[i];
                dst.peak_jd[slot] = src.peak_jd[i];
                dst.max_mag[slot] = src.max_mag[i];
              });
}

// NULL arrays, a capacity that is no power of two
bool table_ok(const char* who, const btsbot_feature_table* t) {
  using T = btsbot_feature_table;
  return common_table_ok(who, t, &T::key, &T::n_alerts, &T::first_jd, &T::last_jd, &T::peak_mag, &T::peak_jd, &T::max_mag,
                         &T::counters);
}

}  // namespace

extern "C" int btsbot_feature_reset(const btsbot_feature_table* table, void* stream) {
  if (!table_ok("feature_reset", table)) return BTSBOT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(feature_reset_kernel, dim3(blocks_strided(table->capacity)), dim3(WG), 0, (hipStream_t)stream,
                     *table);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_feature_update(const btsbot_feature_table* table, const int32_t* perm, const int32_t* seg_offsets,
                                     int n_alerts, int n_runs, const int64_t* object_id, const double* jd,
                                     const double* magpsf, const double* jdstarthist, const int32_t* ncovhist,
                                     const int32_t* ndethist, float* out8, uint8_t* dropped, void* stream) {
  if (!table_ok("feature_update", table)) return BTSBOT_ERR_INVALID_ARG;
  if (perm == nullptr || seg_offsets == nullptr || object_id == nullptr || jd == nullptr || magpsf == nullptr ||
      jdstarthist == nullptr || ncovhist == nullptr || ndethist == nullptr || out8 == nullptr || dropped == nullptr ||
      n_alerts < 0 || n_runs < 0) {
    btsbot_set_error("feature_update: NULL argument or negative n_alerts / n_runs");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_alerts == 0) return BTSBOT_OK;
  if (((uintptr_t)out8 & 15) != 0) {
    btsbot_set_error("feature_update: out8 must be 16-byte aligned");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_runs == 0) {
    btsbot_set_error("feature_update: %d alerts in 0 runs", n_alerts);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const Batch in{perm, object_id, jd, magpsf, jdstarthist, ncovhist, ndethist, out8, dropped, n_alerts};
  hipLaunchKernelGGL(feature_update_kernel, dim3(blocks_per_run(n_runs)), dim3(WG), 0, (hipStream_t)stream, *table, in,
                     seg_offsets, n_runs);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_feature_load(const btsbot_feature_table* table, int n_records, const int64_t* object_id,
                                   const int32_t* n_alerts, const double* first_jd, const double* last_jd,
                                   const double* peak_mag, const double* peak_jd, const double* max_mag, void* stream) {
  if (!table_ok("feature_load", table)) return BTSBOT_ERR_INVALID_ARG;
  if (object_id == nullptr || n_alerts == nullptr || first_jd == nullptr || last_jd == nullptr || peak_mag == nullptr ||
      peak_jd == nullptr || max_mag == nullptr || n_records < 0) {
    btsbot_set_error("feature_load: NULL argument or negative n_records");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_records == 0) return BTSBOT_OK;
  const Records rec{object_id, n_alerts, first_jd, last_jd, peak_mag, peak_jd, max_mag};
  hipLaunchKernelGGL(feature_load_kernel, dim3(blocks_per_record(n_records)), dim3(WG), 0, (hipStream_t)stream,
                     *table, n_records, rec);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_feature_rehash(const btsbot_feature_table* src, const btsbot_feature_table* dst, double keep_from_jd,
                                     void* stream) {
  if (!table_ok("feature_rehash", src) || !table_ok("feature_rehash", dst) || !rehash_ok("feature_rehash", src, dst))
    return BTSBOT_ERR_INVALID_ARG;
  hipLaunchKernelGGL(feature_rehash_kernel, dim3(blocks_strided(src->capacity)), dim3(WG), 0, (hipStream_t)stream, *src,
                     *dst, keep_from_jd);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
