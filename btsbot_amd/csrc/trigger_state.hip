// btsbot_trigger_update / _reset / _load / _rehash: the policies of policy_eval.hip for a live stream.  policy_eval answers "does
// (thr, cut, k, gate) fire on this object, and at which alert first" for a finished split; here the per-object history is
// a record in a hash table on the device, and one launch per scored batch advances the records and says which alerts a
// policy fires at NOW.  A policy is monotone along a light curve (it counts valid alerts so far and asks whether anything
// so far was at or below the gate), so the record is a complete summary: the final state of a time-ordered stream cut
// into batches anywhere equals policy_eval on the whole, bit for bit -- every output is a count or a copy of an input.
//
// Record of one object (struct btsbot_trigger_table: one array per field, `capacity` slots, capacity a power of two):
//   key        int64   the object id; BTSBOT_TRIGGER_FREE (INT64_MIN) = free slot, which is why that id is reserved
//   n_alerts   int32   alerts taken
//   min_magpsf double  NaN skipped; NaN until a magnitude is seen
//   last_jd    double  the largest jd seen; -inf before
//   count      int32 [n_policies]      valid alerts so far
//   trigger    double [n_policies][2]  (jd, magpsf) of the alert the policy fired at; (-1, -1) until it has
// "min_magpsf <= gate" is the bright flag of every gated policy, so no flag is stored.
//
// The table, the walk over a grouped batch (one wave per run, one alert per lane, 64 alerts per step), the dropped runs,
// the late scan, the counters and the load protocol are object_table.h's, shared with feature_state.hip.  A dropped run's
// alerts get fired = 0.
//
// Update, what is particular to policies: what the rule needs at alert l is a prefix over lanes <= l, and each is a
// ballot away:  count so far = carry + popcount(ballot(valid_q) & lanes <= l);  bright so far = carry min <= gate, or
// ballot(mag <= gate_q) & lanes <= l is not empty;  the firing alert is the lowest set lane of ballot(fires_q) unless the
// policy has fired before.  Counts, the minimum and the fired mask are wave-uniform and carried like the rest of the
// record.  Every fired element is written by its own alert's lane, once.
#include "common.h"
#include "object_table.h"

#include <climits>
#include <cmath>

namespace {

constexpr int MAXP = 16;   // policies per table
using namespace object_table;

struct Policies {
  double thr[MAXP], cut[MAXP], gate[MAXP];
  int k[MAXP];
  int n;
};

struct Batch {
  const int32_t* perm;
  const int64_t* id;
  const double* jd;
  const double* mag;
  const float* raw;
  uint8_t* fired;
  uint8_t* dropped;
  int n_alerts;
};

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fmin(v, __shfl_xor(v, d));
  return v;
}

template <int NP>
__global__ __launch_bounds__(WG) void trigger_update_kernel(btsbot_trigger_table t, Policies pol, Batch in,
                                                            const int32_t* __restrict__ seg_offsets, int n_runs) {
  const int lane = threadIdx.x & 63;
  const long run = (long)blockIdx.x * RUNS_PER_WG + (threadIdx.x >> 6);
  if (run >= n_runs) return;
  const Run r = open_run(seg_offsets, run, in.perm, in.id, in.n_alerts, t.key, t.capacity, t.counters);
  if (r.e <= r.s) return;
  const int np = t.n_policies, slot = r.slot;
  const unsigned long long le = ~0ull >> (63 - lane);   // lanes <= this one
  if (slot < 0) {   // table full, or the reserved id
    drop_run(r.s, r.e, in.perm, in.n_alerts, in.dropped, t.counters, [fired = in.fired, np](int a) {
      for (int q = 0; q < np; ++q) fired[(long)a * np + q] = 0;
    });
    return;
  }

  // ---- the record so far (wave-uniform)
  int n_seen = t.n_alerts[slot];
  double lo = t.min_magpsf[slot], last = t.last_jd[slot];
  int cnt[NP];
  unsigned done = 0;   // policies that have fired
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    cnt[q] = q < np ? t.count[(long)slot * np + q] : 0;
    if (q < np && t.trigger[((long)slot * np + q) * 2] >= 0.0) done |= 1u << q;
  }
  int n_late = 0, n_taken = 0;

  for (int b0 = r.s; b0 < r.e; b0 += 64) {
    bool on;
    const int a = step_alert(in.perm, b0, r.e, in.n_alerts, on, n_taken);
    const double jd = on ? in.jd[a] : 0.0;
    const double mag = on ? in.mag[a] : __builtin_nan("");
    const double score = on ? (double)in.raw[a] : 0.0;
    n_late += late_step(on, jd, last);

    unsigned mine = 0;   // policies that fire at this lane's alert
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      if (q < np) {   // (wave-uniform)
        const unsigned long long valid = __ballot(on && score > pol.thr[q] && mag < pol.cut[q]);
        const double g = pol.gate[q];
        const unsigned long long bright_at = __ballot(on && mag <= g);
        const bool bright = g != g || lo <= g || (bright_at & le) != 0;
        const int so_far = cnt[q] + __popcll(valid & le);
        const unsigned long long fires = __ballot(on && so_far >= pol.k[q] && bright);
        if (fires != 0 && !((done >> q) & 1u)) {
          done |= 1u << q;
          if (lane == __ffsll((long long)fires) - 1) {
            mine |= 1u << q;
            double* tr = t.trigger + ((long)slot * np + q) * 2;
            tr[0] = jd;
            tr[1] = mag;
          }
        }
        cnt[q] += __popcll(valid);
      }
    }
    if (on) {
      in.dropped[a] = 0;
      for (int q = 0; q < np; ++q) in.fired[(long)a * np + q] = (uint8_t)((mine >> q) & 1u);
    }

    // the minimum joins the carry after the policies have used the carry of the steps before
    const bool has = mag == mag;
    const double step_lo = wave_min(has ? mag : __builtin_inf());
    if (__ballot(has) != 0) lo = fmin(lo, step_lo);   // (fmin skips a NaN carry)
  }

  if (lane == 0) {
    t.n_alerts[slot] = n_seen + n_taken;
    t.min_magpsf[slot] = lo;
    t.last_jd[slot] = last;
    count(t.counters, C_TAKEN, n_taken);
    count(t.counters, C_LATE, n_late);
  }
#pragma unroll
  for (int q = 0; q < NP; ++q)
    if (lane == q && q < np) t.count[(long)slot * np + q] = cnt[q];
}

__global__ __launch_bounds__(WG) void trigger_reset_kernel(btsbot_trigger_table t) {
  const long stride = (long)gridDim.x * WG;
  const long i0 = (long)blockIdx.x * WG + threadIdx.x;
  for (long i = i0; i < t.capacity; i += stride) {
    t.key[i] = FREE_KEY;
    t.n_alerts[i] = 0;
    t.min_magpsf[i] = __builtin_nan("");
    t.last_jd[i] = -__builtin_inf();
  }
  const long cells = (long)t.capacity * t.n_policies;
  for (long i = i0; i < cells; i += stride) {
    t.count[i] = 0;
    t.trigger[2 * i] = -1.0;
    t.trigger[2 * i + 1] = -1.0;
  }
  if (i0 < C_ROWS * C_STRIDE) t.counters[i0] = 0;
}

__global__ __launch_bounds__(WG) void trigger_load_kernel(btsbot_trigger_table t, int m, const int64_t* __restrict__ id,
                                                          const int32_t* __restrict__ n_alerts,
                                                          const double* __restrict__ min_magpsf,
                                                          const double* __restrict__ last_jd,
                                                          const int32_t* __restrict__ cnt,
                                                          const double* __restrict__ trigger) {
  const long r = (long)blockIdx.x * WG + threadIdx.x;
  if (r >= m) return;
  const int slot = load_claim(t.key, t.capacity, t.counters, id[r]);
  if (slot < 0) return;
  t.n_alerts[slot] = n_alerts[r];
  t.min_magpsf[slot] = min_magpsf[r];
  t.last_jd[slot] = last_jd[r];
  const int np = t.n_policies;
  for (int q = 0; q < np; ++q) {
    t.count[(long)slot * np + q] = cnt[r * np + q];
    t.trigger[((long)slot * np + q) * 2] = trigger[(r * np + q) * 2];
    t.trigger[((long)slot * np + q) * 2 + 1] = trigger[(r * np + q) * 2 + 1];
  }
}

// The survivors of src (last_jd >= keep_from, or NaN) into the freshly reset dst, each with all its n_policies counts and
// trigger pairs: object_table.h's rehash_walk.
__global__ __launch_bounds__(WG) void trigger_rehash_kernel(btsbot_trigger_table src, btsbot_trigger_table dst,
                                                            double keep_from) {
  rehash_walk(src.key, src.last_jd, src.capacity, src.counters, dst.key, dst.capacity, dst.counters, keep_from,
              [src, dst](long i, int slot) {
                dst.n_alerts[slot] = src.n_alerts[i];
                dst.min_magpsf[slot] = src.min_magpsf[i];
                dst.last_jd[slot] = src.last_jd[i];
                const int np = src.n_policies;
                for (int q = 0; q < np; ++q) {
                  dst.count[(long)slot * np + q] = src.count[i * np + q];
                  dst.trigger[((long)slot * np + q) * 2] = src.trigger[(i * np + q) * 2];
                  dst.trigger[((long)slot * np + q) * 2 + 1] = src.trigger[(i * np + q) * 2 + 1];
                }
              });
}

// NULL arrays, a capacity that is no power of two, n_policies outside 1..16
bool table_ok(const char* who, const btsbot_trigger_table* t) {
  using T = btsbot_trigger_table;
  if (!common_table_ok(who, t, &T::key, &T::n_alerts, &T::min_magpsf, &T::last_jd, &T::count, &T::trigger, &T::counters))
    return false;
  if (t->n_policies < 1 || t->n_policies > MAXP) {
    btsbot_set_error("%s: n_policies must be 1..%d, got %d", who, MAXP, t->n_policies);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int btsbot_trigger_reset(const btsbot_trigger_table* table, void* stream) {
  if (!table_ok("trigger_reset", table)) return BTSBOT_ERR_INVALID_ARG;
  const long cells = (long)table->capacity * table->n_policies;
  hipLaunchKernelGGL(trigger_reset_kernel, dim3(blocks_strided(cells)), dim3(WG), 0, (hipStream_t)stream, *table);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_trigger_update(const btsbot_trigger_table* table, const double* policies, const int32_t* perm,
                                     const int32_t* seg_offsets, int n_alerts, int n_runs, const int64_t* object_id,
                                     const double* jd, const double* magpsf, const float* raw_pred, uint8_t* fired,
                                     uint8_t* dropped, void* stream) {
  if (!table_ok("trigger_update", table)) return BTSBOT_ERR_INVALID_ARG;
  if (policies == nullptr || perm == nullptr || seg_offsets == nullptr || object_id == nullptr || jd == nullptr ||
      magpsf == nullptr || raw_pred == nullptr || fired == nullptr || dropped == nullptr || n_alerts < 0 || n_runs < 0) {
    btsbot_set_error("trigger_update: NULL argument or negative n_alerts / n_runs");
    return BTSBOT_ERR_INVALID_ARG;
  }
  Policies pol;
  pol.n = table->n_policies;
  for (int q = 0; q < MAXP; ++q) {
    const bool used = q < pol.n;
    const double k = used ? policies[4 * q + 2] : 1.0;
    if (!(k >= 1.0) || k != std::floor(k)) {
      btsbot_set_error("trigger_update: policy %d: k must be an integer >= 1, got %g", q, k);
      return BTSBOT_ERR_INVALID_ARG;
    }
    pol.thr[q] = used ? policies[4 * q] : 0.0;
    pol.cut[q] = used ? policies[4 * q + 1] : 0.0;
    pol.gate[q] = used ? policies[4 * q + 3] : 0.0;
    pol.k[q] = k > (double)INT_MAX ? INT_MAX : (int)k;   // (more than a record can count: never fires)
  }
  if (n_alerts == 0) return BTSBOT_OK;
  if (n_runs == 0) {
    btsbot_set_error("trigger_update: %d alerts in 0 runs", n_alerts);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const Batch in{perm, object_id, jd, magpsf, raw_pred, fired, dropped, n_alerts};
  const unsigned blocks = blocks_per_run(n_runs);
  if (pol.n <= 4)
    hipLaunchKernelGGL(trigger_update_kernel<4>, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, *table, pol, in,
                       seg_offsets, n_runs);
  else
    hipLaunchKernelGGL(trigger_update_kernel<MAXP>, dim3(blocks), dim3(WG), 0, (hipStream_t)stream, *table, pol, in,
                       seg_offsets, n_runs);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_trigger_load(const btsbot_trigger_table* table, int n_records, const int64_t* object_id,
                                   const int32_t* n_alerts, const double* min_magpsf, const double* last_jd,
                                   const int32_t* count, const double* trigger, void* stream) {
  if (!table_ok("trigger_load", table)) return BTSBOT_ERR_INVALID_ARG;
  if (object_id == nullptr || n_alerts == nullptr || min_magpsf == nullptr || last_jd == nullptr || count == nullptr ||
      trigger == nullptr || n_records < 0) {
    btsbot_set_error("trigger_load: NULL argument or negative n_records");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_records == 0) return BTSBOT_OK;
  hipLaunchKernelGGL(trigger_load_kernel, dim3(blocks_per_record(n_records)), dim3(WG), 0, (hipStream_t)stream,
                     *table, n_records, object_id, n_alerts, min_magpsf, last_jd, count, trigger);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_trigger_rehash(const btsbot_trigger_table* src, const btsbot_trigger_table* dst, double keep_from_jd,
                                     void* stream) {
  if (!table_ok("trigger_rehash", src) || !table_ok("trigger_rehash", dst) || !rehash_ok("trigger_rehash", src, dst))
    return BTSBOT_ERR_INVALID_ARG;
  if (src->n_policies != dst->n_policies) {
    btsbot_set_error("trigger_rehash: n_policies differs: src %d, dst %d", src->n_policies, dst->n_policies);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(trigger_rehash_kernel, dim3(blocks_strided(src->capacity)), dim3(WG), 0, (hipStream_t)stream, *src,
                     *dst, keep_from_jd);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
