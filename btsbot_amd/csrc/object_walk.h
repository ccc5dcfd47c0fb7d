// The per-object walk of btsbot_alert_features, btsbot_split_labels and btsbot_policy_eval: every alert reduces over the
// alerts of its own object -- n^2 compare-and-selects per object, no sort, no atomics, one writer per output element.
//
// The caller has grouped the alerts by object (perm: alert indices, input order inside an object; seg_offsets: where
// each object's run starts).  A workgroup of four waves owns four consecutive objects and picks a form per object:
//   n <= 64         one wave, one alert per lane; the object's (jd, magpsf, index) go round as readlane broadcasts
//   n <= TILE       the workgroup stages the object in LDS once; each thread reduces its alerts over the tile (every lane
//                   reads the same LDS address: a broadcast, no bank conflicts)
//   n >  TILE       the same inner loop, 256 alerts at a time, the object streamed through the LDS tile once per batch
// The three forms make the same take() calls in the same order, so they give identical results.
//
// A kernel supplies its inputs In { const int32_t* perm; const double* jd; const double* mag; int n_alerts; ... } and an
// accumulator Acc: what one alert knows about its object so far, with
//   init()                               the empty object
//   take(kjd, kmag, ka, myjd, mya)       alert (kjd, kmag, ka) of the same object seen from alert (myjd, mya); called in
//                                        grouped order, once per slot of the object, invalid slots (ka = -1) included
//   store(in, mya, myjd)                 write alert mya's row (only called with mya >= 0)
//
// Two extensions, each free for the kernel that does not use it:
//   a payload word: In declares `using Word` (32 bits) and `Word word(a, mag) const`, computed when the alert is loaded
//     (an invalid slot: Word{}).  It travels with the record -- by readlane in the one-wave form, in one more LDS array in
//     the tile forms -- and take() gets it after ka.  Without In::Word there is no such array and no register.
//   a reducer Red: the result is per object, not per alert.  Instead of Acc::store the walk calls
//       init()                            the empty object
//       slot(kjd, kmag, ka)               once per slot, in grouped order, by every thread that walks the object alike
//                                         (the streamed form: in its first pass only)
//       alert_done(in, acc, myjd, mya)    an own alert whose accumulator is complete (mya = -1: none)
//       finish_wave / finish_workgroup(in, obj, s, n)    by the object's one wave (n <= 64) / by the whole workgroup:
//                                         reduce over it and write the row of object obj (n alerts from grouped position s)
//     for every object below n_objects, empty ones included (n = 0 takes the one-wave form); without a reducer empty
//     objects are skipped.  finish_workgroup may meet the other waves through LDS of its own behind its own barrier: a
//     workgroup barrier lies between one object's finish and anything the next object writes to LDS (the next object's
//     first __syncthreads() comes before it stages its tile; a finish of its own is further barriers away).
#pragma once
#include "common.h"

#include <type_traits>

namespace object_walk {

constexpr int TILE = 1024;   // alerts per LDS tile (alert_utils.OBJECT_TILE): 20 KB of LDS, 8 workgroups per CU
constexpr int WG = 256, OBJ_PER_WG = WG / 64;

struct NoWord {};
struct NoReducer {};
template <class In, class = void> struct WordOf { using type = NoWord; };
template <class In> struct WordOf<In, std::void_t<typename In::Word>> { using type = typename In::Word; };
template <class In> using word_t = typename WordOf<In>::type;

// the payload's LDS array (none without a payload), its accesses, its broadcast (k wave-uniform), and take() with it
template <class W> __device__ __forceinline__ W* word_tile() {
  if constexpr (!std::is_same_v<W, NoWord>) {
    __shared__ W s_w[TILE];
    return s_w;
  }
  return nullptr;
}
template <class W> __device__ __forceinline__ void word_put(W* s_w, int i, W w) {
  if constexpr (!std::is_same_v<W, NoWord>) s_w[i] = w;
}
template <class W> __device__ __forceinline__ W word_get(const W* s_w, int k) {
  if constexpr (std::is_same_v<W, NoWord>) return {};
  else return s_w[k];
}
template <class W> __device__ __forceinline__ W word_bcast(W w, int k) {
  static_assert(std::is_same_v<W, NoWord> || sizeof(W) == 4, "the payload is one 32-bit word");
  if constexpr (std::is_same_v<W, NoWord>) return w;
  else return (W)__builtin_amdgcn_readlane((int)w, k);
}
template <class Acc, class W>
__device__ __forceinline__ void take(Acc& c, double kjd, double kmag, int ka, W kw, double myjd, int mya) {
  if constexpr (std::is_same_v<W, NoWord>) c.take(kjd, kmag, ka, myjd, mya);
  else c.take(kjd, kmag, ka, kw, myjd, mya);
}

// alert p of the grouped order: its index (-1: p is outside the object, or perm holds no valid alert there), jd, magpsf
// and payload.  An invalid slot reads as (jd = +inf, magpsf = NaN, payload = Word{}).
template <class In>
__device__ __forceinline__ int load_alert(const In& in, int p, bool inside, double& jd, double& mag, word_t<In>& w) {
  int a = -1;
  jd = __builtin_inf();
  mag = __builtin_nan("");
  w = {};
  if (inside) {
    a = in.perm[p];
    if ((unsigned)a < (unsigned)in.n_alerts) {
      jd = in.jd[a];
      mag = in.mag[a];
      if constexpr (!std::is_same_v<word_t<In>, NoWord>) w = in.word(a, mag);
    } else {
      a = -1;
    }
  }
  return a;
}

// the body of a kernel launched with WG threads and ceil(n_objects / OBJ_PER_WG) workgroups
template <class Acc, class Red = NoReducer, class In>
__device__ __forceinline__ void walk(const In& in, const int32_t* __restrict__ seg_offsets, int n_objects) {
  using W = word_t<In>;
  constexpr bool REDUCE = !std::is_same_v<Red, NoReducer>;
  __shared__ double s_jd[TILE], s_mag[TILE];
  __shared__ int s_a[TILE];
  W* const s_w = word_tile<W>();
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
    if (n <= 64 && (REDUCE ? n >= 0 && obj0 + wave < n_objects : n > 0)) {
      double myjd, mymag;
      W myw;
      const int mya = load_alert(in, s + lane, lane < n, myjd, mymag, myw);
      Acc c;
      c.init();
      [[maybe_unused]] Red red;
      if constexpr (REDUCE) red.init();
      for (int k = 0; k < n; ++k) {
        const double kjd = lane_bcast(myjd, k), kmag = lane_bcast(mymag, k);
        const int ka = __builtin_amdgcn_readlane(mya, k);
        take(c, kjd, kmag, ka, word_bcast(myw, k), myjd, mya);
        if constexpr (REDUCE) red.slot(kjd, kmag, ka);
      }
      if constexpr (REDUCE) {
        red.alert_done(in, c, myjd, mya);
        red.finish_wave(in, obj0 + wave, s, n);
      } else if (mya >= 0) {
        c.store(in, mya, myjd);
      }
    }
  }

  // ---- one workgroup per object, n > 64 (every condition below is uniform over the workgroup)
  for (int q = 0; q < OBJ_PER_WG; ++q) {
    const int s = off[q], n = off[q + 1] - s;
    if (n <= 64) continue;
    [[maybe_unused]] Red red;
    if constexpr (REDUCE) red.init();
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
          W w;
          s_a[i] = load_alert(in, s + t0 + i, true, jd, mag, w);
          s_jd[i] = jd;
          s_mag[i] = mag;
          word_put(s_w, i, w);
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
            const W kw = word_get(s_w, k);
#pragma unroll
            for (int r = 0; r < OWN; ++r) take(c[r], kjd, kmag, ka, kw, myjd[r], mya[r]);
            if constexpr (REDUCE) red.slot(kjd, kmag, ka);
          }
        } else {
          if (t0 == 0) {
            double mag;
            W w;
            mya[0] = load_alert(in, s + b0 + threadIdx.x, (int)threadIdx.x < bn, myjd[0], mag, w);
          }
          for (int k = 0; k < tn; ++k) {
            const double kjd = s_jd[k], kmag = s_mag[k];
            const int ka = s_a[k];
            take(c[0], kjd, kmag, ka, word_get(s_w, k), myjd[0], mya[0]);
            if constexpr (REDUCE)
              if (b0 == 0) red.slot(kjd, kmag, ka);                 // (complete after any one pass over the object)
          }
        }
      }
      // the own alerts are complete: OWN of them in the one-pass form, one in the streamed form
      if constexpr (REDUCE) {
#pragma unroll
        for (int r = 0; r < OWN; ++r) {
          if (r > 0 && n > TILE) break;
          red.alert_done(in, c[r], myjd[r], mya[r]);
        }
      } else if (n <= TILE) {
#pragma unroll
        for (int r = 0; r < OWN; ++r)
          if (mya[r] >= 0) c[r].store(in, mya[r], myjd[r]);
      } else if (mya[0] >= 0) {
        c[0].store(in, mya[0], myjd[0]);
      }
    }
    if constexpr (REDUCE) red.finish_workgroup(in, obj0 + q, s, n);
  }
}

// ---- the host side of the three entries (`who`: the entry's name in the error text)
// the NULL / negative check on the grouping and on the entry's own pointers (all_pointers: none of them is NULL)
inline int check_args(const char* who, bool all_pointers, int n_alerts, int n_objects) {
  if (all_pointers && n_alerts >= 0 && n_objects >= 0) return BTSBOT_OK;
  btsbot_set_error("%s: NULL argument or negative n_alerts / n_objects", who);
  return BTSBOT_ERR_INVALID_ARG;
}
// the launch's workgroups; 0 with BTSBOT_OK: an empty batch, nothing to launch
inline int grid(const char* who, int n_alerts, int n_objects, unsigned* blocks) {
  *blocks = 0;
  if (n_alerts == 0) return BTSBOT_OK;
  if (n_objects == 0) {
    btsbot_set_error("%s: %d alerts in 0 objects", who, n_alerts);
    return BTSBOT_ERR_INVALID_ARG;
  }
  *blocks = (unsigned)(((long)n_objects + OBJ_PER_WG - 1) / OBJ_PER_WG);
  return BTSBOT_OK;
}

}  // namespace object_walk
