// The skeleton shared by the per-object streaming states (trigger_state.hip, feature_state.hip): an open-addressing table
// of object ids on the device, and the one-wave-per-run walk over a grouped batch that advances its records.  What a
// record holds, and what an alert does to it, is the state's own; everything below is the same for every state.
//
// Table: `capacity` slots, capacity a power of two, one array per field; key[slot] is the object id, FREE_KEY a free slot
// (which is why that id is reserved).  Find or claim: slot = mix64(id) & (capacity - 1), linear probing with wrap-around,
// at most `capacity` probes; a free slot is claimed with a 64-bit atomicCAS on key (a vector global atomic).  A key never
// changes once set, so a plain read that sees another object's id may move on, and one that sees "free" is settled by the
// CAS.  A state's reset kernel writes the empty record into every slot, so a claim initialises nothing and needs no
// ordering beyond the CAS; the runs of one launch are distinct objects, so a slot's payload has one owner per launch
// (payloads of earlier launches are visible through stream order).
//
// Update: the batch arrives grouped (perm: alert indices sorted by (object id, jd, input position); seg_offsets: n_runs + 1
// offsets into perm, empty runs allowed, so that the number of objects costs no host read).  One wave per run, one alert
// per lane, 64 alerts per step, RUNS_PER_WG runs per workgroup, no LDS:
//   open_run     the run's bounds (an empty run ends there) and its slot: lane 0 probes, every lane learns the answer
//   drop_run     a run without a slot (table full, or the reserved id) changes nothing in the table: dropped = 1 and the
//                state's fill for each of its alerts
//   step_alert   this lane's alert of the step, or none
//   late_step    late alerts: jd below the largest jd seen before them (the slot's, the earlier steps', the lower lanes')
// The record is wave-uniform: carried from the slot into the first step, from step to step and back into the slot by
// lane 0.  Every per-alert output is written by its own alert's lane, once.
//
// Load: one thread per record, the same find-or-claim; the first writer keeps a slot (load_claim).
//
// Rehash (retention: expire, resize): nothing is ever deleted in place -- a linear-probing chain with a hole in it loses
// the objects behind the hole, and a tombstone would be a key that changes.  The survivors of one table are inserted
// into a second, freshly reset one, of any capacity, with the same find-or-claim (rehash_walk): one thread per source
// slot in a grid-stride loop, key and last_jd read coalesced, the record copied by the thread that claimed its slot.
// The source is only read, so a rehash that does not fit leaves it whole.
//
// Counters: C_ROWS rows of C_STRIDE int64 (one cache line each) whose column sums are the counters; a workgroup adds to
// row blockIdx.x % C_ROWS, so the waves of a large launch do not all queue at one address.
#pragma once
#include <climits>

#include "common.h"

namespace object_table {

constexpr long long FREE_KEY = LLONG_MIN;   // BTSBOT_TRIGGER_FREE: the key of a free slot, the one id a table cannot hold
constexpr int WG = 256, RUNS_PER_WG = WG / 64;
enum {
  C_OBJECTS = 0,
  C_TAKEN = 1,
  C_DROPPED = 2,
  C_LATE = 3,
  C_LOAD_PRESENT = 4,
  C_LOAD_NO_SLOT = 5,
  C_EXPIRED = 6,        // objects a rehash left behind
  C_MOVE_NO_SLOT = 7    // survivors a rehash found no slot for (a smaller destination)
};
constexpr int C_ROWS = BTSBOT_TRIGGER_COUNTER_ROWS, C_STRIDE = 8;

__device__ __forceinline__ void count(int64_t* counters, int which, long long by) {
  if (by != 0)
    atomicAdd((unsigned long long*)(counters + (blockIdx.x % C_ROWS) * C_STRIDE + which), (unsigned long long)by);
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {   // splitmix64's finaliser
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the slot of `id` (never FREE_KEY) in key[0 .. capacity), claimed when the id is new; -1: no free slot within
// `capacity` probes
__device__ inline int find_or_claim(int64_t* key, int capacity, long long id, bool& claimed) {
  claimed = false;
  const unsigned mask = (unsigned)capacity - 1u;
  unsigned idx = (unsigned)mix64((unsigned long long)id) & mask;
  for (int probe = 0; probe < capacity; ++probe, idx = (idx + 1u) & mask) {
    long long k = __atomic_load_n((const long long*)(key + idx), __ATOMIC_RELAXED);
    if (k == FREE_KEY) {
      k = (long long)atomicCAS((unsigned long long*)(key + idx), (unsigned long long)FREE_KEY, (unsigned long long)id);
      if (k == FREE_KEY) {
        claimed = true;
        return (int)idx;
      }
    }
    if (k == id) return (int)idx;
  }
  return -1;
}

// Run `run` of the batch: perm[s .. e) with s, e clamped to [0, n_alerts]; e <= s: an empty run, nothing else was read.
// slot (wave-uniform): the record of the run's object, claimed (and counted) when the object is new; -1: no free slot, or
// the reserved id.
struct Run {
  int s, e, slot;
};

__device__ __forceinline__ Run open_run(const int32_t* seg_offsets, long run, const int32_t* perm, const int64_t* id,
                                        int n_alerts, int64_t* key, int capacity, int64_t* counters) {
  int s = seg_offsets[run], e = seg_offsets[run + 1];
  s = s < 0 ? 0 : s > n_alerts ? n_alerts : s;
  e = e < 0 ? 0 : e > n_alerts ? n_alerts : e;
  int slot = -1;
  if (e <= s) return {s, e, slot};
  const int a0 = perm[s];
  long long oid = FREE_KEY;
  if ((unsigned)a0 < (unsigned)n_alerts) oid = id[a0];
  if ((threadIdx.x & 63) == 0 && oid != FREE_KEY) {
    bool claimed;
    slot = find_or_claim(key, capacity, oid, claimed);
    if (claimed) count(counters, C_OBJECTS, 1);
  }
  return {s, e, __shfl(slot, 0)};
}

// The run changes nothing in the table: dropped = 1 and fill(a) for each of its alerts, which are counted.  (Let fill
// capture what it needs by value: with a reference to the kernel's argument struct hipcc gives trigger_update_kernel<16>
// 81 VGPRs for 80, one wave per SIMD fewer.)
template <class Fill>
__device__ __forceinline__ void drop_run(int s, int e, const int32_t* perm, int n_alerts, uint8_t* dropped,
                                         int64_t* counters, Fill fill) {
  const int lane = threadIdx.x & 63;
  int n_dropped = 0;
  for (int p = s + lane; p < e; p += 64) {
    const int a = perm[p];
    if ((unsigned)a >= (unsigned)n_alerts) continue;
    dropped[a] = 1;
    fill(a);
    ++n_dropped;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) n_dropped += __shfl_xor(n_dropped, d);
  if (lane == 0) count(counters, C_DROPPED, n_dropped);
}

// This lane's alert of the step that starts at perm[b0]; on = false (and -1): past the run's end, or no alert index.
// n_taken counts the step's alerts (wave-uniform).
__device__ __forceinline__ int step_alert(const int32_t* perm, int b0, int e, int n_alerts, bool& on, int& n_taken) {
  const int p = b0 + (threadIdx.x & 63);
  int a = p < e ? perm[p] : -1;
  if ((unsigned)a >= (unsigned)n_alerts) a = -1;
  on = a >= 0;
  n_taken += __popcll(__ballot(on));
  return a;
}

// The step's late alerts: jd below `last`, the largest jd seen before the step, or below a lower lane's; an exclusive
// prefix maximum, six shuffles.  Advances `last` over the step (wave-uniform).
__device__ __forceinline__ int late_step(bool on, double jd, double& last) {
  const int lane = threadIdx.x & 63;
  double upto = on ? jd : -__builtin_inf();   // inclusive prefix maximum
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(upto, d);
    if (lane >= d) upto = fmax(upto, o);
  }
  double before = __shfl_up(upto, 1);
  before = lane == 0 ? last : fmax(before, last);
  const int n_late = __popcll(__ballot(on && jd < before));
  last = fmax(last, __shfl(upto, 63));
  return n_late;
}

// The slot a loaded record is to be written into, claimed and counted as an object; -1, counted: no slot (or the reserved
// id), or the id is in the table already or twice in this record set -- the first writer keeps the slot.
__device__ __forceinline__ int load_claim(int64_t* key, int capacity, int64_t* counters, long long oid) {
  bool claimed = false;
  const int slot = oid == FREE_KEY ? -1 : find_or_claim(key, capacity, oid, claimed);
  if (slot < 0) {
    count(counters, C_LOAD_NO_SLOT, 1);
    return -1;
  }
  if (!claimed) {
    count(counters, C_LOAD_PRESENT, 1);
    return -1;
  }
  count(counters, C_OBJECTS, 1);
  return slot;
}

// The sweep of a rehash: source slot i is free (nothing), expired (last_jd < keep_from, written in exactly this form: a
// NaN last_jd is kept, a NaN or -inf keep_from expires nothing, +inf everything whose last_jd is a number) or a survivor,
// which claims a slot of the destination and has copy(i, slot) move its record.  Source keys are distinct and the
// destination was reset, so a survivor claims or finds no slot; one that finds its id there already (a destination that
// was not reset) is counted with those that found none and overwrites nothing.  Each thread counts in registers, each
// wave adds its three sums once.  Destination counters: objects = survivors moved, C_EXPIRED, C_MOVE_NO_SLOT, and the
// source's taken, dropped, late and expired entries added row by row, so the column sums go on across the rehash.
template <class Copy>
__device__ __forceinline__ void rehash_walk(const int64_t* __restrict__ src_key, const double* __restrict__ src_last_jd,
                                            int src_capacity, const int64_t* __restrict__ src_counters,
                                            int64_t* dst_key, int dst_capacity, int64_t* dst_counters, double keep_from,
                                            Copy copy) {
  const long stride = (long)gridDim.x * WG;
  const long i0 = (long)blockIdx.x * WG + threadIdx.x;
  int n_moved = 0, n_expired = 0, n_no_slot = 0;
  for (long i = i0; i < src_capacity; i += stride) {
    const long long id = src_key[i];
    const double last = src_last_jd[i];
    if (id == FREE_KEY) continue;
    if (last < keep_from) {
      ++n_expired;
      continue;
    }
    bool claimed;
    const int slot = find_or_claim(dst_key, dst_capacity, id, claimed);
    if (slot < 0 || !claimed) {
      ++n_no_slot;
      continue;
    }
    copy(i, slot);
    ++n_moved;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    n_moved += __shfl_xor(n_moved, d);
    n_expired += __shfl_xor(n_expired, d);
    n_no_slot += __shfl_xor(n_no_slot, d);
  }
  if ((threadIdx.x & 63) == 0) {
    count(dst_counters, C_OBJECTS, n_moved);
    count(dst_counters, C_EXPIRED, n_expired);
    count(dst_counters, C_MOVE_NO_SLOT, n_no_slot);
  }
  if (i0 < C_ROWS * C_STRIDE) {   // (the first workgroup; atomic, because the waves above add to C_EXPIRED too)
    const int column = (int)(i0 % C_STRIDE);
    const long long carried = src_counters[i0];
    if ((column == C_TAKEN || column == C_DROPPED || column == C_LATE || column == C_EXPIRED) && carried != 0)
      atomicAdd((unsigned long long*)(dst_counters + i0), (unsigned long long)carried);
  }
}

// ---- host side
// a table and each of the named arrays of it is there, and its capacity is a power of two
template <class Table, class... Array>
bool common_table_ok(const char* who, const Table* t, Array* Table::*... arrays) {
  if (t == nullptr || ((t->*arrays == nullptr) || ...)) {
    btsbot_set_error("%s: NULL table or NULL table array", who);
    return false;
  }
  if (t->capacity < 1 || (t->capacity & (t->capacity - 1)) != 0) {
    btsbot_set_error("%s: capacity must be a power of two, got %d", who, t->capacity);
    return false;
  }
  return true;
}

// what a rehash asks beyond two good tables: two different ones
template <class Table>
bool rehash_ok(const char* who, const Table* src, const Table* dst) {
  if (src->key == dst->key) {
    btsbot_set_error("%s: src and dst share the key array (a rehash is never in place)", who);
    return false;
  }
  return true;
}

// grids of WG threads: one thread per element in a grid-stride loop, one thread per record, one wave per run
inline unsigned blocks_strided(long n) {
  const long blocks = (n + WG - 1) / WG;
  return (unsigned)(blocks < 4096 ? blocks : 4096);
}
inline unsigned blocks_per_record(long n) { return (unsigned)((n + WG - 1) / WG); }
inline unsigned blocks_per_run(long n_runs) { return (unsigned)((n_runs + RUNS_PER_WG - 1) / RUNS_PER_WG); }

}  // namespace object_table
