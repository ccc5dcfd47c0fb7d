// The open-addressing object table shared by the per-object states (trigger_state.hip, feature_state.hip): where an
// object id lives in an array of `capacity` keys, capacity a power of two.
//
// Find or claim: slot = mix64(id) & (capacity - 1), linear probing with wrap-around, at most `capacity` probes; a free
// slot is claimed with a 64-bit atomicCAS on key (a vector global atomic).  A key never changes once set, so a plain read
// that sees another object's id may move on, and one that sees "free" is settled by the CAS.  The tables' reset kernels
// write the empty record into every slot, so a claim initialises nothing and needs no ordering beyond the CAS.
#pragma once
#include <climits>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace object_table {

constexpr long long FREE_KEY = LLONG_MIN;   // BTSBOT_TRIGGER_FREE: the key of a free slot, the one id a table cannot hold

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

}  // namespace object_table
