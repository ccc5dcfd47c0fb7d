// Shared types and host plumbing of libbtsbot_hip.so (gfx950 only); brings in launchers.h and device_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/btsbot_hip.h"

typedef __bf16 bf16_t;
typedef _Float16 f16_t;
struct fp8_t { unsigned char v; };   // tag of the fp8 (OCP e4m3) operand mode of stage2p.hip / stage3.hip
struct f16x2_t { _Float16 v; };      // tag of the split-operand mode (BTSBOT_F16X2): x = hi + lo, both f16
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4v;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2v;
constexpr float LN_EPS = 1e-6f;   // the LayerNorms of both networks

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) holds for ONE device: a launcher keeps one flag per (kernel, device),
// so a handle on cuda:1 after one on cuda:0 sets it again (a process-wide bool skipped it: launch failure on the second
// GPU for every kernel above 64 KB of LDS).  Racing threads may both set the attribute: harmless.
#include <atomic>
struct DevOnce {
  std::atomic<unsigned long long> mask{0};
  static int dev() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d & 63;
  }
  bool need() const { return ((mask.load(std::memory_order_relaxed) >> dev()) & 1ULL) == 0; }
  void done() { mask.fetch_or(1ULL << dev(), std::memory_order_relaxed); }
};

#include "schedule.h"   // the developer switches (BTSBOT_AMD_*): switch_on() / switch_int()

// ---------------------------------------------------------------------------------------
// error plumbing (no exception crosses the ABI)
// ---------------------------------------------------------------------------------------
void btsbot_set_error(const char* fmt, ...);

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      btsbot_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                       __LINE__);                                                       \
      return BTSBOT_ERR_HIP;                                                            \
    }                                                                                   \
  } while (0)

#define LAUNCH_CHECK()                                                                  \
  do {                                                                                  \
    hipError_t _e = hipGetLastError();                                                  \
    if (_e != hipSuccess) {                                                             \
      btsbot_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e),       \
                       __FILE__, __LINE__);                                             \
      return BTSBOT_ERR_HIP;                                                            \
    }                                                                                   \
  } while (0)

// status propagation: a btsbot_status other than BTSBOT_OK ends the calling function (or lambda) with it
#define TRY(call)                   \
  do {                              \
    int _s = (call);                \
    if (_s != BTSBOT_OK) return _s; \
  } while (0)

// every carved buffer (workspace, operand images, caches, scratch) starts on a 256-byte boundary
inline size_t align256(size_t bytes) { return (bytes + 255) / 256 * 256; }
inline size_t bump(size_t& cur, size_t bytes) {
  const size_t o = cur;
  cur += align256(bytes);
  return o;
}

// one stream-ordered allocation, carved into 256-byte aligned pieces: offsets are reserved first, alloc() makes the one
// allocation, and it is released behind the work on the same stream when the object goes out of scope (`who` names the
// entry point in the error text)
struct StreamScratch {
  hipStream_t st;
  const char* who;
  unsigned char* base = nullptr;
  size_t total = 0;
  StreamScratch(hipStream_t s, const char* w) : st(s), who(w) {}
  StreamScratch(const StreamScratch&) = delete;
  ~StreamScratch() {
    if (base != nullptr) (void)hipFreeAsync(base, st);
  }
  size_t reserve(size_t bytes) { return bump(total, bytes); }
  int alloc() {
    if (hipMallocAsync(reinterpret_cast<void**>(&base), total ? total : 256, st) == hipSuccess) return BTSBOT_OK;
    btsbot_set_error("%s: hipMallocAsync of %zu scratch bytes failed", who, total);
    return BTSBOT_ERR_HIP;
  }
  template <typename P = void> P* at(size_t off) const { return reinterpret_cast<P*>(base + off); }
};

#include "launchers.h"     // every launcher prototype, by defining source file
#include "device_math.h"   // the __device__ helpers
