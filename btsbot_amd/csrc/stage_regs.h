// What the stage-0 and stage-1 megakernels (stage0b.hip, stage1b.hip) share: the residual stream of a lane's pixel as
// CT column blocks of the 32x32 MFMA's C/D layout -- x[ct][4 qd + e] = channel 32 ct + 8 qd + 4 h + e, h = lane >> 5,
// the partner lane ^ 32 holding the other half -- its LayerNorm and its way into the 16-bit [pixel][channel] image, and
// the two helpers of the filter ring.  CT is deduced from the argument; the channel count and the image's pitch follow.
#pragma once
#include "mfma.h"

template <int CT> struct StageRegs {
  static constexpr int C = 32 * CT;           // channels
  static constexpr int PITCH = 64 * CT + 16;  // bytes per pixel row of the 16-bit [pixel][channel] image
};

template <int N> __device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ int swz4(int row) {   // F[(row >> 2) & 3], F = {0,3,2,1}
  return (4 - ((row >> 2) & 3)) & 3;
}
// four fp32 words of LDS, read as a 16-bit vector: behind an LDS read of float type hipcc waits vmcnt(0) while an
// LDS-DMA is in flight (its type-based alias test takes the DMA for a possible writer of those words)
__device__ __forceinline__ f32x4 lds_f32x4(const float* q) {
  return __builtin_bit_cast(f32x4, *reinterpret_cast<const bf16x8*>(q));
}
// LayerNorm over the 32 CT channels of this lane's pixel (x[CT][16] here + the partner lane ^ 32)
// LDSW: weight and bias are words of LDS (lds_f32x4()).  They are read two column blocks at a time into 64 registers,
// the first pair in front of the statistics, whose arithmetic hides the round trip; the next pair behind the first
// pair's results (left to itself hipcc reads either everything first -- 128 registers, which spill beside a caller's
// prefetched filter fragments -- or each quad directly in front of its use).  The arithmetic is the same expression.
// done(ct) is called once column block ct of y is written: a caller with more than two column blocks stores them there
// (regs_to_map_ct), which is what keeps a pair's arithmetic in front of the next pair's reads.  (Pinning y itself as
// fp32 registers would do that too, but it changes bits: hipcc rounds the f16 forms' results to f16 inside the last
// fma -- v_fma_mix -- only where the fp32 value has no other use.)
struct LnNoSink {
  __device__ __forceinline__ void operator()(int) const {}
};
template <bool LDSW = false, int CT, typename F = LnNoSink>
__device__ __forceinline__ void ln_regs(const f32x16 (&x)[CT], const float* __restrict__ w,
                                        const float* __restrict__ b, int h, f32x16 (&y)[CT], F done = F()) {
  constexpr int C = StageRegs<CT>::C;
  f32x4 wq[LDSW ? 2 : 1][4], bq[LDSW ? 2 : 1][4];
  auto read_pair = [&](int ct0) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        if (ct0 + k >= CT) continue;
        wq[LDSW ? k : 0][qd] = lds_f32x4(w + (ct0 + k) * 32 + 8 * qd + 4 * h);
        bq[LDSW ? k : 0][qd] = lds_f32x4(b + (ct0 + k) * 32 + 8 * qd + 4 * h);
      }
    __builtin_amdgcn_sched_barrier(0);
  };
  if (LDSW) read_pair(0);
  float s = 0.f;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += x[ct][r];
  s += __shfl_xor(s, 32, 64);
  const float mean = s * (1.0f / C);
  float q = 0.f;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float d = x[ct][r] - mean;
      q += d * d;
    }
  q += __shfl_xor(q, 32, 64);
  const float rstd = rsqrtf(q * (1.0f / C) + LN_EPS);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    if (LDSW && ct > 0 && ct % 2 == 0) {   // the last pair is stored (done) in front of the next pair's reads
      __builtin_amdgcn_sched_barrier(0);
      read_pair(ct);
    }
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int c = ct * 32 + 8 * qd + 4 * h;
      float4 wv, bv;
      if (LDSW) {
        const f32x4 w4 = wq[LDSW ? ct & 1 : 0][qd], b4 = bq[LDSW ? ct & 1 : 0][qd];
        wv = make_float4(w4[0], w4[1], w4[2], w4[3]);
        bv = make_float4(b4[0], b4[1], b4[2], b4[3]);
      } else {
        wv = *reinterpret_cast<const float4*>(w + c);
        bv = *reinterpret_cast<const float4*>(b + c);
      }
      y[ct][4 * qd + 0] = (x[ct][4 * qd + 0] - mean) * rstd * wv.x + bv.x;
      y[ct][4 * qd + 1] = (x[ct][4 * qd + 1] - mean) * rstd * wv.y + bv.y;
      y[ct][4 * qd + 2] = (x[ct][4 * qd + 2] - mean) * rstd * wv.z + bv.z;
      y[ct][4 * qd + 3] = (x[ct][4 * qd + 3] - mean) * rstd * wv.w + bv.w;
    }
    done(ct);
  }
}

// LOPLANE > 0: also the values' f16 remainders, LOPLANE bytes behind (split mode)
// (one column block)
template <typename T, int LOPLANE, int CT>
__device__ __forceinline__ void regs_to_map_ct(const f32x16 (&x)[CT], unsigned char* map, int p, int h, int ct) {
  constexpr int PITCH = StageRegs<CT>::PITCH;
  typedef T T4 __attribute__((ext_vector_type(4)));
  {
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      T4 v, w;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = (T)x[ct][4 * qd + e];
        if (LOPLANE > 0) w[e] = (T)(x[ct][4 * qd + e] - (float)v[e]);
      }
      *reinterpret_cast<T4*>(map + p * PITCH + (ct * 32 + 8 * qd + 4 * h) * 2) = v;
      if (LOPLANE > 0) *reinterpret_cast<T4*>(map + LOPLANE + p * PITCH + (ct * 32 + 8 * qd + 4 * h) * 2) = w;
    }
  }
}
template <typename T, int LOPLANE = 0, int CT>
__device__ __forceinline__ void regs_to_map(const f32x16 (&x)[CT], unsigned char* map, int p, int h) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) regs_to_map_ct<T, LOPLANE>(x, map, p, h, ct);
}
