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
// LayerNorm over the 32 CT channels of this lane's pixel (x[CT][16] here + the partner lane ^ 32)
template <int CT>
__device__ __forceinline__ void ln_regs(const f32x16 (&x)[CT], const float* __restrict__ w,
                                        const float* __restrict__ b, int h, f32x16 (&y)[CT]) {
  constexpr int C = StageRegs<CT>::C;
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
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int c = ct * 32 + 8 * qd + 4 * h;
      const float4 wv = *reinterpret_cast<const float4*>(w + c);
      const float4 bv = *reinterpret_cast<const float4*>(b + c);
      y[ct][4 * qd + 0] = (x[ct][4 * qd + 0] - mean) * rstd * wv.x + bv.x;
      y[ct][4 * qd + 1] = (x[ct][4 * qd + 1] - mean) * rstd * wv.y + bv.y;
      y[ct][4 * qd + 2] = (x[ct][4 * qd + 2] - mean) * rstd * wv.z + bv.z;
      y[ct][4 * qd + 3] = (x[ct][4 * qd + 3] - mean) * rstd * wv.w + bv.w;
    }
}

// LOPLANE > 0: also the values' f16 remainders, LOPLANE bytes behind (split mode)
template <typename T, int LOPLANE = 0, int CT>
__device__ __forceinline__ void regs_to_map(const f32x16 (&x)[CT], unsigned char* map, int p, int h) {
  constexpr int PITCH = StageRegs<CT>::PITCH;
  typedef T T4 __attribute__((ext_vector_type(4)));
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
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
