// The matrix pipe's operand types and products (gfx950), once for every kernel file: Mfma<T> maps an operand type to its
// fragment types and MFMA builtins.  A kernel's own trait keeps only what is its own (layouts, tile constants) and takes
// the product from here; the split (f16x2_t) and fp8 traits call the builtins directly.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(1))) const void* gptr_t;   // the operands of the LDS-DMA builtin
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;   // ds_read_b64_tr_b16's operand

// m16: 16x16x32, m32: 32x32x16 (frag operands); m4: 4x4x4 (frag4 operands)
template <typename T> struct Mfma;
template <> struct Mfma<bf16_t> {
  using frag = bf16x8;
  using frag4 = s16x4;
  static __device__ __forceinline__ f32x4 m16(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x16 m32(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  // 16 independent 4x4x4 products (one per channel): lane = (block, row of A / column of B and D)
  static __device__ __forceinline__ f32x4 m4(frag4 a, frag4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(a, b, c, 0, 0, 0);
  }
};
template <> struct Mfma<f16_t> {
  using frag = f16x8;
  using frag4 = f16x4v;
  static __device__ __forceinline__ f32x4 m16(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x16 m32(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4 m4(frag4 a, frag4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_4x4x4f16(a, b, c, 0, 0, 0);
  }
};
// fp32 operands: one float per lane, the 16x16x4 product
template <> struct Mfma<float> {
  using frag = float;
  static __device__ __forceinline__ f32x4 m16(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
};

// The same products on raw 16-bit lanes, for kernels whose operands come out of ds_read_b64_tr_b16 (s16x4 pieces) or
// are assembled as bits
template <typename T> struct MfmaRaw {
  using frag = typename Mfma<T>::frag;
  using frag4 = typename Mfma<T>::frag4;
  static __device__ __forceinline__ f32x4 m16(s16x8 a, s16x8 b, f32x4 c) {
    return Mfma<T>::m16(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), c);
  }
  static __device__ __forceinline__ f32x16 m32(s16x8 a, s16x8 b, f32x16 c) {
    return Mfma<T>::m32(__builtin_bit_cast(frag, a), __builtin_bit_cast(frag, b), c);
  }
  static __device__ __forceinline__ f32x4 m4(s16x4 a, s16x4 b, f32x4 c) {
    return Mfma<T>::m4(__builtin_bit_cast(frag4, a), __builtin_bit_cast(frag4, b), c);
  }
};
// one such lane as a float
template <typename T> __device__ __forceinline__ float bits_to_f32(unsigned short v) {
  return (float)__builtin_bit_cast(T, v);
}

// 32x32x16 operand read transposed from a [reduction row][column] LDS tile of 16-bit values (pitchb bytes per row): the
// lane's 8 reduction-consecutive elements (rows r0 + 8h .. +7) of column c0 + (lane & 31)
__device__ __forceinline__ s16x8 tr_frag(const unsigned char* tile, int pitchb, int r0, int c0, int lane) {
  const int h = lane >> 5, g1 = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3;
  const unsigned char* a = tile + (r0 + 8 * h + q) * pitchb + (c0 + 16 * g1 + 4 * p) * 2;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(a));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(a + 4 * pitchb));
  return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
