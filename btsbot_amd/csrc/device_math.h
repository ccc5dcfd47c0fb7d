// The __device__ helpers every kernel file shares (gfx950): split operands, the GELU / SiLU family, lane reductions and
// broadcasts, det_add, apply_act.  Part of common.h, which includes it behind the types
// (include common.h, not this file).
#pragma once

// split operands: 8 / 4 values as f16 head + f16 remainder (the remainder of a value below ~2^-13 is an f16
// subnormal: the matrix pipe takes subnormal f16 operands as they are, kernels are built with the default
// denormal mode)
struct h2x8 { f16x8 hi, lo; };
struct h2x4 { f16x4v hi, lo; };
__device__ __forceinline__ void split_f16(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)(v - (float)hi);
}
__device__ __forceinline__ h2x8 split8(const float (&v)[8]) {
  h2x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    _Float16 a, b;
    split_f16(v[j], a, b);
    o.hi[j] = a;
    o.lo[j] = b;
  }
  return o;
}
// Gradient operands of the split training products (btsbot_set_option "train_split") are small -- the BCE mean's 1/B and
// the backbone shrink them -- and split naively their heads would be f16 subnormals.  They enter the products scaled by
// 2^e, one e per tensor, chosen from the tensor's largest magnitude (the bits of a non-negative float, collected with
// atomicMax by the kernel that writes the tensor) so that it lands in [2^14, 2^15); an all-zero tensor (or none) keeps
// e = 0.  Both scalings are powers of two: applying and undoing them is exact.
// A tensor's record is AMAX_WORDS words: AMAX_SUB running maxima on separate cache lines, so that the waves of a large
// launch do not all queue at one address (one line: a copy of stage 0's dy took 4x as long as without the record).
constexpr int AMAX_SUB = 16, AMAX_STRIDE = 32, AMAX_WORDS = AMAX_SUB * AMAX_STRIDE;
__device__ __forceinline__ int split_exp(const unsigned* amax) {
  if (amax == nullptr) return 0;
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < AMAX_SUB; ++i) m = max(m, amax[i * AMAX_STRIDE]);
  const float a = __uint_as_float(m);
  if (!(a > 0.f) || !(a <= 3.0e38f)) return 0;
  int ex;
  (void)frexpf(a, &ex);   // a in [2^(ex-1), 2^ex)
  const int e = 15 - ex;
  return e < -100 ? -100 : e > 100 ? 100 : e;
}
// 64-lane max of a non-negative float's bits, then one vector atomic per wave (every lane of the wave must call it)
__device__ __forceinline__ void wave_amax(unsigned* amax, float v) {
  unsigned b = __float_as_uint(fabsf(v));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned t = (unsigned)__shfl_xor((int)b, o);
    b = t > b ? t : b;
  }
  if ((threadIdx.x & 63) == 0 && b != 0u) atomicMax(amax + (blockIdx.x % AMAX_SUB) * AMAX_STRIDE, b);
}
__device__ __forceinline__ h2x4 split4(const float (&v)[4]) {
  h2x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    _Float16 a, b;
    split_f16(v[j], a, b);
    o.hi[j] = a;
    o.lo[j] = b;
  }
  return o;
}

// ---------------------------------------------------------------------------------------
// device math
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf(float x) {
  // nn.GELU() default (exact erf form), architectures.py:35,149
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

// GELU for the 16-bit MFMA modes, one transcendental instead of erff's ~40 instructions:
//     gelu(x) = x Phi(x) = max(x, 0) - |x| Phi(-|x|),      Phi(-a) = 2^q(a)  for a >= 0,
// q = minimax polynomial of log2 Phi(-a) fitted so that |a 2^q(a) - a Phi(-a)| is smallest (tools/fit_gelu.py).
// The leading coefficients are negative, so q -> -inf and the tail is exactly 0 for any |x|: no clamp.
//   DEG 3: max |error| 5.8e-5 (below half an ulp of bf16 for |gelu| > 0.015), 3 fma + v_exp + v_max + fma;
//   DEG 5: max |error| 4.7e-7 (f32-class), 2 more fma.
// On gfx950 a v_exp_f32 issues in ~8 cycles, a plain VALU op in ~3: 24 / 30 cycles per wave-GELU against 42
// for the x * sigmoid(quintic) form this replaces (v_exp + v_rcp + v_med3 + 6).  The fp32 parity mode keeps gelu_erf.
template <int DEG> __device__ __forceinline__ float gelu_q(float a);
template <> __device__ __forceinline__ float gelu_q<3>(float a) {
  float t = fmaf(a, -0.024772998623334343f, -0.49926576060257244f);
  t = fmaf(a, t, -1.1287482669759885f);
  return fmaf(a, t, -1.0036805164077327f);
}
template <> __device__ __forceinline__ float gelu_q<5>(float a) {
  float t = fmaf(a, -0.0004726569791655389f, 0.007079169600613161f);
  t = fmaf(a, t, -0.05181158088529847f);
  t = fmaf(a, t, -0.46001256950698816f);
  t = fmaf(a, t, -1.1507770495088248f);
  return fmaf(a, t, -1.000039487932206f);
}
// max(x, 0) as ONE instruction: v_max_i32 on the bits (a positive float is a positive integer, anything with the
// sign bit set is negative).  fmaxf costs two (hipcc canonicalises the operand first for its NaN rule), and an
// inline-asm v_max_f32 is invisible to the compiler's hazard recogniser: scheduled right behind the MFMA that
// produces x it read the register before the matrix pipe had written it (stage2p.hip, first cut).
__device__ __forceinline__ float relu_f(float x) {
  const int b = __float_as_int(x);
  return __int_as_float(b > 0 ? b : 0);
}
template <int DEG> __device__ __forceinline__ float gelu_poly(float x) {
  const float a = __builtin_fabsf(x);
  const float e = __builtin_amdgcn_exp2f(gelu_q<DEG>(a));
  return fmaf(-a, e, relu_f(x));
}
// gelu_poly<3> of eight values on packed f16, for hidden activations that go to the matrix pipe as an f16 operand
// (stage0b.hip's bf16 inference form; tools/unit/mlp_occ.hip): value 2 i and 2 i + 1 are rounded to f16 as a pair
// (v_cvt_pkrtz: towards zero, so a finite input never becomes inf), |x| is a mask, q(a) runs on three v_pk_fma_f16 with
// the degree-3 coefficients rounded to f16, 2^q is one v_exp_f16 per half, and max(x, 0) - a E is v_pk_max_f16 + one
// v_pk_fma_f16: 11 instructions per pair, the result IS the operand dword.  Against the erf GELU: max 3.9e-3 / rms
// 1.2e-3 over |x| <= 8 (tests/test_gpu_stage0_gelu.py), a quarter of gelu_poly<3> rounded to bf16.  Past |x| ~ 9 q
// overflows to -inf and E = 0: the result is max(x, 0), at most 65504.
// The four pairs advance together, one step at a time (sched_barrier: hipcc otherwise runs each pair's chain of eight
// dependent instructions to its end, with an s_nop for the hazard between most of them, to save three registers).
__device__ __forceinline__ void gelu_pk4(const float (&x)[8], f16x2v (&g)[4]) {
  const f16x2v c3 = {(_Float16)-0.024772998623334343f, (_Float16)-0.024772998623334343f};
  const f16x2v c2 = {(_Float16)-0.49926576060257244f, (_Float16)-0.49926576060257244f};
  const f16x2v c1 = {(_Float16)-1.1287482669759885f, (_Float16)-1.1287482669759885f};
  const f16x2v c0 = {(_Float16)-1.0036805164077327f, (_Float16)-1.0036805164077327f};
  const f16x2v z = {(_Float16)0.f, (_Float16)0.f};
  f16x2v xh[4], a[4], t[4];
  unsigned e[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) xh[i] = __builtin_bit_cast(f16x2v, __builtin_amdgcn_cvt_pkrtz(x[2 * i], x[2 * i + 1]));
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = __builtin_bit_cast(f16x2v, __builtin_bit_cast(unsigned, xh[i]) & 0x7fff7fffu);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = __builtin_elementwise_fma(a[i], c3, c2);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = __builtin_elementwise_fma(a[i], t[i], c1);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = __builtin_elementwise_fma(a[i], t[i], c0);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) xh[i] = __builtin_elementwise_max(xh[i], z);
  __builtin_amdgcn_sched_barrier(0);
  // 2^q per half, the second one written into the high half in place: from __builtin_elementwise_exp2 hipcc makes
  // v_exp_f16 + v_exp_f16_sdwa + v_pack_b32_f16, a slot more per pair.  The compiler's hazard recogniser does not look
  // inside inline asm: gfx950 wants a wait state between a transcendental or a dst_sel write and a VALU read of the
  // result.  Three other instructions stand between the two writes of a register (volatile: kept in this order), and
  // the s_nop stands in front of whichever product hipcc places first.
#pragma unroll
  for (int i = 0; i < 4; ++i) asm volatile("v_exp_f16_e32 %0, %1" : "=&v"(e[i]) : "v"(__builtin_bit_cast(unsigned, t[i])));
#pragma unroll
  for (int i = 0; i < 4; ++i)
    asm volatile("v_exp_f16_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1"
                 : "+v"(e[i]) : "v"(__builtin_bit_cast(unsigned, t[i])));
  asm volatile("s_nop 0");
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) g[i] = __builtin_elementwise_fma(-a[i], __builtin_bit_cast(f16x2v, e[i]), xh[i]);
}
// d/dx of gelu_poly: with E = 2^q(a), D = E (1 + a ln2 q'(a)):  x > 0: 1 - D,  x < 0: D  (x = 0: 1/2 either way
// up to the fit error).  The 16-bit training forward applies gelu_poly, so its backward differentiates gelu_poly.
template <int DEG> __device__ __forceinline__ float gelu_dq(float a);
template <> __device__ __forceinline__ float gelu_dq<3>(float a) {
  float t = fmaf(a, 3.0f * -0.024772998623334343f, 2.0f * -0.49926576060257244f);
  return fmaf(a, t, -1.1287482669759885f);
}
template <> __device__ __forceinline__ float gelu_dq<5>(float a) {
  float t = fmaf(a, 5.0f * -0.0004726569791655389f, 4.0f * 0.007079169600613161f);
  t = fmaf(a, t, 3.0f * -0.05181158088529847f);
  t = fmaf(a, t, 2.0f * -0.46001256950698816f);
  return fmaf(a, t, -1.1507770495088248f);
}
template <int DEG> __device__ __forceinline__ float gelu_poly_grad(float x) {
  const float a = __builtin_fabsf(x);
  const float e = __builtin_amdgcn_exp2f(gelu_q<DEG>(a));
  const float d = e * fmaf(a * 0.6931471805599453f, gelu_dq<DEG>(a), 1.0f);
  return x > 0.0f ? 1.0f - d : d;
}
template <typename T> struct GeluDeg { static constexpr int value = 5; };     // f16 operands: f32-class GELU
template <> struct GeluDeg<bf16_t> { static constexpr int value = 3; };       // bf16 operands
template <typename T> __device__ __forceinline__ float gelu_for(float x) { return gelu_poly<GeluDeg<T>::value>(x); }
template <> __device__ __forceinline__ float gelu_for<float>(float x) { return gelu_erf(x); }

// d/dx of the exact erf GELU: Phi(x) + x * phi(x)
__device__ __forceinline__ float gelu_grad(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }
// SiLU for the 16-bit modes: v_exp + v_rcp instead of the IEEE division sequence (relative error ~1e-6,
// far below half an ulp of f16 / bf16); the fp32 parity mode keeps silu_f
__device__ __forceinline__ float silu_fast(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
template <typename T> __device__ __forceinline__ float silu_for(float x) { return silu_fast(x); }
template <> __device__ __forceinline__ float silu_for<float>(float x) { return silu_f(x); }

template <typename T> __device__ __forceinline__ float gelu_grad_for(float x) {
  return gelu_poly_grad<GeluDeg<T>::value>(x);
}
template <> __device__ __forceinline__ float gelu_grad_for<float>(float x) { return gelu_grad(x); }

template <typename T> __device__ __forceinline__ float to_f32(T x) { return (float)x; }

// Sum within aligned groups of 16 lanes (a DPP "row"); every lane ends with its row's total.
// quad_perm xor 1, xor 2, then row_half_mirror / row_mirror (the quads / halves are uniform by then):
// four v_add_f32_dpp, no LDS crossbar (ds_bpermute) round trips.
__device__ __forceinline__ float group16_sum(float v) {
#define BTS_DPP_ADD(ctrl)                                                                      \
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, \
                                                             0xF, 0xF, true))
  BTS_DPP_ADD(0xB1);    // quad_perm [1,0,3,2]
  BTS_DPP_ADD(0x4E);    // quad_perm [2,3,0,1]
  BTS_DPP_ADD(0x141);   // row_half_mirror
  BTS_DPP_ADD(0x140);   // row_mirror
#undef BTS_DPP_ADD
  return v;
}

// 64-lane sum; every lane ends with the total.  Rows meet through v_permlane16_swap /
// v_permlane32_swap (gfx950): swap(v, v) hands every lane its own and its partner row's value.
__device__ __forceinline__ float wave_sum(float v) {
  v = group16_sum(v);
  // (inline asm: given the same value for both operands of __builtin_amdgcn_permlane16_swap,
  //  hipcc 7.2 folds its two results into one and adds a register to itself; s_nop covers the
  //  VALU-write -> permlane-read hazard the compiler would otherwise pad)
  float w = v;
  asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(v), "+v"(w));
  v += w;
  w = v;
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(v), "+v"(w));
  return v + w;
}

// the halves / the 16-lane rows of two values meet in one swap (gfx950)
__device__ __forceinline__ float swap_add32(float a, float b) {
  // a' = {a.lo, b.lo}, b' = {a.hi, b.hi}; a'+b': lanes 0-31 total of a, lanes 32-63 total of b
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float swap_add16(float a, float b) {
  // odd 16-lane rows of a swap with even rows of b; a'+b': even rows total of a, odd rows of b
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__device__ __forceinline__ double lane_bcast(double v, int k) {   // k wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}

// ---------------------------------------------------------------------------------------
// Deterministic batch reductions (btsbot_set_option(h, "deterministic", 1) / BTSBOT_AMD_DETERMINISTIC=1): the kernels of
// the ConvNeXt training step that meet across workgroups through fp32 atomics -- LayerNorm / depthwise parameter
// gradients, column sums, the fc1-bias gradient of the fused MLP backward -- write one partial row per workgroup instead
// (`part`, from the scratch of the running btsbot_backward() call) and launch_det_reduce() adds the rows in a fixed order
// behind them on the same stream: two identical backward passes then agree bit for bit.  part == nullptr: atomics.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void det_add(float* out, float v, float* part, size_t slot) {
  if (part != nullptr) part[slot] = v;
  else atomicAdd(out, v);
}

__device__ __forceinline__ float apply_act(float x, int act) {
  if (act == ACT_GELU) return gelu_erf(x);
  if (act == ACT_RELU) return x > 0.f ? x : 0.f;
  return x;
}
