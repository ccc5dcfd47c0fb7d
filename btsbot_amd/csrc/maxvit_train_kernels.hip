// The kernels of the MaxViT training engine (maxvit_train.hip) and their launchers: what has no GEMM shape there --
// BatchNorm2d batch statistics, apply and backward; depthwise 3x3 forward, input and filter gradient; the squeeze-excite
// small dense layers; the attention backward inside a 49-token partition; col2im and the gradient unpackers.  Everything
// is fp32 on NHWC rows [B*H*H][C].  The launchers (prototypes in maxvit.h) are what the engine and the op-level entry
// points of maxvit_train_ops.hip both run.
#include "maxvit.h"

namespace {

constexpr float BN_EPS = 1e-5f, BN_MOM = 0.1f;

inline unsigned nblk(long n, int per = 256) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float silu_grad(float x) {
  const float s = sigmoid_f(x);
  return s * (1.0f + x * (1.0f - s));
}

// The reductions below share one thread layout: a workgroup owns 64 channels, lane q = threadIdx.x & 15 four of them (one
// 16-byte load), row lane rl = threadIdx.x >> 4 every 16th row of its share, four rows in flight per trip (one 4-byte
// load per lane and trip left these kernels at 1.5-1.8 TB/s).
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4_mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 f4_fma(float4 a, float4 b, float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
// sums over the 16 row lanes of a workgroup, then one atomic per channel: dst[c] += total (n4 accumulators of 4 channels)
template <int N>
__device__ __forceinline__ void quad_reduce_atomic(const float4 (&acc)[N], float* const (&dst)[N], int c0, int C, float* sh) {
  const int q = threadIdx.x & 15, rl = threadIdx.x >> 4;
#pragma unroll
  for (int t = 0; t < N; ++t) {
    __syncthreads();
    *reinterpret_cast<float4*>(sh + (rl * 16 + q) * 4) = acc[t];
    __syncthreads();
    if (threadIdx.x < 64 && c0 + (int)threadIdx.x < C) {
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) a += sh[r * 64 + threadIdx.x];
      atomicAdd(dst[t] + c0 + threadIdx.x, a);
    }
  }
}
// ---- per-channel sums over the rows of x [M][C]: sums[c] += sum (x - shift[c]), sums[C + c] += sum (x - shift[c])^2
__global__ __launch_bounds__(256) void col_moments_kernel(const float* __restrict__ x, const float* __restrict__ shift,
                                                          float* __restrict__ sums, long M, int C) {
  __shared__ float sh[16 * 64];
  const int q = threadIdx.x & 15, rl = threadIdx.x >> 4, c0 = blockIdx.x * 64, c = c0 + 4 * q;
  float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  if (c < C) {
    const float4 sf = shift != nullptr ? *reinterpret_cast<const float4*>(shift + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const long step = (long)gridDim.y * 16;
    for (long r = (long)blockIdx.y * 16 + rl; r < M; r += 4 * step) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(x + min(r + u * step, M - 1) * C + c);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (r + u * step < M) {
          const float4 d = f4_sub(v[u], sf);
          acc[0] = f4_add(acc[0], d);
          acc[1] = f4_fma(d, d, acc[1]);
        }
    }
  }
  float* const dst[2] = {sums, sums + C};
  quad_reduce_atomic<2>(acc, dst, c0, C, sh);
}
// pass 1 -> mean;  pass 2 (sums taken about the mean) -> rstd, and the running statistics in the master arena
__global__ void bn_mean_kernel(const float* sums, float* stat, long M, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C) stat[c] = sums[c] / (float)M;
}
__global__ void bn_finish_kernel(const float* sums, float* stat, float* run_mean, float* run_var, long M, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float mean = stat[c] + sums[c] / (float)M;    // (the centred sum is ~0: it only polishes the mean)
  const float d = sums[c] / (float)M;
  const float var = fmaxf(sums[C + c] / (float)M - d * d, 0.f);
  stat[c] = mean;
  stat[C + c] = rsqrtf(var + BN_EPS);
  if (run_mean != nullptr) {   // torch: momentum 0.1, the running variance takes the unbiased estimate
    run_mean[c] = (1.0f - BN_MOM) * run_mean[c] + BN_MOM * mean;
    run_var[c] = (1.0f - BN_MOM) * run_var[c] + BN_MOM * var * ((float)M / (float)(M > 1 ? M - 1 : 1));
  }
}
// y = act(xhat * w + b), xhat = (x - mean) * rstd;  act 0: none, 1: SiLU.  n4 = M * C / 4 (four channels per thread)
__global__ void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ stat, const float* __restrict__ w,
                                const float* __restrict__ b, float* __restrict__ y, long n4, int C, int act) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int c = (int)((i * 4) % C);
  const float4 v = reinterpret_cast<const float4*>(x)[i];
  const float4 mean = *reinterpret_cast<const float4*>(stat + c), rstd = *reinterpret_cast<const float4*>(stat + C + c);
  const float4 z = f4_fma(f4_mul(f4_sub(v, mean), rstd), *reinterpret_cast<const float4*>(w + c),
                          *reinterpret_cast<const float4*>(b + c));
  reinterpret_cast<float4*>(y)[i] =
      act ? make_float4(z.x * sigmoid_f(z.x), z.y * sigmoid_f(z.y), z.z * sigmoid_f(z.z), z.w * sigmoid_f(z.w)) : z;
}
// backward sums: sums[c] += sum dz, sums[C + c] += sum dz * xhat, dz = dy * act'(z)
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          const float* __restrict__ stat, const float* __restrict__ w,
                                                          const float* __restrict__ b, float* __restrict__ sums, long M,
                                                          int C, int act) {
  __shared__ float sh[16 * 64];
  const int q = threadIdx.x & 15, rl = threadIdx.x >> 4, c0 = blockIdx.x * 64, c = c0 + 4 * q;
  float4 acc[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  if (c < C) {
    const float4 mean = *reinterpret_cast<const float4*>(stat + c), rstd = *reinterpret_cast<const float4*>(stat + C + c);
    const float4 wc = *reinterpret_cast<const float4*>(w + c), bc = *reinterpret_cast<const float4*>(b + c);
    const long step = (long)gridDim.y * 16;
    for (long r = (long)blockIdx.y * 16 + rl; r < M; r += 2 * step) {
      float4 xv[2], dv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const long rr = min(r + u * step, M - 1);
        xv[u] = *reinterpret_cast<const float4*>(x + rr * C + c);
        dv[u] = *reinterpret_cast<const float4*>(dy + rr * C + c);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (r + u * step < M) {
          const float4 xh = f4_mul(f4_sub(xv[u], mean), rstd);
          float4 dz = dv[u];
          if (act) {
            const float4 z = f4_fma(xh, wc, bc);
            dz = f4_mul(dz, make_float4(silu_grad(z.x), silu_grad(z.y), silu_grad(z.z), silu_grad(z.w)));
          }
          acc[0] = f4_add(acc[0], dz);
          acc[1] = f4_fma(dz, xh, acc[1]);
        }
    }
  }
  float* const dst[2] = {sums, sums + C};
  quad_reduce_atomic<2>(acc, dst, c0, C, sh);
}
// dx (+)= w rstd (dz - sum dz / M - xhat sum(dz xhat) / M);  block 0 also adds the parameter gradients.  Four channels per thread
__global__ void bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ stat,
                                    const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ sums,
                                    float* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db, long M, int C,
                                    int act, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += 256) {
      atomicAdd(dw + c, sums[C + c]);
      atomicAdd(db + c, sums[c]);
    }
  }
  if (i >= M * C / 4) return;
  const int c = (int)((i * 4) % C);
  const float4 rstd = *reinterpret_cast<const float4*>(stat + C + c);
  const float4 xh = f4_mul(f4_sub(reinterpret_cast<const float4*>(x)[i], *reinterpret_cast<const float4*>(stat + c)), rstd);
  const float4 wc = *reinterpret_cast<const float4*>(w + c);
  float4 dz = reinterpret_cast<const float4*>(dy)[i];
  if (act) {
    const float4 z = f4_fma(xh, wc, *reinterpret_cast<const float4*>(b + c));
    dz = f4_mul(dz, make_float4(silu_grad(z.x), silu_grad(z.y), silu_grad(z.z), silu_grad(z.w)));
  }
  const float inv = 1.0f / (float)M;
  const float4 s0 = *reinterpret_cast<const float4*>(sums + c), s1 = *reinterpret_cast<const float4*>(sums + C + c);
  float4 g;
  g.x = wc.x * rstd.x * (dz.x - s0.x * inv - xh.x * s1.x * inv);
  g.y = wc.y * rstd.y * (dz.y - s0.y * inv - xh.y * s1.y * inv);
  g.z = wc.z * rstd.z * (dz.z - s0.z * inv - xh.z * s1.z * inv);
  g.w = wc.w * rstd.w * (dz.w - s0.w * inv - xh.w * s1.w * inv);
  float4* o = reinterpret_cast<float4*>(dx) + i;
  *o = accumulate ? f4_add(*o, g) : g;
}

// ---- depthwise 3x3, padding 1, stride s: in [B][H][H][C] -> out [B][Ho][Ho][C]; taps w9 [9][C].  A thread owns four
// channels of a pixel; its nine taps are requested as one batch (addresses clamped into the map, values zeroed by a
// select: a load under a bounds branch is waited for on the spot)
__global__ void dw3_fwd_kernel(const float* __restrict__ in, const float* __restrict__ w9, const float* __restrict__ bias,
                               float* __restrict__ out, int B, int H, int C, int s) {
  const int Ho = H / s, C4 = C / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * Ho * Ho * C4) return;
  const int c = (int)(i % C4) * 4;
  long p = i / C4;
  const int ox = (int)(p % Ho);
  p /= Ho;
  const int oy = (int)(p % Ho), b = (int)(p / Ho);
  float4 v[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int iy = min(max(oy * s + t / 3 - 1, 0), H - 1), ix = min(max(ox * s + t % 3 - 1, 0), H - 1);
    v[t] = *reinterpret_cast<const float4*>(in + (((long)b * H + iy) * H + ix) * C + c);
  }
  float4 a = *reinterpret_cast<const float4*>(bias + c);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    asm volatile("" : "+v"(v[t].x), "+v"(v[t].y), "+v"(v[t].z), "+v"(v[t].w));   // (keeps the load unconditional)
    const int iy = oy * s + t / 3 - 1, ix = ox * s + t % 3 - 1;
    if (!(iy >= 0 && iy < H && ix >= 0 && ix < H)) v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    a = f4_fma(*reinterpret_cast<const float4*>(w9 + t * C + c), v[t], a);
  }
  reinterpret_cast<float4*>(out)[i] = a;
}
__global__ void dw3_bwd_in_kernel(const float* __restrict__ dout, const float* __restrict__ w9, float* __restrict__ din,
                                  int B, int H, int C, int s) {
  const int Ho = H / s, C4 = C / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * H * H * C4) return;
  const int c = (int)(i % C4) * 4;
  long p = i / C4;
  const int ix = (int)(p % H);
  p /= H;
  const int iy = (int)(p % H), b = (int)(p / H);
  float4 v[9];
  bool ok[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int ty = iy + 1 - t / 3, tx = ix + 1 - t % 3;
    ok[t] = ty >= 0 && ty % s == 0 && ty / s < Ho && tx >= 0 && tx % s == 0 && tx / s < Ho;
    const int oy = min(max(ty, 0) / s, Ho - 1), ox = min(max(tx, 0) / s, Ho - 1);
    v[t] = *reinterpret_cast<const float4*>(dout + (((long)b * Ho + oy) * Ho + ox) * C + c);
  }
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    asm volatile("" : "+v"(v[t].x), "+v"(v[t].y), "+v"(v[t].z), "+v"(v[t].w));
    if (!ok[t]) v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    a = f4_fma(*reinterpret_cast<const float4*>(w9 + t * C + c), v[t], a);
  }
  reinterpret_cast<float4*>(din)[i] = a;
}
// dw9[t][c] += sum dout * in(shifted by tap t), dbias[c] += sum dout   (the reductions' thread layout; a pixel's nine taps in
// one batch)
__global__ __launch_bounds__(256) void dw3_bwd_w_kernel(const float* __restrict__ in, const float* __restrict__ dout,
                                                        float* __restrict__ dw9, float* __restrict__ dbias, int B, int H,
                                                        int C, int s) {
  __shared__ float sh[16 * 64];
  const int Ho = H / s;
  const int q = threadIdx.x & 15, rl = threadIdx.x >> 4, c0 = blockIdx.x * 64, c = c0 + 4 * q;
  float4 acc[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < C) {
    const long npix = (long)B * Ho * Ho;
    for (long p = (long)blockIdx.y * 16 + rl; p < npix; p += (long)gridDim.y * 16) {
      const int ox = (int)(p % Ho), oy = (int)((p / Ho) % Ho), b = (int)(p / ((long)Ho * Ho));
      const float4 d = *reinterpret_cast<const float4*>(dout + p * C + c);
      float4 v[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int iy = min(max(oy * s + t / 3 - 1, 0), H - 1), ix = min(max(ox * s + t % 3 - 1, 0), H - 1);
        v[t] = *reinterpret_cast<const float4*>(in + (((long)b * H + iy) * H + ix) * C + c);
      }
      acc[9] = f4_add(acc[9], d);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        asm volatile("" : "+v"(v[t].x), "+v"(v[t].y), "+v"(v[t].z), "+v"(v[t].w));
        const int iy = oy * s + t / 3 - 1, ix = ox * s + t % 3 - 1;
        if (!(iy >= 0 && iy < H && ix >= 0 && ix < H)) v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        acc[t] = f4_fma(d, v[t], acc[t]);
      }
    }
  }
  float* dst[10];
#pragma unroll
  for (int t = 0; t < 9; ++t) dst[t] = dw9 + t * C;
  dst[9] = dbias;
  float* const (&dref)[10] = reinterpret_cast<float* const (&)[10]>(dst);
  quad_reduce_atomic<10>(acc, dref, c0, C, sh);
}

// ---- per-alert column sums: out[b][c] = scale * sum_p a[b][p][c] * (m ? m[b][p][c] : 1)   (the reductions' thread layout)
__global__ __launch_bounds__(256) void alert_colsum_kernel(const float* __restrict__ a, const float* __restrict__ m,
                                                           float* __restrict__ out, int P, int C, float scale) {
  __shared__ float sh[16 * 64];
  const int q = threadIdx.x & 15, rl = threadIdx.x >> 4, c0 = blockIdx.x * 64, c = c0 + 4 * q, b = blockIdx.y;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < C)
    for (int p = rl; p < P; p += 64) {
      float4 av[4], mv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long i = ((long)b * P + min(p + 16 * u, P - 1)) * C + c;
        av[u] = *reinterpret_cast<const float4*>(a + i);
        mv[u] = m != nullptr ? *reinterpret_cast<const float4*>(m + i) : make_float4(1.f, 1.f, 1.f, 1.f);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (p + 16 * u < P) s = f4_fma(av[u], mv[u], s);
    }
  *reinterpret_cast<float4*>(sh + (rl * 16 + q) * 4) = s;
  __syncthreads();
  if (threadIdx.x < 64 && c0 + (int)threadIdx.x < C) {
    float t = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += sh[r * 64 + threadIdx.x];
    out[(long)b * C + c0 + threadIdx.x] = scale * t;
  }
}
// small dense layers over the batch (squeeze-excite: B rows): y[b][o] = act(bias[o] + sum_i x[b][i] w[o][i]); act 0 none,
// 1 SiLU, 2 sigmoid; pre (optional) keeps the pre-activation
__global__ void lin_fwd_small_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                     float* __restrict__ pre, float* __restrict__ y, int B, int I, int O, int act) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * O) return;
  const int o = i % O, b = i / O;
  // (four chains: one chain over up to 2048 inputs was 58 us of exposed load + FMA latency on a 64-row batch)
  float a0 = bias[o], a1 = 0.f, a2 = 0.f, a3 = 0.f;
  const float* xp = x + (long)b * I;
  const float* wp = w + (long)o * I;
  int k = 0;
#pragma unroll 2
  for (; k + 3 < I; k += 4) {
    a0 = fmaf(xp[k], wp[k], a0);
    a1 = fmaf(xp[k + 1], wp[k + 1], a1);
    a2 = fmaf(xp[k + 2], wp[k + 2], a2);
    a3 = fmaf(xp[k + 3], wp[k + 3], a3);
  }
  for (; k < I; ++k) a0 = fmaf(xp[k], wp[k], a0);
  const float a = (a0 + a1) + (a2 + a3);
  if (pre != nullptr) pre[i] = a;
  y[i] = act == 1 ? a * sigmoid_f(a) : act == 2 ? sigmoid_f(a) : a;
}
// dpre[b][o] = dy[b][o] * act'(pre)   (act 1: SiLU from the pre-activation; 2: sigmoid from its OUTPUT in pre)
__global__ void act_bwd_small_kernel(const float* __restrict__ dy, const float* __restrict__ pre, float* __restrict__ dpre,
                                     int n, int act) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = pre[i];
  dpre[i] = dy[i] * (act == 1 ? silu_grad(v) : v * (1.0f - v));
}
__global__ void lin_bwd_in_small_kernel(const float* __restrict__ dpre, const float* __restrict__ w, float* __restrict__ dx,
                                        int B, int I, int O) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * I) return;
  const int k = i % I, b = i / I;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;   // four chains (as lin_fwd_small_kernel: 137 us with one)
  const float* dp = dpre + (long)b * O;
  const float* wp = w + k;
  int o = 0;
#pragma unroll 2
  for (; o + 3 < O; o += 4) {
    a0 = fmaf(dp[o], wp[(long)o * I], a0);
    a1 = fmaf(dp[o + 1], wp[(long)(o + 1) * I], a1);
    a2 = fmaf(dp[o + 2], wp[(long)(o + 2) * I], a2);
    a3 = fmaf(dp[o + 3], wp[(long)(o + 3) * I], a3);
  }
  for (; o < O; ++o) a0 = fmaf(dp[o], wp[(long)o * I], a0);
  dx[i] = (a0 + a1) + (a2 + a3);
}
__global__ void lin_bwd_w_small_kernel(const float* __restrict__ dpre, const float* __restrict__ x, float* __restrict__ dw,
                                       float* __restrict__ db, int B, int I, int O) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= O * I) return;
  const int k = i % I, o = i / I;
  float a = 0.f, s = 0.f;
  for (int b = 0; b < B; ++b) {
    const float d = dpre[(long)b * O + o];
    a = fmaf(d, x[(long)b * I + k], a);
    s += d;
  }
  dw[i] += a;
  if (k == 0) db[o] += s;
}
// y[b][p][c] = a[b][p][c] * g[b][c]  (four channels per thread; y may be a)
__global__ void gate_mul_kernel(const float* a, const float* __restrict__ g, float* y, int P, int C, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int c = (int)((i * 4) % C);
  const long b = (i * 4) / ((long)P * C);
  reinterpret_cast<float4*>(y)[i] = f4_mul(reinterpret_cast<const float4*>(a)[i], *reinterpret_cast<const float4*>(g + b * C + c));
}
// d[b][p][c] += v[b][c] * scale
__global__ void bcast_add_kernel(float* __restrict__ d, const float* __restrict__ v, int P, int C, long n, float scale) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  const long b = i / ((long)P * C);
  d[i] += v[b * C + c] * scale;
}
__global__ void bcast_set_kernel(float* __restrict__ d, const float* __restrict__ v, int P, int C, long n, float scale) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  const long b = i / ((long)P * C);
  d[i] = v[b * C + c] * scale;
}
// dx[b][y][x][c] (+)= 0.25 g[b][y / 2][x / 2][c]
__global__ void avgpool2_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, int B, int H, int C, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * H * H * C) return;
  const int c = (int)(i % C);
  long p = i / C;
  const int x = (int)(p % H);
  p /= H;
  const int y = (int)(p % H), b = (int)(p / H), Ho = H / 2;
  const float v = 0.25f * g[(((long)b * Ho + y / 2) * Ho + x / 2) * C + c];
  dx[i] = accumulate ? dx[i] + v : v;
}
// (elementwise kernels: four values per thread; every count here is a multiple of 4)
__global__ void add_kernel(float* __restrict__ a, const float* __restrict__ b, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) reinterpret_cast<float4*>(a)[i] = f4_add(reinterpret_cast<float4*>(a)[i], reinterpret_cast<const float4*>(b)[i]);
}
__global__ void gelu_fwd_kernel(const float* __restrict__ pre, float* __restrict__ out, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(pre)[i];
  reinterpret_cast<float4*>(out)[i] = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
}
__global__ void gelu_bwd_kernel(const float* __restrict__ pre, float* __restrict__ d, long n4) {   // d *= gelu'(pre)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(pre)[i];
  float4* o = reinterpret_cast<float4*>(d) + i;
  *o = f4_mul(*o, make_float4(gelu_grad(v.x), gelu_grad(v.y), gelu_grad(v.z), gelu_grad(v.w)));
}
// col2im of a 3x3 s1 p1 convolution: din[b][y][x][c] = sum over taps dcol[b][y - ky + 1][x - kx + 1][(ky*3+kx)*C + c]
__global__ void col2im3_kernel(const float* __restrict__ dcol, float* __restrict__ din, int B, int H, int C) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * H * H * C) return;
  const int c = (int)(i % C);
  long p = i / C;
  const int x = (int)(p % H);
  p /= H;
  const int y = (int)(p % H), b = (int)(p / H);
  float a = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int oy = y - ky + 1;
    if (oy < 0 || oy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ox = x - kx + 1;
      if (ox < 0 || ox >= H) continue;
      a += dcol[(((long)b * H + oy) * H + ox) * (9 * C) + (ky * 3 + kx) * C + c];
    }
  }
  din[i] = a;
}
// packed convolution gradient [O][(ky*3+kx)*C + c] (row pitch ldp) -> master layout [O][C][3][3], accumulated
__global__ void unpack_conv3_grad_kernel(const float* __restrict__ gp, float* __restrict__ g, int O, int C, int ldp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= O * C * 9) return;
  const int t = i % 9, c = (i / 9) % C, o = i / (9 * C);
  g[i] += gp[(long)o * ldp + t * C + c];
}
// tap-major depthwise gradient [9][C] -> master [C][1][3][3], accumulated
__global__ void unpack_dw_grad_kernel(const float* __restrict__ g9, float* __restrict__ g, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 9 * C) return;
  const int t = i % 9, c = i / 9;
  g[i] += g9[t * C + c];
}
// relative-position bias gradient [heads][49 key][49 query] -> table [169][heads], accumulated
__global__ void relbias_grad_kernel(const float* __restrict__ dbias, float* __restrict__ dtable, int heads) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // [169][heads]
  if (i >= 169 * heads) return;
  const int hd = i % heads, idx = i / heads;
  const int dy = idx / 13 - 6, dx = idx % 13 - 6;
  float s = 0.f;
  for (int kj = 0; kj < 49; ++kj) {
    const int qy = kj / 7 + dy, qx = kj % 7 + dx;
    if (qy < 0 || qy >= 7 || qx < 0 || qx >= 7) continue;
    s += dbias[((long)hd * 49 + kj) * 49 + qy * 7 + qx];
  }
  dtable[i] += s;
}

// ---- attention backward: one wave per (alert, partition, head); the forward's conventions (mv_attn_kernel,
// maxvit_ops.hip): q scaled by 32^-0.5, s[query][key j] = q . k_j + bias_t[head][j][query], softmax over the keys.
// Phase 1, lane = query t: P[t][:], dP[t][j] = dO_t . v_j, dS[t][j] = P (dP - sum_j P dP), dq_t = SC sum_j dS k_j,
// dbias[head][j][t] += dS.  Phase 2, lane = key j: dk_j = sum_t dS[t][j] (SC q_t), dv_j = sum_t P[t][j] dO_t.
// A workgroup walks `units` (alert, partition) pairs of ONE head and keeps the bias gradient of its lane's query in
// registers (49 values), added to the table once at the end: one atomic per (block, j, t) instead of one per (unit, j, t)
// -- 8192 units of stage 0 hammering the same 2401 addresses per head was most of this kernel.  The lane's own q and dO
// rows stay in registers; k, v (and q, dO for phase 2) are read from LDS as 16-byte broadcasts.
__global__ __launch_bounds__(64) void mv_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ bias_t,
                                                         const float* __restrict__ dout, float* __restrict__ dqkv,
                                                         float* __restrict__ dbias, int H, int C, int grid_mode, int units) {
  constexpr int RP = 36;               // row pitch in floats (16-byte aligned rows)
  __shared__ __attribute__((aligned(16))) float ks[49][RP];
  __shared__ __attribute__((aligned(16))) float vs[49][RP];
  __shared__ __attribute__((aligned(16))) float qs[49][RP];     // SC * q
  __shared__ __attribute__((aligned(16))) float dos[49][RP];
  __shared__ float ps[49][50];     // [query][key]
  __shared__ float dss[49][50];
  const int heads = C / 32, G = H / 7, nW = G * G;
  const int head = blockIdx.x % heads, ustep = gridDim.x / heads;
  const int t = threadIdx.x;
  const bool active = t < 49;
  const int ty = t / 7, tx = t % 7;
  constexpr float SC = 0.17677669529663687f;
  // (the products run as PACKED fp32 FMAs -- v_pk_fma_f32, two per instruction: this kernel is bound by the ~8 k FMA
  //  instructions a (partition, head) costs on one wave)
  typedef float f2 __attribute__((ext_vector_type(2)));
  float db[49];
#pragma unroll
  for (int j = 0; j < 49; ++j) db[j] = 0.f;
  for (int u = blockIdx.x / heads; u < units; u += ustep) {
    const int w = u % nW;
    const long b = u / nW;
    const int wy = w / G, wx = w % G;
    const int py = grid_mode ? ty * G + wy : wy * 7 + ty;
    const int px = grid_mode ? tx * G + wx : wx * 7 + tx;
    const long row = active ? (b * H + py) * H + px : 0;
    f2 qr[16], dor[16];            // this lane's SC * q row and dO row
    __syncthreads();               // the previous unit's phase 2 has read the images
    if (active) {
      const float4* base = reinterpret_cast<const float4*>(qkv + row * 3 * C + head * 96);
      const float4* dob = reinterpret_cast<const float4*>(dout + row * C + head * 32);
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const float4 q4 = base[d], o4 = dob[d];
        const float4 qs4 = make_float4(q4.x * SC, q4.y * SC, q4.z * SC, q4.w * SC);
        qr[2 * d] = f2{qs4.x, qs4.y};
        qr[2 * d + 1] = f2{qs4.z, qs4.w};
        dor[2 * d] = f2{o4.x, o4.y};
        dor[2 * d + 1] = f2{o4.z, o4.w};
        *reinterpret_cast<float4*>(&qs[t][4 * d]) = qs4;
        *reinterpret_cast<float4*>(&ks[t][4 * d]) = base[8 + d];
        *reinterpret_cast<float4*>(&vs[t][4 * d]) = base[16 + d];
        *reinterpret_cast<float4*>(&dos[t][4 * d]) = o4;
      }
    }
    __syncthreads();
    if (active) {
      const float* bt = bias_t + (size_t)head * 2401 + t;
      float mx = -3.0e38f;
      for (int j = 0; j < 49; ++j) {
        f2 a2 = f2{0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 16; ++d) a2 = qr[d] * *reinterpret_cast<const f2*>(&ks[j][2 * d]) + a2;
        const float a = a2.x + a2.y + bt[j * 49];
        ps[t][j] = a;
        mx = fmaxf(mx, a);
      }
      float sum = 0.f;
      for (int j = 0; j < 49; ++j) {
        const float e = __expf(ps[t][j] - mx);
        ps[t][j] = e;
        sum += e;
      }
      const float inv = 1.0f / sum;
      float dot = 0.f;
      for (int j = 0; j < 49; ++j) {
        f2 d2 = f2{0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 16; ++d) d2 = dor[d] * *reinterpret_cast<const f2*>(&vs[j][2 * d]) + d2;
        const float dp = d2.x + d2.y;
        const float p = ps[t][j] * inv;
        ps[t][j] = p;
        dss[t][j] = dp;
        dot = fmaf(p, dp, dot);
      }
      f2 dq[16];
#pragma unroll
      for (int d = 0; d < 16; ++d) dq[d] = f2{0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 49; ++j) {
        const float ds = ps[t][j] * (dss[t][j] - dot);
        dss[t][j] = ds;
        db[j] += ds;
        const f2 ds2 = f2{ds, ds};
#pragma unroll
        for (int d = 0; d < 16; ++d) dq[d] = ds2 * *reinterpret_cast<const f2*>(&ks[j][2 * d]) + dq[d];
      }
      float4* dst = reinterpret_cast<float4*>(dqkv + row * 3 * C + head * 96);
#pragma unroll
      for (int d = 0; d < 8; ++d)
        dst[d] = make_float4(dq[2 * d].x * SC, dq[2 * d].y * SC, dq[2 * d + 1].x * SC, dq[2 * d + 1].y * SC);
    }
    __syncthreads();
    if (active) {   // lane = key t
      f2 dk[16], dv[16];
#pragma unroll
      for (int d = 0; d < 16; ++d) dk[d] = dv[d] = f2{0.f, 0.f};
      for (int q = 0; q < 49; ++q) {
        const float ds = dss[q][t], p = ps[q][t];
        const f2 ds2 = f2{ds, ds}, p2 = f2{p, p};
#pragma unroll
        for (int d = 0; d < 16; ++d) {
          dk[d] = ds2 * *reinterpret_cast<const f2*>(&qs[q][2 * d]) + dk[d];
          dv[d] = p2 * *reinterpret_cast<const f2*>(&dos[q][2 * d]) + dv[d];
        }
      }
      float4* dst = reinterpret_cast<float4*>(dqkv + row * 3 * C + head * 96);
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        dst[8 + d] = make_float4(dk[2 * d].x, dk[2 * d].y, dk[2 * d + 1].x, dk[2 * d + 1].y);
        dst[16 + d] = make_float4(dv[2 * d].x, dv[2 * d].y, dv[2 * d + 1].x, dv[2 * d + 1].y);
      }
    }
  }
  if (active) {
#pragma unroll
    for (int j = 0; j < 49; ++j) atomicAdd(dbias + ((size_t)head * 49 + j) * 49 + t, db[j]);
  }
}

}  // namespace

// ---- launchers: every kernel's launch with its grid arithmetic, on plain pointers and sizes.  The engine
// (maxvit_train.hip) and the op-level entry points (maxvit_train_ops.hip: btsbot_op_mvt_*, one kernel group at a time for
// the tests) run the same ones.  Row blocks (gridDim.y) of the BatchNorm reductions over M rows, and of dw3_bwd_w over
// npix output pixels:
unsigned bn_row_blocks(long M) { return (unsigned)(M / 256 > 256 ? 256 : (M / 256 > 0 ? M / 256 : 1)); }
unsigned dw3_bwd_w_row_blocks(long npix) { return (unsigned)(npix / 64 > 256 ? 256 : (npix / 64 > 0 ? npix / 64 : 1)); }
// attention backward: three workgroups fit a CU (LDS): 768 x 4 of them walk the units, each for one head
long attn_bwd_groups_per_head(long units, int heads) { return units < 3072 / heads ? units : 3072 / heads; }

// BatchNorm2d, training mode: batch statistics of x [M][C] into stat (mean | rstd), running statistics updated (or
// nullptr), y = act(...);  sums0 / sums: two zeroed slots of 2C floats
int launch_bn_train(const float* x, const float* w, const float* b, float* stat, float* sums0, float* sums, float* run_mean,
                    float* run_var, float* y, long M, int C, int act, hipStream_t st) {
  const dim3 grid((C + 63) / 64, bn_row_blocks(M));
  hipLaunchKernelGGL(col_moments_kernel, grid, dim3(256), 0, st, x, (const float*)nullptr, sums0, M, C);
  hipLaunchKernelGGL(bn_mean_kernel, dim3(nblk(C)), dim3(256), 0, st, sums0, stat, M, C);
  hipLaunchKernelGGL(col_moments_kernel, grid, dim3(256), 0, st, x, (const float*)stat, sums, M, C);
  hipLaunchKernelGGL(bn_finish_kernel, dim3(nblk(C)), dim3(256), 0, st, sums, stat, run_mean, run_var, M, C);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(nblk(M * C / 4)), dim3(256), 0, st, x, stat, w, b, y, M * C / 4, C, act);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
// ... and its backward: dy = gradient w.r.t. the layer's output (behind the activation), dx (+)= gradient w.r.t. x (dx may
// be dy), dw / db += ;  sums: one zeroed slot
int launch_bn_train_bwd(const float* x, const float* dy, const float* stat, const float* w, const float* b, float* sums,
                        float* dx, float* dw, float* db, long M, int C, int act, int accumulate, hipStream_t st) {
  const dim3 grid((C + 63) / 64, bn_row_blocks(M));
  hipLaunchKernelGGL(bn_bwd_sums_kernel, grid, dim3(256), 0, st, x, dy, stat, w, b, sums, M, C, act);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(nblk(M * C / 4)), dim3(256), 0, st, x, dy, stat, w, b, (const float*)sums, dx,
                     dw, db, M, C, act, accumulate);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
// depthwise 3x3 on packed taps w9 [9][C] (launch_mv_pack_dw)
int launch_dw3_fwd(const float* in, const float* w9, const float* bias, float* out, int B, int H, int C, int s, hipStream_t st) {
  const long Mo = (long)B * (H / s) * (H / s);
  hipLaunchKernelGGL(dw3_fwd_kernel, dim3(nblk(Mo * C / 4)), dim3(256), 0, st, in, w9, bias, out, B, H, C, s);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
int launch_dw3_bwd_in(const float* dout, const float* w9, float* din, int B, int H, int C, int s, hipStream_t st) {
  const long Min = (long)B * H * H;
  hipLaunchKernelGGL(dw3_bwd_in_kernel, dim3(nblk(Min * C / 4)), dim3(256), 0, st, dout, w9, din, B, H, C, s);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
// filter / bias gradients: tap-major into the scratch g9 [10][C] (zeroed here), then added into the master layout dw [C][1][3][3]
int launch_dw3_bwd_w(const float* in, const float* dout, float* g9, float* dw, float* dbias, int B, int H, int C, int s,
                     hipStream_t st) {
  HIP_TRY(hipMemsetAsync(g9, 0, (size_t)10 * C * 4, st));
  const long npix = (long)B * (H / s) * (H / s);
  const dim3 grid((C + 63) / 64, dw3_bwd_w_row_blocks(npix));
  hipLaunchKernelGGL(dw3_bwd_w_kernel, grid, dim3(256), 0, st, in, dout, g9, dbias, B, H, C, s);
  hipLaunchKernelGGL(unpack_dw_grad_kernel, dim3(nblk(9L * C)), dim3(256), 0, st, (const float*)g9, dw, C);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
// attention backward of one layer: dqkv written, dtable [169][heads] += ;  dbias: scratch [32][2401], the gradient of the
// bias [heads <= 16][49][49] in its first half, the bias image bias_t in its second
int launch_attn_bwd(const float* qkv, const float* table, const float* dout, float* dqkv, float* dbias, float* dtable, int B,
                    int H, int C, int grid_mode, hipStream_t st) {
  const int heads = C / 32;
  HIP_TRY(hipMemsetAsync(dbias, 0, (size_t)heads * 2401 * 4, st));
  TRY(launch_mv_pack_relbias(table, dbias + 16 * 2401, heads, st));
  const long units = (long)B * (H / 7) * (H / 7);
  const long per_head = attn_bwd_groups_per_head(units, heads);
  hipLaunchKernelGGL(mv_attn_bwd_kernel, dim3((unsigned)(per_head * heads)), dim3(64), 0, st, qkv, (const float*)(dbias + 16 * 2401),
                     dout, dqkv, dbias, H, C, grid_mode, (int)units);
  hipLaunchKernelGGL(relbias_grad_kernel, dim3(nblk(169 * heads)), dim3(256), 0, st, (const float*)dbias, dtable, heads);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
// y[b][p][c] = a[b][p][c] * g[b][c]   (y may be a)
int launch_gate_mul(const float* a, const float* g, float* y, int B, int P, int C, hipStream_t st) {
  const long n4 = (long)B * P * C / 4;
  hipLaunchKernelGGL(gate_mul_kernel, dim3(nblk(n4)), dim3(256), 0, st, a, g, y, P, C, n4);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
// squeeze-excite of a2 [B][P][C]: pool = mean_p a2, r = silu(rpre = fc1 pool), gate = sigmoid(fc2 r), gated = a2 * gate
int launch_se_fwd(const float* a2, const float* w1, const float* b1, const float* w2, const float* b2, float* pool, float* rpre,
                  float* r, float* gate, float* gated, int B, int P, int C, int RD, hipStream_t st) {
  hipLaunchKernelGGL(alert_colsum_kernel, dim3((C + 63) / 64, B), dim3(256), 0, st, a2, (const float*)nullptr, pool, P, C,
                     1.0f / (float)P);
  hipLaunchKernelGGL(lin_fwd_small_kernel, dim3(nblk((long)B * RD)), dim3(256), 0, st, (const float*)pool, w1, b1, rpre, r, B, C,
                     RD, 1);
  hipLaunchKernelGGL(lin_fwd_small_kernel, dim3(nblk((long)B * C)), dim3(256), 0, st, (const float*)r, w2, b2, (float*)nullptr,
                     gate, B, RD, C, 2);
  return launch_gate_mul(a2, gate, gated, B, P, C, st);
}
// ... and its backward, in place: d [B][P][C] holds d(gated) and leaves as d(a2);  dg[b][c] = sum_p d(gated) a2,
// d(a2) = d(gated) g + the pooled path;  dw1 / db1 / dw2 / db2 += ;  dgate, dpool, dgpre [B][C] and dr [B][RD]: scratch
int launch_se_bwd(float* d, const float* a2, const float* pool, const float* rpre, const float* r, const float* gate,
                  const float* w1, const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dgate, float* dr,
                  float* dpool, float* dgpre, int B, int P, int C, int RD, hipStream_t st) {
  hipLaunchKernelGGL(alert_colsum_kernel, dim3((C + 63) / 64, B), dim3(256), 0, st, (const float*)d, a2, dgate, P, C, 1.0f);
  TRY(launch_gate_mul(d, gate, d, B, P, C, st));                                   // d(a2) = d(gated) * g, in place
  hipLaunchKernelGGL(act_bwd_small_kernel, dim3(nblk((long)B * C)), dim3(256), 0, st, (const float*)dgate, gate, dgpre, B * C, 2);
  hipLaunchKernelGGL(lin_bwd_w_small_kernel, dim3(nblk((long)C * RD)), dim3(256), 0, st, (const float*)dgpre, r, dw2, db2, B, RD,
                     C);
  hipLaunchKernelGGL(lin_bwd_in_small_kernel, dim3(nblk((long)B * RD)), dim3(256), 0, st, (const float*)dgpre, w2, dr, B, RD, C);
  hipLaunchKernelGGL(act_bwd_small_kernel, dim3(nblk((long)B * RD)), dim3(256), 0, st, (const float*)dr, rpre, dr, B * RD, 1);
  hipLaunchKernelGGL(lin_bwd_w_small_kernel, dim3(nblk((long)RD * C)), dim3(256), 0, st, (const float*)dr, pool, dw1, db1, B, C,
                     RD);
  hipLaunchKernelGGL(lin_bwd_in_small_kernel, dim3(nblk((long)B * C)), dim3(256), 0, st, (const float*)dr, w1, dpool, B, C, RD);
  const long n = (long)B * P * C;
  hipLaunchKernelGGL(bcast_add_kernel, dim3(nblk(n)), dim3(256), 0, st, d, (const float*)dpool, P, C, n, 1.0f / (float)P);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
int launch_bcast_set(float* d, const float* v, int B, int P, int C, float scale, hipStream_t st) {
  const long n = (long)B * P * C;
  hipLaunchKernelGGL(bcast_set_kernel, dim3(nblk(n)), dim3(256), 0, st, d, v, P, C, n, scale);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
int launch_avgpool2_bwd(const float* g, float* dx, int B, int H, int C, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(avgpool2_bwd_kernel, dim3(nblk((long)B * H * H * C)), dim3(256), 0, st, g, dx, B, H, C, accumulate);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
int launch_add(float* a, const float* b, long n4, hipStream_t st) {   // a += b, n4 = count / 4
  hipLaunchKernelGGL(add_kernel, dim3(nblk(n4)), dim3(256), 0, st, a, b, n4);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
int launch_gelu_fwd(const float* pre, float* out, long n4, hipStream_t st) {
  hipLaunchKernelGGL(gelu_fwd_kernel, dim3(nblk(n4)), dim3(256), 0, st, pre, out, n4);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
int launch_gelu_bwd(const float* pre, float* d, long n4, hipStream_t st) {
  hipLaunchKernelGGL(gelu_bwd_kernel, dim3(nblk(n4)), dim3(256), 0, st, pre, d, n4);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
int launch_col2im3(const float* dcol, float* din, int B, int H, int C, hipStream_t st) {
  hipLaunchKernelGGL(col2im3_kernel, dim3(nblk((long)B * H * H * C)), dim3(256), 0, st, dcol, din, B, H, C);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
int launch_unpack_conv3_grad(const float* gp, float* g, int O, int C, int ldp, hipStream_t st) {
  hipLaunchKernelGGL(unpack_conv3_grad_kernel, dim3(nblk((long)O * C * 9)), dim3(256), 0, st, gp, g, O, C, ldp);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
