// LayerNorm and depthwise backward of the ConvNeXt image branch, one launch per step (gfx950), and the fc2 / layer-scale
// gradients.  Of the block
//
//   y = x + gamma * fc2(gelu(fc1(LN(dwconv(x)))))
//
// given G = dy^T h (the filter-gradient GEMM in front): dW2 = gamma (.) G, dgamma = <W2, G> + b2 * colsum(dy)
// (fc2_grads_kernel); LayerNorm backward on the depthwise output (ln_bwd_kernel, ln_bwd_narrow_kernel); depthwise dgrad =
// the same depthwise kernel with the 7x7 filter flipped (dw_plain_kernel); depthwise wgrad = per-tap correlation reduced
// over pixels and alerts (dw_wgrad_kernel); on 1x1 maps the three as one kernel (ln_dw1_bwd_kernel).  Reductions over the
// batch use fp32 atomics into the (pre-zeroed) gradient arena, or det_reduce.hip's partial rows.  dwln_bwd.hip fuses the
// three steps for the larger maps; cn_bwd_ops.hip exposes these launchers one at a time.
#include "common.h"

namespace {

// fc2 weight/scale gradients from G = dy^T h:  dW2[c][k] = gamma[c] G[c][k];
// dgamma[c] = sum_k W2[c][k] G[c][k] + b2[c] S[c];  db2[c] = gamma[c] S[c]    (S = colsum(dy))
// G and S are accumulators of the filter-gradient GEMM in front: every element is read exactly once here and left
// zero for the next block's GEMM (was: a memset launch per block)
__global__ __launch_bounds__(256) void fc2_grads_kernel(float* __restrict__ G,
                                                        float* __restrict__ S,
                                                        const float* __restrict__ w2,
                                                        const float* __restrict__ b2,
                                                        const float* __restrict__ gamma,
                                                        float* dW2, float* db2, float* dgamma,
                                                        int C, int H) {
  const int c = blockIdx.x;
  const float g = gamma[c];
  float part = 0.f;
  for (int k = threadIdx.x; k < H; k += 256) {
    const float gv = G[(size_t)c * H + k];
    G[(size_t)c * H + k] = 0.f;
    dW2[(size_t)c * H + k] = g * gv;
    part += w2[(size_t)c * H + k] * gv;
  }
  part = wave_sum(part);
  __shared__ float sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float sc = S[c];
    S[c] = 0.f;
    dgamma[c] = sh[0] + sh[1] + sh[2] + sh[3] + b2[c] * sc;
    db2[c] = g * sc;
  }
}

// Source row of the LayerNorm backward's incoming gradient.  Dense: dxn + r * C.  After a 2x2 / stride-2 downsample
// (patch_hw = side of the downsample's INPUT map): the gradient arrives as patches [B * HO * HO][4 C] (k = q * C + c,
// q = 2 (y & 1) + (x & 1)); input pixel r = (b, y, x) reads its slice of the patch that covers it, pixels outside
// every patch (the odd last row / column) get zero.  (Was: unpatch_kernel scattering into a dense map first.)
__device__ __forceinline__ const float* ln_bwd_src(const float* dxn, long r, int C, int patch_hw, bool* zero) {
  *zero = false;
  if (patch_hw == 0) return dxn + r * C;
  const int P = patch_hw * patch_hw, HO = patch_hw / 2;
  const long b = r / P;
  const int p = (int)(r - b * P), iy = p / patch_hw, ix = p - iy * patch_hw;
  if (iy >= 2 * HO || ix >= 2 * HO) {
    *zero = true;
    return dxn;
  }
  return dxn + ((b * HO + (iy >> 1)) * HO + (ix >> 1)) * 4 * (long)C + ((iy & 1) * 2 + (ix & 1)) * C;
}

// LayerNorm backward over the C channels of each row.  One wave per row (grid-stride).
//   xhat = (d - mean) * rstd;  t = dxn * g;  dd = rstd * (t - mean(t) - xhat * mean(t * xhat))
//   dg += dxn * xhat;  dbeta += dxn
template <int CPT>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ d,
                                                     const float* __restrict__ dxn,
                                                     const float* __restrict__ g, float* dd,
                                                     float* dg, float* dbeta, long rows, int C,
                                                     void* __restrict__ out16, int prec16, int patch_hw,
                                                     float* part) {
  const int lane = threadIdx.x & 63;
  const long w0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  float gl[CPT], adg[CPT], adb[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = lane + 64 * i;
    gl[i] = c < C ? g[c] : 0.f;
    adg[i] = adb[i] = 0.f;
  }
  // dd may be dxn (in place): a load cannot move above an earlier store, so the NEXT row's pieces are requested
  // explicitly before this row's stores (they arrive under the four wave reductions)
  float nv[CPT], ndx[CPT];
  auto fetch = [&](long r) {
    bool zero;
    const float* src = ln_bwd_src(dxn, r, C, patch_hw, &zero);
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = lane + 64 * i;
      nv[i] = c < C ? d[r * C + c] : 0.f;
      const float g = c < C ? src[c] : 0.f;
      ndx[i] = zero ? 0.f : g;
    }
  };
  if (w0 < rows) fetch(w0);
  for (long r = w0; r < rows; r += nw) {
    float v[CPT], t[CPT], dxr[CPT];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      v[i] = nv[i];
      dxr[i] = ndx[i];
      s += v[i];
    }
    if (r + nw < rows) fetch(r + nw);
    const float mean = wave_sum(s) / C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = lane + 64 * i;
      v[i] = c < C ? v[i] - mean : 0.f;
      q += v[i] * v[i];
    }
    const float rstd = rsqrtf(wave_sum(q) / C + LN_EPS);
    float st = 0.f, stx = 0.f;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const float dx = dxr[i];
      v[i] *= rstd;                     // xhat
      t[i] = dx * gl[i];
      st += t[i];
      stx += t[i] * v[i];
      adg[i] += dx * v[i];
      adb[i] += dx;
    }
    st = wave_sum(st) / C;
    stx = wave_sum(stx) / C;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = lane + 64 * i;
      if (c < C) {
        const float o = rstd * (t[i] - st - v[i] * stx);
        dd[r * C + c] = o;
        if (out16 != nullptr) {   // the same values as the next 16-bit GEMM's operand (was a cast launch)
          if (prec16 == BTSBOT_BF16) reinterpret_cast<bf16_t*>(out16)[r * C + c] = (bf16_t)o;
          else reinterpret_cast<f16_t*>(out16)[r * C + c] = (f16_t)o;
        }
      }
    }
  }
  // the block's 4 waves meet in LDS: one atomic per channel per block
  __shared__ float sh[2][4][CPT * 64];
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    sh[0][wv][lane + 64 * i] = adg[i];
    sh[1][wv][lane + 64 * i] = adb[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    det_add(dg + c, sh[0][0][c] + sh[0][1][c] + sh[0][2][c] + sh[0][3][c], part, (size_t)blockIdx.x * 2 * C + c);
    det_add(dbeta + c, sh[1][0][c] + sh[1][1][c] + sh[1][2][c] + sh[1][3][c], part, (size_t)blockIdx.x * 2 * C + C + c);
  }
}

// 1x1 maps (stage 3): the block's LayerNorm backward, depthwise filter gradient and depthwise input gradient in one
// launch.  On a 1x1 map the 7x7 depthwise convolution is its centre tap, so everything is per (alert, channel):
//   dd = LN'(d) . dxn;   dy += dd * w[24][c];   dW[c][24] += dd * x_in;   db[c] += dd;   dg, dbeta as ln_bwd_kernel
// One wave per alert (grid-stride); the workgroup's four waves meet in LDS, one atomic per channel per workgroup and
// gradient.  (Was ln_bwd_kernel + dw_wgrad_kernel<1> + its column sum + dw_plain_kernel<1>: 48 us per block.)
template <int CPT>
__global__ __launch_bounds__(256) void ln_dw1_bwd_kernel(const float* __restrict__ d, const float* __restrict__ dxn,
                                                         const float* __restrict__ g, const float* __restrict__ xin,
                                                         const float* __restrict__ wc, float* dy,
                                                         void* __restrict__ out16, int prec16, float* dg, float* dbeta,
                                                         float* dw, float* dbias, long rows, int C, float* part) {
  const int lane = threadIdx.x & 63;
  const long w0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  float gl[CPT], wl[CPT], adg[CPT], adb[CPT], adw[CPT], adc[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = lane + 64 * i;
    gl[i] = c < C ? g[c] : 0.f;
    wl[i] = c < C ? wc[c] : 0.f;
    adg[i] = adb[i] = adw[i] = adc[i] = 0.f;
  }
  // Two rows per trip (r and r + nw): their 8 x CPT loads are in flight together and their wave sums interleave -- one
  // row per trip was a chain of dependent memory round trips and lane reductions (8 rows per wave: 23-27 us per launch
  // for a 2 MB tensor)
  for (long r = w0; r < rows; r += 2 * nw) {
    const bool two = r + nw < rows;          // wave-uniform
    const long rr[2] = {r, two ? r + nw : r};
    float v[2][CPT], t[2][CPT], dxr[2][CPT], xr[2][CPT], yr[2][CPT];
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int c = lane + 64 * i;
        v[u][i] = c < C ? d[rr[u] * C + c] : 0.f;
        dxr[u][i] = c < C && (u == 0 || two) ? dxn[rr[u] * C + c] : 0.f;   // (an absent second row: dxn = 0, so dd = 0)
        xr[u][i] = c < C ? xin[rr[u] * C + c] : 0.f;
        yr[u][i] = c < C ? dy[rr[u] * C + c] : 0.f;
        s[u] += v[u][i];
      }
    float mean[2], q[2] = {0.f, 0.f}, rstd[2], st[2] = {0.f, 0.f}, stx[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) mean[u] = wave_sum(s[u]) / C;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int c = lane + 64 * i;
        v[u][i] = c < C ? v[u][i] - mean[u] : 0.f;
        q[u] += v[u][i] * v[u][i];
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) rstd[u] = rsqrtf(wave_sum(q[u]) / C + LN_EPS);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        v[u][i] *= rstd[u];                     // xhat
        t[u][i] = dxr[u][i] * gl[i];
        st[u] += t[u][i];
        stx[u] += t[u][i] * v[u][i];
        adg[i] += dxr[u][i] * v[u][i];
        adb[i] += dxr[u][i];
      }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      st[u] = wave_sum(st[u]) / C;
      stx[u] = wave_sum(stx[u]) / C;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u == 1 && !two) break;
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const int c = lane + 64 * i;
        if (c < C) {
          const float dd = rstd[u] * (t[u][i] - st[u] - v[u][i] * stx[u]);
          adw[i] += dd * xr[u][i];
          adc[i] += dd;
          const float o = yr[u][i] + dd * wl[i];
          dy[rr[u] * C + c] = o;
          if (out16 != nullptr) {
            if (prec16 == BTSBOT_BF16) reinterpret_cast<bf16_t*>(out16)[rr[u] * C + c] = (bf16_t)o;
            else reinterpret_cast<f16_t*>(out16)[rr[u] * C + c] = (f16_t)o;
          }
        }
      }
    }
  }
  __shared__ float sh[4][4][CPT * 64];
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    sh[0][wv][lane + 64 * i] = adg[i];
    sh[1][wv][lane + 64 * i] = adb[i];
    sh[2][wv][lane + 64 * i] = adw[i];
    sh[3][wv][lane + 64 * i] = adc[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    const size_t row = (size_t)blockIdx.x * 4 * C;
    det_add(dg + c, sh[0][0][c] + sh[0][1][c] + sh[0][2][c] + sh[0][3][c], part, row + c);
    det_add(dbeta + c, sh[1][0][c] + sh[1][1][c] + sh[1][2][c] + sh[1][3][c], part, row + C + c);
    det_add(dw + (size_t)c * 49 + 24, sh[2][0][c] + sh[2][1][c] + sh[2][2][c] + sh[2][3][c], part, row + 2 * C + c);
    det_add(dbias + c, sh[3][0][c] + sh[3][1][c] + sh[3][2][c] + sh[3][3][c], part, row + 3 * C + c);
  }
}

// Depthwise 7x7 p3 without LayerNorm, fp32 in / fp32 out, one workgroup per alert, thread =
// channel (grid-stride over channels), whole map in LDS.  out = conv(x, w) [+ bias] [+ addend].
// With the taps flipped (w'[t] = w[48 - t]) this is the gradient w.r.t. the conv input.
template <int HW>
__global__ __launch_bounds__(256) void dw_plain_kernel(const float* __restrict__ x,
                                                       const float* __restrict__ w, int flip,
                                                       const float* __restrict__ bias,
                                                       const float* addend, float* out, int C,
                                                       void* __restrict__ out16, int prec16) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [HW*HW][C] map | [49][C] taps
  constexpr int P = HW * HW;
  float* ws = xs + P * C;
  const size_t base = (size_t)blockIdx.x * P * C;
  // taps in LDS (already flipped if asked) and a rolled ky loop: with the 49 taps in registers and the ky
  // loop unrolled the 15x15 instance needed 256 VGPRs + scratch and ran one wave per SIMD (131 us per launch)
  constexpr bool TAPS_LDS = HW >= 15;
  constexpr bool TAPS_GLOBAL = HW == 7;   // 7x7 maps: rolled ky loop, the row's 7 taps re-read from L1 per ky
  constexpr int KY_UNROLL = (TAPS_LDS || TAPS_GLOBAL) ? 1 : 7;   // small maps: the taps stay in registers (staging them costs more
                                        // than the whole convolution there)
  if (TAPS_LDS)
    for (int i = threadIdx.x; i < 49 * C; i += 256) {
      const int t = i / C, cc = i - t * C;
      ws[i] = w[(flip ? 48 - t : t) * C + cc];
    }
  {
    // 16-byte pieces, eight in flight per thread before the first LDS store (the scalar copy loop waited
    // for every 4-byte load: 56 exposed HBM latencies per workgroup at 15x15x64)
    const float4* src = reinterpret_cast<const float4*>(x + base);
    float4* dst = reinterpret_cast<float4*>(xs);
    const int n4 = P * C / 4;
    for (int i0 = threadIdx.x; i0 < n4; i0 += 2048) {
      float4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = src[min(i0 + k * 256, n4 - 1)];   // (clamped: no conditional definition)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (i0 + k * 256 < n4) dst[i0 + k * 256] = v[k];
    }
  }
  __syncthreads();
  // thread = (channel, row group): narrow maps (C < 256) spread their rows over the idle waves
  const int G = C < 256 ? 256 / C : 1;
  const int rg = C < 256 ? threadIdx.x / C : 0;
  const bool idle = C < 256 && (int)threadIdx.x >= G * C;   // C does not divide 256 (nano)
  for (int c = idle ? C : (C < 256 ? threadIdx.x % C : threadIdx.x); c < C; c += 256) {
    const float b = bias != nullptr ? bias[c] : 0.f;
    float wv[(TAPS_LDS || TAPS_GLOBAL) ? 1 : 49];
    if (!TAPS_LDS && !TAPS_GLOBAL) {
#pragma unroll
      for (int t = 0; t < 49; ++t) wv[t] = w[(flip ? 48 - t : t) * C + c];
    }
    for (int y = rg; y < HW; y += G) {
      float acc[HW];
      // the row's addend pieces are requested before the taps run: `out` may be `addend` (dx = dy + conv), so inside
      // the store loop below every load had to wait for the previous store -- HW exposed HBM round trips per row
#pragma unroll
      for (int xx = 0; xx < HW; ++xx)
        acc[xx] = b + (addend != nullptr ? addend[base + (size_t)(y * HW + xx) * C + c] : 0.f);
#pragma unroll KY_UNROLL
      for (int ky = 0; ky < 7; ++ky) {
        const int iy = y + ky - 3;
        if (iy < 0 || iy >= HW) continue;
        float in[HW], wk[7];
#pragma unroll
        for (int xx = 0; xx < HW; ++xx) in[xx] = xs[(iy * HW + xx) * C + c];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
          wk[kx] = TAPS_LDS      ? ws[(ky * 7 + kx) * C + c]
                   : TAPS_GLOBAL ? w[(flip ? 48 - (ky * 7 + kx) : ky * 7 + kx) * C + c]
                                 : wv[(TAPS_LDS || TAPS_GLOBAL) ? 0 : ky * 7 + kx];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
#pragma unroll
          for (int xx = 0; xx < HW; ++xx) {
            const int ix = xx + kx - 3;
            if (ix >= 0 && ix < HW) acc[xx] = fmaf(in[ix], wk[kx], acc[xx]);
          }
      }
#pragma unroll
      for (int xx = 0; xx < HW; ++xx) {
        const size_t o = base + (size_t)(y * HW + xx) * C + c;
        out[o] = acc[xx];
        if (out16 != nullptr) {   // the same values as the next block's 16-bit GEMM operand (was a cast launch)
          if (prec16 == BTSBOT_BF16) reinterpret_cast<bf16_t*>(out16)[o] = (bf16_t)acc[xx];
          else reinterpret_cast<f16_t*>(out16)[o] = (f16_t)acc[xx];
        }
      }
    }
  }
}

// Depthwise filter gradient: sum_{alerts,pixels} dd[p][c] * x[p + delta_t][c] per tap, and sum dd
// for the bias.  Workgroup = GA alerts (sequentially), thread = (channel, row group); every row
// group writes ONE partial row [C*49 | C] which launch_dw_wgrad then column-sums into the gradient arena (the filter
// and its bias are adjacent there) -- no same-address atomic storm.
template <int HW>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const float* __restrict__ x,
                                                       const float* __restrict__ dd, float* dw,
                                                       float* dbias, int B, int C, int ga) {
  extern __shared__ __attribute__((aligned(16))) float sm[];   // xs [P][C], ds [P][C]
  constexpr int P = HW * HW;
  float* xs = sm;
  float* ds = sm + P * C;
  const int a0 = blockIdx.x * ga, a1 = min(B, a0 + ga);
  // thread = (channel, row group), as in dw_plain_kernel; every row group owns a partial row
  const int G = C < 256 ? 256 / C : 1;
  const int rg = C < 256 ? threadIdx.x / C : 0;
  for (int c0 = 0; c0 < C; c0 += 256) {
    const bool idle = C < 256 && (int)threadIdx.x >= G * C;   // C does not divide 256 (nano)
    const int c = idle ? C : (C < 256 ? threadIdx.x % C : c0 + threadIdx.x);
    float acc[49], ab = 0.f;
#pragma unroll
    for (int t = 0; t < 49; ++t) acc[t] = 0.f;
    for (int a = a0; a < a1; ++a) {
      __syncthreads();
      const size_t base = (size_t)a * P * C;
      {
        const float4* sx = reinterpret_cast<const float4*>(x + base);
        const float4* sd = reinterpret_cast<const float4*>(dd + base);
        float4* dx4 = reinterpret_cast<float4*>(xs);
        float4* dd4 = reinterpret_cast<float4*>(ds);
        const int n4 = P * C / 4;
        // 16 pieces in flight per thread (two trips for a 15x15x64 map; with 4 in flight the 7 trips were 7 exposed
        // HBM latencies per alert, most of this kernel's time: one workgroup per CU, nothing else to switch to)
        constexpr int NB = 8;
        for (int i0 = threadIdx.x; i0 < n4; i0 += 256 * NB) {
          float4 a[NB], b[NB];
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            const int ii = min(i0 + k * 256, n4 - 1);
            a[k] = sx[ii];
            b[k] = sd[ii];
          }
#pragma unroll
          for (int k = 0; k < NB; ++k)
            if (i0 + k * 256 < n4) {
              dx4[i0 + k * 256] = a[k];
              dd4[i0 + k * 256] = b[k];
            }
        }
      }
      __syncthreads();
      if (c < C) {
        for (int y = rg; y < HW; y += G) {
          float g[HW];
#pragma unroll
          for (int xx = 0; xx < HW; ++xx) {
            g[xx] = ds[(y * HW + xx) * C + c];
            ab += g[xx];
          }
#pragma unroll
          for (int ky = 0; ky < 7; ++ky) {
            const int iy = y + ky - 3;
            if (iy < 0 || iy >= HW) continue;
            float in[HW];
#pragma unroll
            for (int xx = 0; xx < HW; ++xx) in[xx] = xs[(iy * HW + xx) * C + c];
#pragma unroll
            for (int kx = 0; kx < 7; ++kx)
#pragma unroll
              for (int xx = 0; xx < HW; ++xx) {
                const int ix = xx + kx - 3;
                if (ix >= 0 && ix < HW) acc[ky * 7 + kx] = fmaf(g[xx], in[ix], acc[ky * 7 + kx]);
              }
          }
        }
      }
    }
    if (c < C) {   // this workgroup's partial row: [C][49] filter taps, then [C] biases
      float* row = dw + ((size_t)blockIdx.x * G + rg) * 50 * C;
#pragma unroll
      for (int t = 0; t < 49; ++t) row[(size_t)c * 49 + t] = acc[t];
      row[(size_t)49 * C + c] = ab;
    }
  }
}

}  // namespace

int launch_fc2_grads(float* G, float* S, const float* w2, const float* b2,
                     const float* gamma, float* dW2, float* db2, float* dgamma, int C, int H,
                     hipStream_t st) {
  hipLaunchKernelGGL(fc2_grads_kernel, dim3(C), dim3(256), 0, st, G, S, w2, b2, gamma, dW2, db2,
                     dgamma, C, H);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

// Narrow maps (C = 4 * LPR, LPR = 16 or 32 lanes per pixel row): every lane owns 4 consecutive
// channels (float4 loads), a wave normalises 64 / LPR rows at once and runs two such groups per
// iteration, so that 4 x 16-byte loads per lane are in flight instead of one dword.
template <int LPR>
__global__ __launch_bounds__(256) void ln_bwd_narrow_kernel(const float* __restrict__ d,
                                                            const float* __restrict__ dxn,
                                                            const float* __restrict__ g, float* dd,
                                                            float* dg, float* dbeta, long rows,
                                                            void* __restrict__ out16, int prec16, int patch_hw,
                                                            float* part) {
  constexpr int C = 4 * LPR, R = 64 / LPR;       // rows per wave pass
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int sub = lane / LPR, l = lane % LPR;
  const float4 gl = *reinterpret_cast<const float4*>(g + 4 * l);
  float adg[4] = {0.f, 0.f, 0.f, 0.f}, adb[4] = {0.f, 0.f, 0.f, 0.f};
  auto gsum = [](float v) {
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
  };
  const long stride = (long)gridDim.x * 4 * R * 2;
  // (dd may be dxn: the next pass's pieces are requested before this pass's stores, as in ln_bwd_kernel)
  float4 nv[2], ndx[2];
  auto fetch = [&](long r0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long r = r0 + u * R + sub;
      const long rr = r < rows ? r : 0;
      nv[u] = *reinterpret_cast<const float4*>(d + rr * C + 4 * l);
      bool zero;
      const float* src = ln_bwd_src(dxn, rr, C, patch_hw, &zero);
      const float4 g4 = *reinterpret_cast<const float4*>(src + 4 * l);
      ndx[u] = zero ? make_float4(0.f, 0.f, 0.f, 0.f) : g4;
    }
  };
  const long rfirst = ((long)blockIdx.x * 4 + wv) * R * 2;
  if (rfirst < rows) fetch(rfirst);
  for (long r0 = rfirst; r0 < rows; r0 += stride) {
    float4 v[2], dx[2];
    bool ok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      ok[u] = r0 + u * R + sub < rows;
      v[u] = nv[u];
      dx[u] = ndx[u];
    }
    if (r0 + stride < rows) fetch(r0 + stride);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long r = r0 + u * R + sub;
      float x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      const float dxa[4] = {dx[u].x, dx[u].y, dx[u].z, dx[u].w};
      const float ga[4] = {gl.x, gl.y, gl.z, gl.w};
      const float mean = gsum((x[0] + x[1]) + (x[2] + x[3])) * (1.f / C);
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[i] -= mean;
        q += x[i] * x[i];
      }
      const float rstd = rsqrtf(gsum(q) * (1.f / C) + LN_EPS);
      float t[4], st = 0.f, stx = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[i] *= rstd;
        t[i] = dxa[i] * ga[i];
        st += t[i];
        stx += t[i] * x[i];
        if (ok[u]) {
          adg[i] += dxa[i] * x[i];
          adb[i] += dxa[i];
        }
      }
      st = gsum(st) * (1.f / C);
      stx = gsum(stx) * (1.f / C);
      if (ok[u]) {
        const float4 o = make_float4(rstd * (t[0] - st - x[0] * stx), rstd * (t[1] - st - x[1] * stx),
                                     rstd * (t[2] - st - x[2] * stx), rstd * (t[3] - st - x[3] * stx));
        *reinterpret_cast<float4*>(dd + r * C + 4 * l) = o;
        if (out16 != nullptr) {   // the same values as the next 16-bit GEMM's operand (was a cast launch)
          if (prec16 == BTSBOT_BF16) {
            typedef bf16_t __attribute__((ext_vector_type(4))) b4;
            *reinterpret_cast<b4*>(reinterpret_cast<bf16_t*>(out16) + r * C + 4 * l) =
                b4{(bf16_t)o.x, (bf16_t)o.y, (bf16_t)o.z, (bf16_t)o.w};
          } else {
            typedef f16_t __attribute__((ext_vector_type(4))) h4;
            *reinterpret_cast<h4*>(reinterpret_cast<f16_t*>(out16) + r * C + 4 * l) =
                h4{(f16_t)o.x, (f16_t)o.y, (f16_t)o.z, (f16_t)o.w};
          }
        }
      }
    }
  }
  // row groups of the wave and the 4 waves meet in LDS: one atomic per channel per block
  __shared__ float sh[2][4 * R][C];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sh[0][wv * R + sub][4 * l + i] = adg[i];
    sh[1][wv * R + sub][4 * l + i] = adb[i];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int j = 0; j < 4 * R; ++j) {
      a += sh[0][j][c];
      b += sh[1][j][c];
    }
    det_add(dg + c, a, part, (size_t)blockIdx.x * 2 * C + c);
    det_add(dbeta + c, b, part, (size_t)blockIdx.x * 2 * C + C + c);
  }
}

int launch_ln_bwd(const float* d, const float* dxn, const float* g, float* dd, float* dg,
                  float* dbeta, long rows, int C, hipStream_t st, void* out16, int prec16, int patch_hw) {
  if (rows <= 0) return BTSBOT_OK;
  static const long cap = [] {
    const long v = switch_int(SW_LNBWD_BLOCKS, 0);   // tuning knob: workgroups (= same-address atomics per channel;
                                                            //  measured per step: 256 4.64 ms, 384/512 4.58, 1024 4.70, 2048 5.02)
    return v >= 1 ? v : 512;
  }();
  long blocks = (rows + 3) / 4;
  if (blocks > cap) blocks = cap;     // <= cap same-address atomics per channel
  if (C == 64 || C == 128) {
    const int rpb = 4 * (C == 64 ? 4 : 2) * 2;   // rows per block pass
    long nb = (rows + rpb - 1) / rpb;
    if (nb > cap) nb = cap;
    float* part = det_alloc((size_t)nb * 2 * C);
    if (C == 64)
      hipLaunchKernelGGL((ln_bwd_narrow_kernel<16>), dim3((unsigned)nb), dim3(256), 0, st, d, dxn, g,
                         dd, dg, dbeta, rows, out16, prec16, patch_hw, part);
    else
      hipLaunchKernelGGL((ln_bwd_narrow_kernel<32>), dim3((unsigned)nb), dim3(256), 0, st, d, dxn, g,
                         dd, dg, dbeta, rows, out16, prec16, patch_hw, part);
    LAUNCH_CHECK();
    if (part != nullptr) {
      const DetOut o[2] = {{dg, 1}, {dbeta, 1}};
      return launch_det_reduce(part, (int)nb, C, 2, o, st);
    }
    return BTSBOT_OK;
  }
  const int cpt = (C + 63) / 64;
  float* part = det_alloc((size_t)blocks * 2 * C);
#define LNB(CPT)                                                                                \
  hipLaunchKernelGGL((ln_bwd_kernel<CPT>), dim3((unsigned)blocks), dim3(256), 0, st, d, dxn, g, \
                     dd, dg, dbeta, rows, C, out16, prec16, patch_hw, part)
  if (cpt <= 1) LNB(1);
  else if (cpt <= 2) LNB(2);
  else if (cpt <= 4) LNB(4);
  else if (cpt <= 5) LNB(5);
  else if (cpt <= 8) LNB(8);
  else if (cpt <= 10) LNB(10);
  else {
    btsbot_set_error("ln_bwd: C=%d too wide", C);
    return BTSBOT_ERR_INVALID_ARG;
  }
#undef LNB
  LAUNCH_CHECK();
  if (part != nullptr) {
    const DetOut o[2] = {{dg, 1}, {dbeta, 1}};
    return launch_det_reduce(part, (int)blocks, C, 2, o, st);
  }
  return BTSBOT_OK;
}

// w: taps [49][C] (the centre row is read); dw: filter gradient [C][49], dbias [C] (master-arena layout)
int launch_ln_dw1_bwd(const float* d, const float* dxn, const float* g, const float* xin, const float* w, float* dy,
                      void* out16, int prec16, float* dg, float* dbeta, float* dw, float* dbias, long rows, int C,
                      hipStream_t st) {
  if (rows <= 0) return BTSBOT_OK;
  long blocks = (rows + 3) / 4;
  if (blocks > 32) blocks = 32;   // 4 x <= 32 same-address atomics per channel: with 256 workgroups the step was 0.04 ms slower
  const float* wc = w + (size_t)24 * C;
  const int cpt = (C + 63) / 64;
  float* part = det_alloc((size_t)blocks * 4 * C);
#define LD1(CPT)                                                                                       \
  hipLaunchKernelGGL((ln_dw1_bwd_kernel<CPT>), dim3((unsigned)blocks), dim3(256), 0, st, d, dxn, g, xin, wc, dy, \
                     out16, prec16, dg, dbeta, dw, dbias, rows, C, part)
  if (cpt <= 8) LD1(8);
  else if (cpt <= 10) LD1(10);
  else {
    btsbot_set_error("ln_dw1_bwd: C=%d too wide", C);
    return BTSBOT_ERR_INVALID_ARG;
  }
#undef LD1
  LAUNCH_CHECK();
  if (part != nullptr) {
    const DetOut o[4] = {{dg, 1}, {dbeta, 1}, {dw + 24, 49}, {dbias, 1}};
    return launch_det_reduce(part, (int)blocks, C, 4, o, st);
  }
  return BTSBOT_OK;
}

int launch_dw_plain(const float* x, const float* w, int flip, const float* bias,
                    const float* addend, float* out, int B, int HW, int C, hipStream_t st,
                    void* out16, int prec16) {
  if (B <= 0) return BTSBOT_OK;
  const size_t lds = ((size_t)HW * HW + 49) * C * sizeof(float);
#define DWP(H)                                                                                 \
  {                                                                                            \
    static size_t attr = 0;                                                                    \
    if (lds > attr) {                                                                          \
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(dw_plain_kernel<H>),           \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));      \
      attr = lds;                                                                              \
    }                                                                                          \
    hipLaunchKernelGGL((dw_plain_kernel<H>), dim3(B), dim3(256), lds, st, x, w, flip, bias,    \
                       addend, out, C, out16, prec16);                                         \
  }
  if (HW == 15) DWP(15)
  else if (HW == 7) DWP(7)
  else if (HW == 3) DWP(3)
  else if (HW == 1) DWP(1)
  else {
    btsbot_set_error("dw_plain: no kernel for HW=%d", HW);
    return BTSBOT_ERR_INVALID_ARG;
  }
#undef DWP
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int launch_dw_wgrad(const float* x, const float* dd, float* dw, float* dbias, float* partials,
                    int B, int HW, int C, hipStream_t st) {
  if (B <= 0) return BTSBOT_OK;
  if (dbias != dw + (size_t)49 * C) {
    btsbot_set_error("dw_wgrad: filter and bias gradients must be adjacent in the arena");
    return BTSBOT_ERR_INVALID_ARG;
  }
  const size_t lds = 2 * (size_t)HW * HW * C * sizeof(float);
  int ga = (B + 255) / 256;            // <= 256 workgroups => <= 256 atomics per filter tap
  if (ga < 1) ga = 1;
  const int grid = (B + ga - 1) / ga;
#define DWW(H)                                                                                 \
  {                                                                                            \
    static size_t attr = 0;                                                                    \
    if (lds > attr) {                                                                          \
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(dw_wgrad_kernel<H>),           \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));      \
      attr = lds;                                                                              \
    }                                                                                          \
    hipLaunchKernelGGL((dw_wgrad_kernel<H>), dim3(grid), dim3(256), lds, st, x, dd, partials,  \
                       dbias, B, C, ga);                                                       \
  }
  if (HW == 15) DWW(15)
  else if (HW == 7) DWW(7)
  else if (HW == 3) DWW(3)
  else if (HW == 1) DWW(1)
  else {
    btsbot_set_error("dw_wgrad: no kernel for HW=%d", HW);
    return BTSBOT_ERR_INVALID_ARG;
  }
#undef DWW
  LAUNCH_CHECK();
  return launch_colsum(BTSBOT_F32, partials, dw, grid * (C < 256 ? 256 / C : 1), 50 * C, st);
}
