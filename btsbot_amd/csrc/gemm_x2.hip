// Split-operand GEMM (BTSBOT_F16X2) for the MaxViT inference forward and the split ConvNeXt training step (gfx950).
//
//   out[m][n] = epi( sum_k X[m][k] * W[n][k] + bias[n] )
//
// X = fp32 activations [M][K], the maps the fp32 MaxViT schedule produces; W = a filter bank packed ONCE as two f16
// planes of the [N][K] layout PyTorch stores: heads hi = f16(w) at W, remainders lo = f16(w - hi) at W + N*K.
// Every value enters the products as head + remainder, and each product is lo*hi + hi*lo + hi*hi on
// v_mfma_f32_16x16x32_f16 with fp32 accumulation, small terms first: an fp32-class result at the
// f16 matrix rate.  The epilogues are the fp32 ones of gemm.hip (exact erf GELU, expf SiLU), output always fp32.
// Training (btsbot_set_option "train_split"): the forward's GELU_SAVE and the input-gradient products' DGELU / PLAIN.
// Their X is a gradient there: it enters scaled by 2^e (device_math.h: split_exp of its largest magnitude) so that its heads
// stay normal f16 values, and the epilogue multiplies the accumulator by 2^-e; DGELU also reports its output's largest
// magnitude, the scale of the products that read it next.
//
// Tiling: 256 threads = 4 waves, workgroup tile TM x TN, K tile = 64.  X is read global -> registers as 16-byte
// vectors (two per 8-column chunk), split in registers (the MBConv squeeze-excite gate applied to the fp32 value
// first) and written as f16 head and remainder images into LDS; W's two planes go the same way without the split.
// Every LDS image has 128-byte rows; 16-byte chunk c of row r lives at chunk position c ^ ((r >> 1) & 7) (gemm2.hip's
// swizzle), so the fragment reads of 16 consecutive rows spread over all banks.  The next tile's global loads are
// issued before the current tile's MFMAs.  As in gemm.hip the MFMA runs "transposed" (filter rows = A operand,
// activation rows = B operand); the output tile then goes out through LDS in whole rows (the MaxViT GEMMs with
// N = 3C / 4C write far more than they read: with 64-byte pieces of 16 rows per store the forward took 117.2 ms, 109.6 now).
#include "common.h"

namespace {

constexpr int BK = 64;      // K elements per tile
constexpr int ROWB = 128;   // bytes per LDS row of one plane (64 f16)

__device__ __forceinline__ f32x4 mma_x2(const h2x8& a, const h2x8& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.lo, b.hi, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.lo, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.hi, c, 0, 0, 0);
}

__device__ __forceinline__ int swz(int row, int chunk) { return row * ROWB + ((chunk ^ ((row >> 1) & 7)) << 4); }

template <int TM, int TN, int WM, int WN, int EPI, bool GATED>
__global__ __launch_bounds__(256) void gemm_x2_kernel(const float* __restrict__ X, const f16_t* __restrict__ W,
                                                      const float* __restrict__ bias, const float* __restrict__ gamma,
                                                      const float* resid, float* out, int M, int N, int K,
                                                      const float* __restrict__ gate, int rows_per_alert,
                                                      const unsigned* __restrict__ xamax, unsigned* oamax) {
  constexpr int WTM = TM / WM, WTN = TN / WN;
  constexpr int MI = WTM / 16, NI = WTN / 16;
  constexpr int XCH = TM * 8 / 256, WCH = TN * 8 / 256;   // 8-element chunks per thread and K tile
  static_assert(WM * WN == 4 && XCH >= 1 && WCH >= 1 && MI >= 1 && NI >= 1, "tile/wave layout");

  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (TM + TN) * ROWB];
  unsigned char* Xh = smem;
  unsigned char* Xl = Xh + TM * ROWB;
  unsigned char* Wh = Xl + TM * ROWB;
  unsigned char* Wl = Wh + TN * ROWB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
  const f16_t* Wlo = W + (size_t)N * K;
  const int xe = split_exp(xamax);
  const float xs = ldexpf(1.f, xe), xu = ldexpf(1.f, -xe);   // exact powers of two (|xe| <= 100)

  float4 xr[XCH][2];
  float4 gr[GATED ? XCH : 1][2];
  uint4 wrh[WCH], wrl[WCH];
  auto gload = [&](int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
      const int c = tid + i * 256, row = c >> 3, kc = c & 7;
      const int gm = m0 + row, gk = k0 + kc * 8;
      const bool ok = gm < M && gk < K;   // (K % 8 == 0: a chunk is wholly inside or wholly outside)
      const float4* p = reinterpret_cast<const float4*>(X + (size_t)gm * K + gk);
      xr[i][0] = ok ? p[0] : make_float4(0.f, 0.f, 0.f, 0.f);
      xr[i][1] = ok ? p[1] : make_float4(0.f, 0.f, 0.f, 0.f);
      if (GATED) {   // the per-alert squeeze-excite gate of the row (its value scales X before the split)
        const float4* g = reinterpret_cast<const float4*>(gate + (size_t)(min(gm, M - 1) / rows_per_alert) * K + gk);
        gr[i][0] = ok ? g[0] : make_float4(0.f, 0.f, 0.f, 0.f);
        gr[i][1] = ok ? g[1] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int c = tid + i * 256, row = c >> 3, kc = c & 7;
      const int gn = n0 + row, gk = k0 + kc * 8;
      const bool ok = gn < N && gk < K;
      const size_t o = (size_t)gn * K + gk;
      wrh[i] = ok ? *reinterpret_cast<const uint4*>(W + o) : make_uint4(0, 0, 0, 0);
      wrl[i] = ok ? *reinterpret_cast<const uint4*>(Wlo + o) : make_uint4(0, 0, 0, 0);
    }
  };
  auto sstore = [&]() {
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
      const int c = tid + i * 256, row = c >> 3, kc = c & 7;
      float v[8] = {xr[i][0].x, xr[i][0].y, xr[i][0].z, xr[i][0].w, xr[i][1].x, xr[i][1].y, xr[i][1].z, xr[i][1].w};
      if (GATED) {
        const float g[8] = {gr[i][0].x, gr[i][0].y, gr[i][0].z, gr[i][0].w,
                            gr[i][1].x, gr[i][1].y, gr[i][1].z, gr[i][1].w};
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] *= g[q];
      }
      if (xe != 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] *= xs;
      }
      const h2x8 s = split8(v);
      const int o = swz(row, kc);
      *reinterpret_cast<f16x8*>(Xh + o) = s.hi;
      *reinterpret_cast<f16x8*>(Xl + o) = s.lo;
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int c = tid + i * 256, row = c >> 3, kc = c & 7;
      const int o = swz(row, kc);
      *reinterpret_cast<uint4*>(Wh + o) = wrh[i];
      *reinterpret_cast<uint4*>(Wl + o) = wrl[i];
    }
  };

  f32x4 acc[NI][MI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (K + BK - 1) / BK;
  const int lrow = lane & 15, lq = lane >> 4;
  gload(0);
  for (int kt = 0; kt < nk; ++kt) {
    sstore();
    __syncthreads();
    if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      h2x8 bfr[MI], afr[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int o = swz(wm * WTM + mi * 16 + lrow, ks * 4 + lq);
        bfr[mi].hi = *reinterpret_cast<const f16x8*>(Xh + o);
        bfr[mi].lo = *reinterpret_cast<const f16x8*>(Xl + o);
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int o = swz(wn * WTN + ni * 16 + lrow, ks * 4 + lq);
        afr[ni].hi = *reinterpret_cast<const f16x8*>(Wh + o);
        afr[ni].lo = *reinterpret_cast<const f16x8*>(Wl + o);
      }
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = mma_x2(afr[ni], bfr[mi], acc[ni][mi]);
    }
    __syncthreads();
  }

  // epilogue (gemm.hip's fp32 forms), staged through the now idle LDS so that HBM sees whole rows: the accumulators go
  // to an fp32 [TM][TN] image (16-byte slot s of row r at s ^ (r & XM): the 16 rows of a fragment hit 16 different
  // slots), then each thread finishes 4 consecutive channels of a row per pass, TN * 4 contiguous bytes per row
  constexpr int SL = TN / 4;                  // 16-byte slots per image row
  constexpr int XM = (SL < 16 ? SL : 16) - 1;
  static_assert(TM * TN * 4 <= 2 * (TM + TN) * ROWB && 256 % SL == 0, "epilogue image");
  float* T = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int r = wm * WTM + mi * 16 + lrow, sl = (wn * WTN + ni * 16) / 4 + lq;
      *reinterpret_cast<f32x4*>(T + r * TN + ((sl ^ (r & XM)) << 2)) = acc[ni][mi];
    }
  __syncthreads();
  const int j = tid % SL, n = n0 + 4 * j;
  const bool live = n < N;
  constexpr bool NOBIAS = GATED || EPI == EPI_DGELU || EPI == EPI_PLAIN;
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!NOBIAS && live) bv = *reinterpret_cast<const float4*>(bias + n);
  float4 gv = make_float4(1.f, 1.f, 1.f, 1.f);
  if (EPI == EPI_RESID && !GATED && live) gv = *reinterpret_cast<const float4*>(gamma + n);
  float omax = 0.f;
#pragma unroll 4
  for (int r = tid / SL; r < TM && live; r += 256 / SL) {
    const int m = m0 + r;
    if (m >= M) break;
    const float4 a = *reinterpret_cast<const float4*>(T + r * TN + ((j ^ (r & XM)) << 2));
    const size_t o = (size_t)m * N + n;
    float4 v;
    if (EPI == EPI_GELU) {
      v = make_float4(gelu_erf(a.x + bv.x), gelu_erf(a.y + bv.y), gelu_erf(a.z + bv.z), gelu_erf(a.w + bv.w));
    } else if (EPI == EPI_SILU) {
      v = make_float4(silu_f(a.x + bv.x), silu_f(a.y + bv.y), silu_f(a.z + bv.z), silu_f(a.w + bv.w));
    } else if (EPI == EPI_RESID) {
      const float4 rv = *reinterpret_cast<const float4*>(resid + o);
      v.x = rv.x + gv.x * (a.x + bv.x);
      v.y = rv.y + gv.y * (a.y + bv.y);
      v.z = rv.z + gv.z * (a.z + bv.z);
      v.w = rv.w + gv.w * (a.w + bv.w);
    } else if (EPI == EPI_GELU_SAVE) {   // the fp32 pre-activation to resid, its GELU to out (gemm.hip)
      const float4 pre = make_float4(a.x + bv.x, a.y + bv.y, a.z + bv.z, a.w + bv.w);
      *reinterpret_cast<float4*>(const_cast<float*>(resid) + o) = pre;
      v = make_float4(gelu_erf(pre.x), gelu_erf(pre.y), gelu_erf(pre.z), gelu_erf(pre.w));
    } else if (EPI == EPI_DGELU) {      // out = acc * gelu'(pre), pre = the saved fp32 pre-activation
      const float4 pre = *reinterpret_cast<const float4*>(resid + o);
      v = make_float4(a.x * xu * gelu_grad(pre.x), a.y * xu * gelu_grad(pre.y), a.z * xu * gelu_grad(pre.z),
                      a.w * xu * gelu_grad(pre.w));
      omax = fmaxf(omax, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    } else if (EPI == EPI_PLAIN) {
      v = make_float4(a.x * xu, a.y * xu, a.z * xu, a.w * xu);
    } else {   // EPI_BIAS, EPI_BIAS_T
      v = make_float4(a.x + bv.x, a.y + bv.y, a.z + bv.z, a.w + bv.w);
    }
    *reinterpret_cast<float4*>(out + o) = v;
  }
  if (EPI == EPI_DGELU && oamax != nullptr) wave_amax(oamax, omax);   // (every lane of every wave gets here)
}

template <int TM, int TN, int WM, int WN, int EPI, bool GATED>
int launch_tile(const float* x, const f16_t* w, const float* bias, const float* gamma, const float* resid, float* out,
                int M, int N, int K, const float* gate, int rpa, hipStream_t st, const unsigned* xamax = nullptr,
                unsigned* oamax = nullptr) {
  dim3 grid((M + TM - 1) / TM, (N + TN - 1) / TN);
  hipLaunchKernelGGL((gemm_x2_kernel<TM, TN, WM, WN, EPI, GATED>), grid, dim3(256), 0, st, x, w, bias, gamma, resid,
                     out, M, N, K, gate, rpa, xamax, oamax);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

// Tile choice: 128 x 128 where that still gives the 256 CUs a few workgroups each, 128 x 64 / 128 x 32 for the
// narrow filters (stem, shortcut, stage-0 qkv-less GEMMs), 64 x 64 for the short late-stage maps.
template <int EPI, bool GATED>
int launch_shape(const float* x, const f16_t* w, const float* bias, const float* gamma, const float* resid, float* out,
                 int M, int N, int K, const float* gate, int rpa, hipStream_t st, const unsigned* xa = nullptr,
                 unsigned* oa = nullptr) {
  const long wg128 = (long)((M + 127) / 128) * ((N + 127) / 128);
  const long wg12864 = (long)((M + 127) / 128) * ((N + 63) / 64);
  if (N <= 32) return launch_tile<128, 32, 4, 1, EPI, GATED>(x, w, bias, gamma, resid, out, M, N, K, gate, rpa, st, xa, oa);
  if (N >= 128 && wg128 >= 512)
    return launch_tile<128, 128, 2, 2, EPI, GATED>(x, w, bias, gamma, resid, out, M, N, K, gate, rpa, st, xa, oa);
  if (wg12864 >= 512 || N < 64)
    return launch_tile<128, 64, 4, 1, EPI, GATED>(x, w, bias, gamma, resid, out, M, N, K, gate, rpa, st, xa, oa);
  return launch_tile<64, 64, 2, 2, EPI, GATED>(x, w, bias, gamma, resid, out, M, N, K, gate, rpa, st, xa, oa);
}

int check_shape(const char* who, int M, int N, int K) {
  if (K % 8 != 0 || N % 4 != 0 || K < 8 || N < 4) {
    btsbot_set_error("%s: K=%d must be a positive multiple of 8 and N=%d of 4", who, K, N);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((N + 31) / 32 > 65535 || (long)(M + 63) / 64 > 0x7fffffffL) {
    btsbot_set_error("%s: grid too large (M=%d N=%d)", who, M, N);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

}  // namespace

int launch_gemm_x2(int epi, const float* X, const void* W, const float* bias, const float* gamma, const float* resid,
                   float* out, int M, int N, int K, hipStream_t st) {
  if (epi == EPI_GELU_SAVE || epi == EPI_DGELU || epi == EPI_PLAIN) {
    btsbot_set_error("launch_gemm_x2: epilogue %d is a training one (launch_gemm_x2_train)", epi);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_gemm_x2_train(epi, X, W, bias, gamma, resid, out, M, N, K, nullptr, nullptr, st);
}

int launch_gemm_x2_train(int epi, const float* X, const void* W, const float* bias, const float* gamma, const float* resid,
                         float* out, int M, int N, int K, const unsigned* xa, unsigned* oa, hipStream_t st) {
  if (M <= 0) return BTSBOT_OK;
  const int s = check_shape("launch_gemm_x2", M, N, K);
  if (s != BTSBOT_OK) return s;
  const f16_t* w = reinterpret_cast<const f16_t*>(W);
  switch (epi) {
    case EPI_GELU_SAVE: return launch_shape<EPI_GELU_SAVE, false>(X, w, bias, gamma, resid, out, M, N, K, nullptr, 1, st);
    case EPI_DGELU: return launch_shape<EPI_DGELU, false>(X, w, bias, gamma, resid, out, M, N, K, nullptr, 1, st, xa, oa);
    case EPI_PLAIN: return launch_shape<EPI_PLAIN, false>(X, w, bias, gamma, resid, out, M, N, K, nullptr, 1, st, xa);
    case EPI_GELU: return launch_shape<EPI_GELU, false>(X, w, bias, gamma, resid, out, M, N, K, nullptr, 1, st);
    case EPI_RESID: return launch_shape<EPI_RESID, false>(X, w, bias, gamma, resid, out, M, N, K, nullptr, 1, st);
    case EPI_BIAS: return launch_shape<EPI_BIAS, false>(X, w, bias, gamma, resid, out, M, N, K, nullptr, 1, st);
    case EPI_SILU: return launch_shape<EPI_SILU, false>(X, w, bias, gamma, resid, out, M, N, K, nullptr, 1, st);
    case EPI_BIAS_T: return launch_shape<EPI_BIAS_T, false>(X, w, bias, gamma, resid, out, M, N, K, nullptr, 1, st);
  }
  btsbot_set_error("launch_gemm_x2: epilogue %d has no split-operand form", epi);
  return BTSBOT_ERR_INVALID_ARG;
}

int launch_gemm_x2_gated(const float* X, const float* gate, int rows_per_alert, const void* W, const float* resid,
                         float* out, int M, int N, int K, hipStream_t st) {
  if (M <= 0) return BTSBOT_OK;
  const int s = check_shape("launch_gemm_x2_gated", M, N, K);
  if (s != BTSBOT_OK) return s;
  if (rows_per_alert < 1) {
    btsbot_set_error("launch_gemm_x2_gated: rows_per_alert=%d", rows_per_alert);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_shape<EPI_RESID, true>(X, reinterpret_cast<const f16_t*>(W), nullptr, nullptr, resid, out, M, N, K,
                                       gate, rows_per_alert, st);
}
