// Fused classifier heads (fp32): optional head LayerNorm on the 1x1 image feature, metadata branch
// (BatchNorm1d folded to scale/shift -> Linear -> act -> Linear [-> act]), concat (image first, then
// metadata), fusion MLP, logits + sigmoid scores -- one kernel; the logits leave the CU and, where the caller asks
// for them (btsbot_forward_embed), the two embedding rows: `features`, the concat row, and `hidden`, the input of
// the last layer.
//
// Reference wiring: /root/reference/btsbot/architectures.py:146-171 (mm_ConvNeXt, GELU),
// :109-122 (ConvNeXt head), :282-293 (um_nn, ReLU), :299-313,358-372 (frozen_fusion, ReLU, metadata
// branch without its trailing activation); sigmoid: inference_example.py:91.
#include "common.h"

namespace {

constexpr int HG = 8;     // alerts per workgroup
constexpr int HNT = 512;   // threads (1024 would cap VGPRs at 128 and spill)
constexpr float HN_EPS = 1e-6f;
constexpr int PARTN = 2048;   // cross-slice scratch: KS * N <= PARTN rows of HG floats (64 KB)

// Activations of the workgroup's HG alerts live in LDS k-major: v[k][g] (8 alerts = two float4),
// so one thread reads all alerts of a k with two ds_read_b128 broadcasts.
// out[n][g] = act(bias[n] + sum_k in[k][g] * wt[k][n]); wt is K-major.  The head is a chain of small
// dependent layers, i.e. latency-bound, so the layout aims at few dependent memory round trips:
//   * a thread owns NPT = 4 consecutive neurons (one float4 weight load per k) of one K slice;
//     the HNT threads cover N/4 quads x KS slices, KS <= 16 so the cross-slice sum stays short;
//   * two groups of 8 k are in flight per thread (a slice of <= 16 k issues every load up front);
//   * partial sums meet in LDS (`part`), biases are fetched before the K loop.
// N not a multiple of 4 (the final N = 1 layer) takes the scalar path with the same structure.
template <int NPT>
__device__ __forceinline__ void dense_t(const float* in, int K, const float* __restrict__ wt,
                                        const float* __restrict__ bias, int N, int act, float* outp,
                                        float* part) {
  constexpr int GK = 8;
  typedef float __attribute__((ext_vector_type(NPT))) wvec;
  const int nq = N / NPT;                              // neuron groups
  int ks = 1;
  while (ks * 2 * nq <= HNT && ks * 2 * N <= PARTN && ks < 16 && K / (ks * 2) >= 8) ks *= 2;
  const int kchunk = (K + ks - 1) / ks;
  for (int q0 = 0; q0 < nq; q0 += HNT) {               // nq > HNT: several passes (ks == 1)
    const int q = q0 + (threadIdx.x % (nq < HNT ? nq : HNT));
    const int slice = nq < HNT ? threadIdx.x / nq : 0;
    const bool live = q < nq && slice < ks;
    const int fin = threadIdx.x;                       // element of [N][HG] finalised by this thread
    const float bfin = fin < HG * N ? bias[fin / HG] : 0.f;
    float acc[NPT][HG];
#pragma unroll
    for (int j = 0; j < NPT; ++j)
#pragma unroll
      for (int g = 0; g < HG; ++g) acc[j][g] = 0.f;
    if (live) {
      const int k0 = slice * kchunk, k1 = min(K, k0 + kchunk);
      const int ngrp = k1 > k0 ? (k1 - k0 + GK - 1) / GK : 0;
      const float* wp = wt + (size_t)q * NPT;
      wvec wa[GK], wb[GK];
      auto ld = [&](int kk) {
        return kk < k1 ? *reinterpret_cast<const wvec*>(wp + (size_t)kk * N) : wvec(0.f);
      };
      if (ngrp > 0) {
#pragma unroll
        for (int u = 0; u < GK; ++u) wa[u] = ld(k0 + u);
      }
      if (ngrp > 1) {
#pragma unroll
        for (int u = 0; u < GK; ++u) wb[u] = ld(k0 + GK + u);
      }
      for (int gi = 0; gi < ngrp; ++gi) {
        const int kb = k0 + gi * GK;
#pragma unroll
        for (int u = 0; u < GK; ++u) {
          const int kk = min(kb + u, k1 - 1);          // padded taps carry weight 0
          const float4 a0 = *reinterpret_cast<const float4*>(in + kk * HG);
          const float4 a1 = *reinterpret_cast<const float4*>(in + kk * HG + 4);
#pragma unroll
          for (int j = 0; j < NPT; ++j) {
            const float w = wa[u][j];
            acc[j][0] = fmaf(a0.x, w, acc[j][0]); acc[j][1] = fmaf(a0.y, w, acc[j][1]);
            acc[j][2] = fmaf(a0.z, w, acc[j][2]); acc[j][3] = fmaf(a0.w, w, acc[j][3]);
            acc[j][4] = fmaf(a1.x, w, acc[j][4]); acc[j][5] = fmaf(a1.y, w, acc[j][5]);
            acc[j][6] = fmaf(a1.z, w, acc[j][6]); acc[j][7] = fmaf(a1.w, w, acc[j][7]);
          }
        }
#pragma unroll
        for (int u = 0; u < GK; ++u) wa[u] = wb[u];
        if (gi + 2 < ngrp) {
          const int kn = k0 + (gi + 2) * GK;
#pragma unroll
          for (int u = 0; u < GK; ++u) wb[u] = ld(kn + u);
        }
      }
#pragma unroll
      for (int j = 0; j < NPT; ++j)
#pragma unroll
        for (int g = 0; g < HG; ++g) part[((size_t)slice * N + q * NPT + j) * HG + g] = acc[j][g];
    }
    __syncthreads();
    for (int i = fin; i < HG * N; i += HNT) {
      float t = i == fin ? bfin : bias[i / HG];
      for (int s2 = 0; s2 < ks; ++s2) t += part[s2 * N * HG + i];
      outp[i] = apply_act(t, act);
    }
  }
}

__device__ __forceinline__ void dense(const float* in, int K, const float* __restrict__ wt,
                                      const float* __restrict__ bias, int N, int act, float* outp,
                                      float* part, bool skipk = false) {
  if (skipk) K = 0;
  if ((N & 3) == 0)
    dense_t<4>(in, K, wt, bias, N, act, outp, part);
  else
    dense_t<1>(in, K, wt, bias, N, act, outp, part);
}

// Embedding output: v[n][HG] (k-major LDS rows) -> dst[b0 + g][n] for the `rows` live alerts of the workgroup (the
// padded alerts of the last workgroup hold duplicates of alert B - 1 and are never written).  A lane owns 4
// consecutive k of one alert and stores them as one float4; a wave's 64 lanes are 8 alerts x 8 quads, 128
// contiguous bytes per alert row.  The four reads of a lane are ds_read_b32 at dwords 32 q + 8 j + g (32 banks, 32
// lanes per group): taken in the order j every quad of an alert would meet on one bank (4-way), so quad q starts at
// j = q & 3 -- the group's 8 alerts x 4 quads then cover the 32 banks once -- and the lane turns its four values
// back.  Widths that are not a multiple of 4, or a destination off 16 bytes, take dword stores, k along the lanes.
__device__ __forceinline__ void store_rows(const float* v, int n, float* __restrict__ dst, int b0, int rows) {
  static_assert(HG == 8, "store_rows: 8 alerts per k");
  if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const int nq = n >> 2;
    for (int i = threadIdx.x; i < HG * nq; i += HNT) {
      const int g = i & (HG - 1), q = i >> 3, rot = q & 3;
      float t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] = v[(4 * q + ((j + rot) & 3)) * HG + g];   // t[j] = element (j + rot) & 3
      float4 o;
      o.x = rot == 0 ? t[0] : rot == 1 ? t[3] : rot == 2 ? t[2] : t[1];
      o.y = rot == 0 ? t[1] : rot == 1 ? t[0] : rot == 2 ? t[3] : t[2];
      o.z = rot == 0 ? t[2] : rot == 1 ? t[1] : rot == 2 ? t[0] : t[3];
      o.w = rot == 0 ? t[3] : rot == 1 ? t[2] : rot == 2 ? t[1] : t[0];
      if (g < rows) *reinterpret_cast<float4*>(dst + (size_t)(b0 + g) * n + 4 * q) = o;
    }
  } else {
    for (int i = threadIdx.x; i < rows * n; i += HNT) {
      const int g = i / n, k = i - g * n;
      dst[(size_t)(b0 + g) * n + k] = v[k * HG + g];
    }
  }
}

__global__ __launch_bounds__(HNT) void head_kernel(HeadArgs a) {
  static_assert(HG == 8, "dense() reads the 8 alerts of a k as two float4");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int zd = a.dims[0];
  int maxw = a.f1 > a.n_meta ? a.f1 : a.n_meta;
  for (int i = 1; i <= a.n_layers; ++i) maxw = a.dims[i] > maxw ? a.dims[i] : maxw;
  float* z = smem;               // [zd][HG]
  float* t0 = z + HG * zd;       // [maxw][HG]
  float* t1 = t0 + HG * maxw;    // [maxw][HG]
  float* part = t1 + HG * maxw;  // [KS][N][HG], KS * N <= PARTN
  const int b0 = blockIdx.x * HG;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ---- image feature (+ head LayerNorm) -> z[0:feat_dim][g]
  if (a.feat_dim > 0 && !(a.diag & 1)) {
    for (int g = wave; g < HG; g += HNT / 64) {
      const int b = b0 + g;
      const float* src = a.feat + (size_t)(b < a.B ? b : a.B - 1) * a.feat_dim;
      if (a.hn_w != nullptr) {
        float v[12];                                   // feat_dim <= 768: one load per value
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          const int c = lane + 64 * i;
          v[i] = c < a.feat_dim ? src[c] : 0.f;
          sum += v[i];
        }
        const float mean = wave_sum(sum) / a.feat_dim;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          const float d = lane + 64 * i < a.feat_dim ? v[i] - mean : 0.f;
          sq += d * d;
        }
        const float rstd = rsqrtf(wave_sum(sq) / a.feat_dim + HN_EPS);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
          const int c = lane + 64 * i;
          if (c < a.feat_dim) z[c * HG + g] = (v[i] - mean) * rstd * a.hn_w[c] + a.hn_b[c];
        }
      } else {
        for (int c = lane; c < a.feat_dim; c += 64) z[c * HG + g] = src[c];
      }
    }
  }
  // ---- metadata branch -> z[feat_dim : feat_dim + f2][g]
  if (a.n_meta > 0 && !(a.diag & 2)) {
    for (int i = tid; i < HG * a.n_meta; i += HNT) {
      const int g = i / a.n_meta, j = i - g * a.n_meta;
      const int b = b0 + g;
      const float v = a.meta[(size_t)(b < a.B ? b : a.B - 1) * a.n_meta + j];
      t0[j * HG + g] = fmaf(v, a.bn_scale[j], a.bn_shift[j]);
    }
    __syncthreads();
    dense(t0, a.n_meta, a.m1_wt, a.m1_b, a.f1, a.meta_act, t1, part, a.diag & 16);
    __syncthreads();
    dense(t1, a.f1, a.m2_wt, a.m2_b, a.f2, a.meta_trailing_act ? a.meta_act : ACT_NONE,
          z + a.feat_dim * HG, part, a.diag & 16);
  }
  __syncthreads();
  const int live = min(HG, a.B - b0);   // alerts of this workgroup that exist
  if (a.features != nullptr) store_rows(z, zd, a.features, b0, live);
  // ---- fusion MLP
  const float* in = z;
  float* bufs[2] = {t0, t1};
  for (int i = 0; i < a.n_layers; ++i) {
    float* o = bufs[i & 1];
    if (a.hidden != nullptr && i + 1 == a.n_layers) store_rows(in, a.dims[i], a.hidden, b0, live);
    if ((i == 0 && (a.diag & 4)) || (i > 0 && (a.diag & 8))) { in = o; continue; }
    dense(in, a.dims[i], a.wt[i], a.b[i], a.dims[i + 1],
          i + 1 < a.n_layers ? a.comb_act : ACT_NONE, o, part, a.diag & 16);
    __syncthreads();
    in = o;
  }
  if (tid < HG && b0 + tid < a.B) {
    const float zz = in[tid];
    a.logits[b0 + tid] = zz;
    if (a.scores != nullptr) a.scores[b0 + tid] = 1.0f / (1.0f + expf(-zz));
  }
}

}  // namespace

int launch_head(const HeadArgs& a, hipStream_t st) {
  if (a.diag != 0 && (a.features != nullptr || a.hidden != nullptr)) {
    btsbot_set_error("head: embedding outputs with the timing diagnostics on (diag %d skips the layers that make them)", a.diag);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (a.B <= 0) return BTSBOT_OK;
  int maxw = a.f1 > a.n_meta ? a.f1 : a.n_meta;
  for (int i = 1; i <= a.n_layers; ++i) maxw = a.dims[i] > maxw ? a.dims[i] : maxw;
  const size_t lds = (size_t)HG * (a.dims[0] + 2 * maxw + PARTN) * sizeof(float);
  if (a.feat_dim > 768) {
    btsbot_set_error("head: feature width %d above 768", a.feat_dim);
    return BTSBOT_ERR_INVALID_ARG;
  }
  int widest = a.f1 > a.f2 ? a.f1 : a.f2;   // (f2 lands in z, so maxw does not see it)
  widest = widest > maxw ? widest : maxw;
  if (widest > PARTN) {   // dense_t's `part` holds PARTN rows
    btsbot_set_error("head: layer width %d above %d", widest, PARTN);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (lds > 150 * 1024) {
    btsbot_set_error("head: layer widths too large for one workgroup (%zu bytes of LDS)", lds);
    return BTSBOT_ERR_INVALID_ARG;
  }
  static size_t lds_attr = 0;
  if (lds > lds_attr) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(head_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_attr = lds;
  }
  hipLaunchKernelGGL(head_kernel, dim3((a.B + HG - 1) / HG), dim3(HNT), lds, st, a);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
