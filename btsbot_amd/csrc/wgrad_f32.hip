// The filter-gradient GEMM on fp32 operands (gfx950): out[n][k] += sum_m D[m][n] * A[m][k], with the column sums of D
// (the bias gradient) beside it.  The fp32 training mode's form of what autograd does for nn.Linear / 1x1 Conv2d weight
// gradients; the 16-bit operands go through wgrad.hip, the split ones through wgrad_x2.hip.  Both kernels cut the
// reduction into slices that meet through fp32 atomics in the (pre-zeroed) gradient arena.
#include "mfma.h"

namespace {

// ---------------------------------------------------------------------------------------
// The fallback for shapes the matrix-pipe kernel below does not take (N or K no multiple of 64, operands off a 16-byte
// boundary), and the form BTSBOT_AMD_WGRAD_F32_OLD=1 keeps for every shape.
// wgrad: out[n][k] += sum_m D[m][n] * A[m][k]   (D: [M][N], A: [M][K], both row-major, fp32)
// Workgroup = 64x64 output tile x one slice of M; 4 waves in 2x2, each a 32x32 sub-tile.
// Both operands are "reduction-major" in memory, so fragments are gathered from row-major LDS
// tiles, one float per lane and 16x16x4 product (lane (i, g) takes row g of column i).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wgrad_f32_fallback_kernel(const float* __restrict__ D,
                                                                 const float* __restrict__ A,
                                                                 float* __restrict__ out, int M, int N, int K,
                                                                 int ldo, int mslice) {
  using MM = Mfma<float>;
  constexpr int KR = 4;                  // reduction depth per MFMA
  constexpr int TM = 64;                 // rows of the reduction dimension per LDS tile
  constexpr int PITCH = 64 + 8;          // elements per LDS row (padded)
  __shared__ float Ds[TM * PITCH];
  __shared__ float As[TM * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  const int n0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
  const int mbeg = blockIdx.z * mslice, mend = min(M, mbeg + mslice);
  const int li = lane & 15, lg = lane >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int m0 = mbeg; m0 < mend; m0 += TM) {
    // stage [64 m][64 n] of D and [64 m][64 k] of A (zero-filled at the edges)
    for (int i = tid; i < TM * 64; i += 256) {
      const int r = i >> 6, c = i & 63;
      const int m = m0 + r;
      Ds[r * PITCH + c] = (m < mend && n0 + c < N) ? D[(size_t)m * N + n0 + c] : 0.f;
      As[r * PITCH + c] = (m < mend && k0 + c < K) ? A[(size_t)m * K + k0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int ms = 0; ms < TM; ms += KR) {
      float af[2], bf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int cn = wn * 32 + t * 16 + li, ck = wk * 32 + t * 16 + li;
        af[t] = Ds[(ms + lg) * PITCH + cn];
        bf[t] = As[(ms + lg) * PITCH + ck];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = MM::m16(af[i], bf[j], acc[i][j]);
    }
    __syncthreads();
  }
  // C/D layout: col = lane&15 -> k, row = 4*(lane>>4)+r -> n
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn * 32 + i * 16 + lg * 4 + r;
        const int k = k0 + wk * 32 + j * 16 + li;
        if (n < N && k < K) atomicAdd(out + (size_t)n * ldo + k, acc[i][j][r]);
      }
}

// The same product for fp32 operands at the matrix pipe's fp32 rate (v_mfma_f32_32x32x2_f32: 256 FLOP per clock and CU).
// The kernel above stages 64 x 64 tiles element by element under a bounds test and ran the fp32 mode's 28 filter-gradient
// GEMMs per training step at 24 TFLOP/s -- 5.7 ms of a 10.5 ms step, on the side stream that bounds it.  Here: TN x TK
// output tile (64 or 128 each: one wave per 64 x 64), both operands in 16-row stages through LDS as 16-byte pieces, the
// next stage's loads in flight under the current stage's products (registers -> the other LDS buffer, one barrier per
// stage).  Both operands are reduction-major in memory, which is what the 32x32x2 fragments want: lane l reads element
// [m + (l >> 5)][base + (l & 31)] -- 32 consecutive floats per half wave.  N % TN == K % TK == 0 (the launcher picks).
template <int TN, int TK>
__global__ __launch_bounds__(64 * (TN / 64) * (TK / 64)) void wgrad_f32_kernel(const float* __restrict__ D,
                                                                                const float* __restrict__ A,
                                                                                float* __restrict__ out, int M, int N, int K,
                                                                                int ldo, int mslice, float* __restrict__ cs) {
  // cs != nullptr: cs[n] += sum_m D[m][n] as well (the bias gradient beside the filter gradient): the workgroups of the
  // first k-tile column add up the D rows they stage anyway -- was a launch of its own reading D once more (fp32 mode:
  // 32 launches, 1.9 ms of kernel time per training step)
  constexpr int WK = TK / 64, NTH = 64 * (TN / 64) * WK, TM = 16;
  constexpr int DV = TM * TN / 4, AV = TM * TK / 4;                 // 16-byte pieces per stage
  constexpr int DPT = (DV + NTH - 1) / NTH, APT = (AV + NTH - 1) / NTH;
  static_assert(DV % NTH == 0 && AV % NTH == 0, "whole pieces per thread");
  __shared__ __attribute__((aligned(16))) float Ds[2][TM * TN];
  __shared__ __attribute__((aligned(16))) float As[2][TM * TK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave / WK, wk = wave - wn * WK;
  const int n0 = blockIdx.x * TN, k0 = blockIdx.y * TK;
  const int mbeg = blockIdx.z * mslice, mend = min(M, mbeg + mslice);
  const int l31 = lane & 31, lh = lane >> 5;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float4 dr[DPT], ar[APT];
  const bool do_cs = cs != nullptr && blockIdx.y == 0;   // (uniform)
  float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);         // this thread's columns 4 (tid % (TN / 4)) .. + 3, its rows
  static_assert(NTH % (TN / 4) == 0, "a thread's pieces share their columns");
  auto fetch = [&](int m0) {
#pragma unroll
    for (int u = 0; u < DPT; ++u) {
      const int i = tid + u * NTH, r = i / (TN / 4), c = i - r * (TN / 4);
      dr[u] = m0 + r < mend ? *reinterpret_cast<const float4*>(D + (size_t)(m0 + r) * N + n0 + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < APT; ++u) {
      const int i = tid + u * NTH, r = i / (TK / 4), c = i - r * (TK / 4);
      ar[u] = m0 + r < mend ? *reinterpret_cast<const float4*>(A + (size_t)(m0 + r) * K + k0 + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto park = [&](int buf) {
#pragma unroll
    for (int u = 0; u < DPT; ++u) {
      reinterpret_cast<float4*>(Ds[buf])[tid + u * NTH] = dr[u];
      if (do_cs) {
        csum.x += dr[u].x;
        csum.y += dr[u].y;
        csum.z += dr[u].z;
        csum.w += dr[u].w;
      }
    }
#pragma unroll
    for (int u = 0; u < APT; ++u) reinterpret_cast<float4*>(As[buf])[tid + u * NTH] = ar[u];
  };
  if (mbeg < mend) {
    fetch(mbeg);
    park(0);
  }
  __syncthreads();
  int buf = 0;
  for (int m0 = mbeg; m0 < mend; m0 += TM) {
    const bool more = m0 + TM < mend;   // (uniform)
    if (more) fetch(m0 + TM);
    const float* ds = Ds[buf] + wn * 64 + l31;
    const float* as = As[buf] + wk * 64 + l31;
#pragma unroll
    for (int ms = 0; ms < TM; ms += 2) {
      float af[2], bf[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        af[t] = ds[(ms + lh) * TN + 32 * t];
        bf[t] = as[(ms + lh) * TK + 32 * t];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (more) park(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  // C/D layout of 32x32: column (lane & 31) -> k, register r -> row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> n
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + wn * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int k = k0 + wk * 64 + 32 * j + l31;
        atomicAdd(out + (size_t)n * ldo + k, acc[i][j][r]);
      }
  if (do_cs) {   // the row groups' column sums meet in LDS (the operand stages are dead: the loop ended on a barrier)
    constexpr int CG = TN / 4, RG = NTH / CG;
    float4* red = reinterpret_cast<float4*>(Ds[0]);
    static_assert(RG * CG * 16 <= (int)sizeof(Ds), "the partial sums fit the D stages");
    red[tid] = csum;   // [row group = tid / CG][column group = tid % CG]
    __syncthreads();
    if (tid < CG) {
      float4 t = red[tid];
#pragma unroll
      for (int g = 1; g < RG; ++g) {
        const float4 e = red[g * CG + tid];
        t.x += e.x;
        t.y += e.y;
        t.z += e.z;
        t.w += e.w;
      }
      float* d = cs + n0 + 4 * tid;
      atomicAdd(d, t.x);
      atomicAdd(d + 1, t.y);
      atomicAdd(d + 2, t.z);
      atomicAdd(d + 3, t.w);
    }
  }
}

// slices of the reduction: about target_wg workgroups over `tiles` output tiles, at least min_rows rows each, the slice
// length a multiple of `round` rows (the kernel's LDS stage); the last slice may be ragged
struct Slices { int nsl, mslice; };
inline Slices plan_slices(int tiles, int M, int target_wg, int min_rows, int round) {
  int nsl = (target_wg + tiles - 1) / tiles;
  if (nsl > (M + min_rows - 1) / min_rows) nsl = (M + min_rows - 1) / min_rows;
  if (nsl < 1) nsl = 1;
  const int mslice = ((M + nsl - 1) / nsl + round - 1) / round * round;
  return Slices{(M + mslice - 1) / mslice, mslice};
}

template <int TN, int TK>
int wgrad_f32_launch(const float* D, const float* A, float* out, int M, int N, int K, int ldo, hipStream_t st, float* cs) {
  // ~768 workgroups (two or three per CU), at least 256 rows each
  const Slices s = plan_slices((N / TN) * (K / TK), M, 768, 256, 16);
  hipLaunchKernelGGL((wgrad_f32_kernel<TN, TK>), dim3(N / TN, K / TK, s.nsl), dim3(64 * (TN / 64) * (TK / 64)), 0, st, D, A, out, M,
                     N, K, ldo, s.mslice, cs);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

// the matrix-pipe kernel where the shapes allow it; *cs_done says whether the column sums went along
int wgrad_f32(const float* D, const float* A, float* out, int M, int N, int K, int ldo, hipStream_t st, float* cs, bool* cs_done) {
  *cs_done = false;
  static const bool old_form = switch_on(SW_WGRAD_F32_OLD);   // 1: the 64 x 64 kernel for every shape (A/B timing, parity)
  const bool aligned = ((reinterpret_cast<uintptr_t>(D) | reinterpret_cast<uintptr_t>(A)) & 15) == 0;
  if (!old_form && aligned && N % 64 == 0 && K % 64 == 0) {
    // (deterministic mode: the column sums keep their own launch with its fixed-order reduction)
    float* csk = cs != nullptr && det_alloc(0) == nullptr ? cs : nullptr;
    if (csk != nullptr) *cs_done = true;
    const bool n128 = N % 128 == 0, k128 = K % 128 == 0;
    if (n128 && k128) return wgrad_f32_launch<128, 128>(D, A, out, M, N, K, ldo, st, csk);
    if (n128) return wgrad_f32_launch<128, 64>(D, A, out, M, N, K, ldo, st, csk);
    if (k128) return wgrad_f32_launch<64, 128>(D, A, out, M, N, K, ldo, st, csk);
    return wgrad_f32_launch<64, 64>(D, A, out, M, N, K, ldo, st, csk);
  }
  // enough workgroups to fill the chip, at least 512 rows each
  const dim3 tiles((N + 63) / 64, (K + 63) / 64);
  const Slices s = plan_slices((int)(tiles.x * tiles.y), M, 1024, 512, 64);
  hipLaunchKernelGGL(wgrad_f32_fallback_kernel, dim3(tiles.x, tiles.y, s.nsl), dim3(256), 0, st, D, A, out, M, N, K, ldo, s.mslice);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

}  // namespace

// fp32 operands: filter gradient and (cs != nullptr) the column sums of D, in one launch where the matrix-pipe kernel applies
int launch_wgrad_cs_f32(const float* D, const float* A, float* out, float* cs, int M, int N, int K, int ldo, hipStream_t st) {
  if (M <= 0) return BTSBOT_OK;
  bool done = false;
  const int rc = wgrad_f32(D, A, out, M, N, K, ldo, st, cs, &done);
  if (rc != BTSBOT_OK || cs == nullptr || done) return rc;
  return launch_colsum(BTSBOT_F32, D, cs, M, N, st);
}
