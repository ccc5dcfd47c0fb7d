// Input gradient of the 4x4 / stride-4 patch stem: the last link of the chain from a logit back to the pixels.
//
//     d_img[b][c][4i+u][4j+v] = sum_o dxn[b][i][j][o] * W[o][c][u][v]        i, j < 15
//
// dxn [B*225][C0] fp32 is the gradient behind the stem convolution (what the stem LayerNorm's backward leaves in every
// precision mode), W [C0][3][4][4] the filter as the state dict holds it (the fp32 mirror), d_img [B][3][63][63] the layout
// of the triplets.  Rows and columns 60..62 are never read by the stem (15 patches of 4 cover 60 pixels): their
// gradient is +0.0f, written here like every other element -- each element of d_img exactly once, no atomics, no clear.
//
// One wave per (alert, patch row i): a [15 (+1 zero row)][C0] x [C0][48] product on v_mfma_f32_16x16x4_f32 -- three
// 16-column tiles (one per image channel: column = c*16 + u*4 + v), C0 / 4 steps, fp32 accumulation.  The reduction
// index may be walked in any order as long as A and B agree, so a lane loads its A operands as 16-byte pieces
// (k = 16 s + 4 (lane >> 4) + e, e = 0..3 of one float4) and the B operands follow the same order.  The filter is
// staged through LDS once per workgroup (row pitch 52 floats: the four reduction rows an MFMA's lanes read lie 16 banks
// apart) into registers, where it stays for every patch row the wave walks.  The result tile is turned in LDS (row
// pitch 68: the 64 lanes of one store hit 64 banks) so that the global stores run along image rows: the four rows
// 4i .. 4i+3 of a channel are 252 consecutive floats, written as four 256-byte pieces; patch row 14 appends the 189
// zeros of rows 60..62.  An image row starts at an odd float offset (63 is odd), so the stores are dwords.
#include "common.h"
#include "mfma.h"

namespace {

constexpr int WPITCH = 52, OPITCH = 68, WAVES = 4;

template <int C0>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const float* __restrict__ dxn, const float* __restrict__ w,
                                                         float* __restrict__ dimg, int ntask) {
  static_assert(C0 % 16 == 0, "a lane's A operands are whole float4 pieces");
  constexpr int S = C0 / 16;
  __shared__ float sW[C0 * WPITCH];
  __shared__ float sO[WAVES][12 * OPITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int q = tid; q < C0 * 12; q += 256) {
    const int o = q / 12, c4 = q - o * 12;
    *reinterpret_cast<float4*>(&sW[o * WPITCH + 4 * c4]) = *reinterpret_cast<const float4*>(w + o * 48 + 4 * c4);
  }
  __syncthreads();
  const int n = lane & 15, kq = lane >> 4;
  float bf[3][S][4];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int e = 0; e < 4; ++e) bf[t][s][e] = sW[(16 * s + 4 * kq + e) * WPITCH + 16 * t + n];
  float* so = sO[wave];
  // (every wave of the workgroup makes the same number of trips: the barriers below are workgroup-wide)
  for (int t0 = blockIdx.x * WAVES; t0 < ntask; t0 += gridDim.x * WAVES) {
    const int task = t0 + wave;
    const bool live = task < ntask;
    const int b = task / 15, i = task - b * 15;
    // A: lane (j = lane & 15, kq) holds dxn[b][i][j][16 s + 4 kq .. + 3]; row 15 is the zero pad
    float4 af[S];
    const float* ap = dxn + ((size_t)task * 15 + n) * C0 + 4 * kq;
#pragma unroll
    for (int s = 0; s < S; ++s)
      af[s] = live && n < 15 ? *reinterpret_cast<const float4*>(ap + 16 * s) : make_float4(0.f, 0.f, 0.f, 0.f);
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float a4[4] = {af[s].x, af[s].y, af[s].z, af[s].w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] = Mfma<float>::m16(a4[e], bf[t][s][e], acc[t]);
    }
    // D: lane holds column n = (u, v) of channel t, patch columns j = 4 kq + r  ->  so[t*4 + u][4 j + v]
    const int u = n >> 2, v = n & 3;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) so[(t * 4 + u) * OPITCH + 4 * (4 * kq + r) + v] = acc[t][r];
    __syncthreads();
    if (live) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* dst = dimg + ((size_t)(b * 3 + c) * 63 + 4 * i) * 63;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int idx = q * 64 + lane;
          const int y = idx / 63, x = idx - y * 63;
          if (idx < 252) dst[idx] = x < 60 ? so[(c * 4 + y) * OPITCH + x] : 0.f;
        }
        if (i == 14)   // rows 60..62 of the channel follow row 59 in memory
          for (int idx = lane; idx < 189; idx += 64) dst[252 + idx] = 0.f;
      }
    }
    __syncthreads();
  }
}

}  // namespace

int stem_dgrad_grid(int B) {
  const long tasks = (long)B * 15;
  const long wg = (tasks + WAVES - 1) / WAVES;
  return (int)(wg < 2048 ? wg : 2048);   // 8 workgroups per CU on 256 CUs; larger batches loop
}

int launch_stem_dgrad(const float* dxn, const float* w, float* dimg, int B, int C0, hipStream_t st) {
  if (B < 1) return BTSBOT_OK;
  if (C0 != 64 && C0 != 80) {
    btsbot_set_error("stem_dgrad: no kernel for a stem of %d channels (64 or 80)", C0);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((((uintptr_t)dxn | (uintptr_t)w) & 15) != 0) {
    btsbot_set_error("stem_dgrad: dxn and the filter must be 16-byte aligned");
    return BTSBOT_ERR_INVALID_ARG;
  }
  const dim3 grid(stem_dgrad_grid(B));
  if (C0 == 64) hipLaunchKernelGGL(stem_dgrad_kernel<64>, grid, dim3(256), 0, st, dxn, w, dimg, B * 15);
  else hipLaunchKernelGGL(stem_dgrad_kernel<80>, grid, dim3(256), 0, st, dxn, w, dimg, B * 15);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
