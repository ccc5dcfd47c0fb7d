// Fixed-order reductions of the training step (gfx950): the scratch of the deterministic mode (det_begin / det_alloc: the
// partial rows kernels write through det_add, common.h), the kernel that adds those rows in order, and the column sum
// out[n] += sum_m in[m][n] that uses them.
#include "common.h"

// ---- deterministic mode: the scratch of the running backward call (thread-local: launchers run on the caller's thread)
namespace {
thread_local float* g_det_base = nullptr;
thread_local size_t g_det_cap = 0, g_det_used = 0;
thread_local bool g_det_short = false;   // a request did not fit the scratch: that reduction fell back to atomics

// 32 columns x 8 row groups per workgroup: group q adds rows q, q + 8, ... in order, the groups meet in LDS in order
__global__ __launch_bounds__(256) void det_reduce_kernel(const float* __restrict__ part, int nrows, int C, int W,
                                                         DetOut o0, DetOut o1, DetOut o2, DetOut o3) {
  __shared__ float sh[8][32];
  const int cl = threadIdx.x & 31, q = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (col < W)
    for (int r = q; r < nrows; r += 8) s += part[(size_t)r * W + col];
  sh[q][cl] = s;
  __syncthreads();
  if (q == 0 && col < W) {
    float t = sh[0][cl];
#pragma unroll
    for (int i = 1; i < 8; ++i) t += sh[i][cl];
    const int o = col / C, c = col - o * C;
    const DetOut d = o == 0 ? o0 : o == 1 ? o1 : o == 2 ? o2 : o3;
    d.ptr[(size_t)c * d.stride] += t;
  }
}

// out[n] += sum_m in[m][n].  Block = 64 columns x 4 row groups over one slice of M; the row groups
// meet in LDS so that every column costs ONE atomic per block (same-address atomics serialise).
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ in, float* out, int M,
                                                     int N, int mslice, float* part) {
  __shared__ float sh[4][64];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cl;
  const int mbeg = blockIdx.y * mslice, mend = min(M, mbeg + mslice);
  float s0 = 0.f, s1 = 0.f;
  if (n < N) {
    int m = mbeg + rg;
    for (; m + 4 < mend; m += 8) {
      s0 += (float)in[(size_t)m * N + n];
      s1 += (float)in[(size_t)(m + 4) * N + n];
    }
    if (m < mend) s0 += (float)in[(size_t)m * N + n];
  }
  sh[rg][cl] = s0 + s1;
  __syncthreads();
  if (rg == 0 && n < N) det_add(out + n, sh[0][cl] + sh[1][cl] + sh[2][cl] + sh[3][cl], part, (size_t)blockIdx.y * N + n);
}

template <typename T>
int colsum_t(const void* in, float* out, int M, int N, hipStream_t st) {
  const int nb = (N + 63) / 64;
  int nsl = (768 + nb - 1) / nb;                 // ~768 blocks in flight
  if (nsl > 64) nsl = 64;                        // ... but at most 64 atomics per column
  if (nsl > (M + 63) / 64) nsl = (M + 63) / 64;
  if (nsl < 1) nsl = 1;
  const int mslice = (M + nsl - 1) / nsl;
  dim3 grid(nb, (M + mslice - 1) / mslice);
  float* part = det_alloc((size_t)grid.y * N);
  hipLaunchKernelGGL(colsum_kernel<T>, grid, dim3(256), 0, st, reinterpret_cast<const T*>(in), out,
                     M, N, mslice, part);
  LAUNCH_CHECK();
  if (part != nullptr) {
    const DetOut o{out, 1};
    return launch_det_reduce(part, (int)grid.y, N, 1, &o, st);
  }
  return BTSBOT_OK;
}
}  // namespace

void det_begin(float* base, size_t floats) {
  g_det_base = base;
  g_det_cap = base != nullptr ? floats : 0;
  g_det_used = 0;
}
void det_end() { det_begin(nullptr, 0); }
bool det_fell_short() {   // since the last call: did any reduction of this thread's backward not fit the scratch?
  const bool v = g_det_short;
  g_det_short = false;
  return v;
}
float* det_alloc(size_t floats) {
  if (g_det_base == nullptr) return nullptr;
  if (g_det_used + floats > g_det_cap) {
    g_det_short = true;
    return nullptr;
  }
  float* p = g_det_base + g_det_used;
  g_det_used += (floats + 63) / 64 * 64;
  return p;
}
int launch_det_reduce(const float* part, int nrows, int C, int nout, const DetOut* outs, hipStream_t st) {
  if (nout < 1 || nout > 4) {
    btsbot_set_error("det_reduce: %d outputs", nout);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int W = nout * C;
  DetOut o[4] = {outs[0], outs[0], outs[0], outs[0]};
  for (int i = 0; i < nout; ++i) o[i] = outs[i];
  hipLaunchKernelGGL(det_reduce_kernel, dim3((W + 31) / 32), dim3(256), 0, st, part, nrows, C, W, o[0], o[1], o[2], o[3]);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int launch_colsum(int prec, const void* in, float* out, int M, int N, hipStream_t st) {
  if (M <= 0) return BTSBOT_OK;
  switch (prec) {
    case BTSBOT_F32: return colsum_t<float>(in, out, M, N, st);
    case BTSBOT_BF16: return colsum_t<bf16_t>(in, out, M, N, st);
    case BTSBOT_F16: return colsum_t<f16_t>(in, out, M, N, st);
  }
  btsbot_set_error("backward: bad precision %d", prec);
  return BTSBOT_ERR_INVALID_ARG;
}
