// Filter-gradient GEMM of the 1x1 convolutions on split operands (BTSBOT_F16X2 handles with "train_split", gfx950):
//
//   out[n][k] += sum_m D[m][n] * A[m][k]
//
// D = gradient w.r.t. the layer output [M pixels][N], A = the layer input [M][K], both fp32 and pixel-major (the
// reduction index outermost), as the fp32 training schedule keeps them.  wgrad.hip's form for 16-bit operands with the
// split of gemm_x2.hip in front: the fp32 tiles are read global -> registers as 16-byte vectors, D scaled by 2^e (device_math.h:
// split_exp of its largest magnitude -- gradients are small and their heads would be f16 subnormals), split into f16
// head and remainder images in LDS and read back with ds_read_b64_tr_b16, the transposing LDS read that hands a lane
// eight reduction-consecutive values of one output row / column.  Each product is lo*hi + hi*lo + hi*hi on
// v_mfma_f32_32x32x16_f16, small terms first.
//
// Workgroup = TN x TK output tile x one slice of M, 4 waves in 2 x 2, 64-row tiles; the next tile's global loads are in
// flight while the current one is multiplied (register-staged, one LDS image set: 4 images of 64 rows).  Slices leave as
// dense partial tiles, 2^-e applied (exact), and wgrad_reduce_kernel adds them in a fixed order -- no atomics whenever the
// caller lends the scratch, a single slice included.
#include "mfma.h"

namespace {

constexpr int TM = 64;   // reduction rows per LDS tile

// 4 fp32 values (times s) -> f16 heads and remainders at row r, 4-column chunk cc of the two images
__device__ __forceinline__ void put4(unsigned char* hi, unsigned char* lo, int off, float4 v, float s) {
  const float f[4] = {v.x * s, v.y * s, v.z * s, v.w * s};
  const h2x4 x = split4(f);
  *reinterpret_cast<f16x4v*>(hi + off) = x.hi;
  *reinterpret_cast<f16x4v*>(lo + off) = x.lo;
}

template <int TN, int TK>
__global__ __launch_bounds__(256) void wgrad_x2_kernel(const float* __restrict__ D, const float* __restrict__ A,
                                                       float* __restrict__ out, float* __restrict__ colsum,
                                                       float* __restrict__ cpart, int M, int N, int K, int ldo, int mslice,
                                                       float* __restrict__ part, const unsigned* __restrict__ damax,
                                                       const unsigned* __restrict__ aamax) {
  constexpr int PN = TN * 2 + 64, PK = TK * 2 + 64;      // row pitch of an f16 image in bytes (wgrad.hip's padding)
  constexpr int DB = TM * PN, AB = TM * PK;               // bytes per image
  constexpr int FN = TN / 64, FK = TK / 64;               // 32x32 fragments per wave
  constexpr int LN = TN * TM / 1024, LK = TK * TM / 1024; // 16-byte (4-float) chunks per thread per tile
  __shared__ __attribute__((aligned(16))) unsigned char sm[2 * (DB + AB)];
  unsigned char* dh = sm;
  unsigned char* dl = dh + DB;
  unsigned char* ah = dl + DB;
  unsigned char* al = ah + AB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  const int n0 = blockIdx.x * TN, k0 = blockIdx.y * TK;
  const int mbeg = blockIdx.z * mslice, mend = min(M, mbeg + mslice);
  const int nt = (mend - mbeg + TM - 1) / TM;
  const int de = split_exp(damax), ae = split_exp(aamax);
  const float ds = ldexpf(1.f, de), as = ldexpf(1.f, ae);
  // undone one factor after the other (|de|, |ae| <= 100: each factor is a normal float, where their product 2^-(de + ae)
  // could not be; each multiplication is exact while its result is a normal float)
  const float dud = ldexpf(1.f, -de), dua = ldexpf(1.f, -ae);
  // column sums of D (the first tile column only): a thread's chunks all hold the same four columns (256 % (TN / 4) == 0)
  const bool do_sum = colsum != nullptr && blockIdx.y == 0;
  float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);

  f32x16 acc[FN][FK];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FK; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 rd[LN], ra[LK];
  auto fetch = [&](int t) {
    const int m0 = mbeg + t * TM;
#pragma unroll
    for (int s = 0; s < LN; ++s) {
      const int q = tid + 256 * s, r = q / (TN / 4), cc = q % (TN / 4);
      const int m = m0 + r, n = n0 + 4 * cc;
      const bool ok = m < mend && n < N;
      const float4 v = *reinterpret_cast<const float4*>(D + (size_t)(ok ? m : mbeg) * N + (ok ? n : 0));
      rd[s] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int s = 0; s < LK; ++s) {
      const int q = tid + 256 * s, r = q / (TK / 4), cc = q % (TK / 4);
      const int m = m0 + r, k = k0 + 4 * cc;
      const bool ok = m < mend && k < K;
      const float4 v = *reinterpret_cast<const float4*>(A + (size_t)(ok ? m : mbeg) * K + (ok ? k : 0));
      ra[s] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int s = 0; s < LN; ++s) {
      const int q = tid + 256 * s, r = q / (TN / 4), cc = q % (TN / 4);
      put4(dh, dl, r * PN + cc * 8, rd[s], ds);
      if (do_sum) {
        csum.x += rd[s].x;
        csum.y += rd[s].y;
        csum.z += rd[s].z;
        csum.w += rd[s].w;
      }
    }
#pragma unroll
    for (int s = 0; s < LK; ++s) {
      const int q = tid + 256 * s, r = q / (TK / 4), cc = q % (TK / 4);
      put4(ah, al, r * PK + cc * 8, ra[s], as);
    }
  };

  if (nt > 0) fetch(0);
  for (int t = 0; t < nt; ++t) {
    stash();
    __syncthreads();
    if (t + 1 < nt) fetch(t + 1);   // (workgroup-uniform)
#pragma unroll
    for (int ms = 0; ms < TM; ms += 16) {
      s16x8 afh[FN], afl[FN], bfh[FK], bfl[FK];
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        afh[i] = tr_frag(dh, PN, ms, wn * (TN / 2) + 32 * i, lane);
        afl[i] = tr_frag(dl, PN, ms, wn * (TN / 2) + 32 * i, lane);
      }
#pragma unroll
      for (int j = 0; j < FK; ++j) {
        bfh[j] = tr_frag(ah, PK, ms, wk * (TK / 2) + 32 * j, lane);
        bfl[j] = tr_frag(al, PK, ms, wk * (TK / 2) + 32 * j, lane);
      }
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FK; ++j) {
          acc[i][j] = MfmaRaw<f16_t>::m32(afl[i], bfh[j], acc[i][j]);
          acc[i][j] = MfmaRaw<f16_t>::m32(afh[i], bfl[j], acc[i][j]);
          acc[i][j] = MfmaRaw<f16_t>::m32(afh[i], bfh[j], acc[i][j]);
        }
    }
    __syncthreads();
  }

  if (do_sum) {   // the threads of one column group meet in LDS in a fixed order (every tile read is behind the barrier)
    constexpr int CG = TN / 4, G = 256 / CG;
    float4* red = reinterpret_cast<float4*>(sm);
    red[tid] = csum;
    __syncthreads();
    if (tid < CG && n0 + 4 * tid < N) {
      float4 t = red[tid];
#pragma unroll
      for (int g2 = 1; g2 < G; ++g2) {
        const float4 v = red[tid + CG * g2];
        t.x += v.x;
        t.y += v.y;
        t.z += v.z;
        t.w += v.w;
      }
      const int n = n0 + 4 * tid;
      if (cpart != nullptr) {   // deterministic mode: one partial row per slice, launch_det_reduce adds them in order
        *reinterpret_cast<float4*>(cpart + (size_t)blockIdx.z * N + n) = t;
      } else {
        atomicAdd(colsum + n, t.x);
        atomicAdd(colsum + n + 1, t.y);
        atomicAdd(colsum + n + 2, t.z);
        atomicAdd(colsum + n + 3, t.w);
      }
    }
  }

  // C/D layout of 32x32: column = lane & 31 -> k, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> n
  const int lc = lane & 31, lh = lane >> 5;
  if (part != nullptr) {
    float* pt = part + ((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (TN * TK);
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FK; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int nl = wn * (TN / 2) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const int kl = wk * (TK / 2) + 32 * j + lc;
          pt[nl * TK + kl] = (acc[i][j][r] * dud) * dua;
        }
  } else {
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FK; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int n = n0 + wn * (TN / 2) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
          const int k = k0 + wk * (TK / 2) + 32 * j + lc;
          if (n < N && k < K) atomicAdd(out + (size_t)n * ldo + k, (acc[i][j][r] * dud) * dua);
        }
  }
}

template <int TN, int TK>
int wgrad_x2_launch(const float* D, const float* A, float* out, float* colsum, int M, int N, int K, int ldo, const unsigned* damax,
                    const unsigned* aamax, hipStream_t st, float* part, size_t part_floats, WgradReduceJob* defer) {
  const int gx = (N + TN - 1) / TN, gy = (K + TK - 1) / TK;
  // slices of the reduction as in wgrad.hip: ~384 workgroups of at least 256 rows (two-pass), 512 rows (atomics)
  int nsl = 1, mslice = M;
  auto slices = [&](int min_rows, int target_wg) {
    nsl = (target_wg + gx * gy - 1) / (gx * gy);
    if (nsl > (M + min_rows - 1) / min_rows) nsl = (M + min_rows - 1) / min_rows;
    if (nsl < 1) nsl = 1;
    mslice = ((M + nsl - 1) / nsl + TM - 1) / TM * TM;
    nsl = (M + mslice - 1) / mslice;
  };
  slices(256, 384);
  const bool two_pass = part != nullptr && (size_t)nsl * gx * gy * TN * TK <= part_floats;
  if (!two_pass) slices(512, 384);
  if (nsl > 65535) {
    btsbot_set_error("wgrad_x2: M=%d needs %d slices", M, nsl);
    return BTSBOT_ERR_INVALID_ARG;
  }
  float* cpart = colsum != nullptr ? det_alloc((size_t)nsl * N) : nullptr;
  hipLaunchKernelGGL((wgrad_x2_kernel<TN, TK>), dim3(gx, gy, nsl), dim3(256), 0, st, D, A, out, colsum, cpart, M, N, K,
                     ldo, mslice, two_pass ? part : nullptr, damax, aamax);
  LAUNCH_CHECK();
  if (cpart != nullptr) {
    const DetOut o{colsum, 1};
    TRY(launch_det_reduce(cpart, nsl, N, 1, &o, st));
  }
  WgradReduceJob job = {part, out, N, K, ldo, gx, gy, two_pass ? nsl : 0, TN, TK};
  if (defer != nullptr) {
    *defer = job;   // (nsl == 0: the slices met through atomics, nothing left to add)
    return BTSBOT_OK;
  }
  return launch_wgrad_reduce(&job, 1, st);
}

__global__ __launch_bounds__(256) void copy_amax_kernel(const float4* __restrict__ in, float4* __restrict__ out, long n4,
                                                        unsigned* amax) {
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 v = in[i];
    if (out != nullptr) out[i] = v;
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  }
  wave_amax(amax, m);
}

// one row of workgroups per job (blockIdx.y), each walking its job's elements
__global__ __launch_bounds__(256) void split_jobs_kernel(const SplitJob* __restrict__ jobs) {
  const SplitJob J = jobs[blockIdx.y];
  f16_t* hi = reinterpret_cast<f16_t*>(J.dst);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < J.n; i += (long)gridDim.x * 256) {
    _Float16 a, b;
    split_f16(J.src[i], a, b);
    hi[i] = a;
    hi[J.n + i] = b;
  }
}

}  // namespace

int launch_wgrad_x2(const float* D, const float* A, float* out, float* colsum, int M, int N, int K, int ldo, const unsigned* damax,
                    const unsigned* aamax, hipStream_t st, float* part, size_t part_floats, WgradReduceJob* defer) {
  if (defer != nullptr) defer->nsl = 0;
  if (M <= 0) return BTSBOT_OK;
  if ((N & 15) || (K & 15) || N < 16 || K < 16 || ((uintptr_t)D & 15) || ((uintptr_t)A & 15) || (N + 63) / 64 > 65535 ||
      (K + 63) / 64 > 65535) {
    btsbot_set_error("wgrad_x2: N=%d K=%d must be positive multiples of 16 and the operands 16-byte aligned", N, K);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (N > 64 && K > 64) return wgrad_x2_launch<128, 128>(D, A, out, colsum, M, N, K, ldo, damax, aamax, st, part, part_floats, defer);
  if (N > 64) return wgrad_x2_launch<128, 64>(D, A, out, colsum, M, N, K, ldo, damax, aamax, st, part, part_floats, defer);
  if (K > 64) return wgrad_x2_launch<64, 128>(D, A, out, colsum, M, N, K, ldo, damax, aamax, st, part, part_floats, defer);
  return wgrad_x2_launch<64, 64>(D, A, out, colsum, M, N, K, ldo, damax, aamax, st, part, part_floats, defer);
}

int launch_copy_amax(const float* in, float* out, long n, unsigned* amax, hipStream_t st) {
  if (n <= 0) return BTSBOT_OK;
  if ((n & 3) || ((uintptr_t)in & 15) || ((uintptr_t)out & 15)) {
    btsbot_set_error("copy_amax: n=%ld must be a multiple of 4 and the buffers 16-byte aligned", n);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const long n4 = n / 4;
  long g = (n4 + 255) / 256;
  if (g > 1024) g = 1024;   // (a grid-stride walk: one atomic per wave)
  hipLaunchKernelGGL(copy_amax_kernel, dim3((unsigned)g), dim3(256), 0, st, reinterpret_cast<const float4*>(in),
                     reinterpret_cast<float4*>(out), n4, amax);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int launch_split_jobs(const SplitJob* jobs_dev, int njobs, hipStream_t st) {
  if (njobs <= 0) return BTSBOT_OK;
  if (njobs > 65535) {
    btsbot_set_error("split_jobs: %d jobs", njobs);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(split_jobs_kernel, dim3(32, njobs), dim3(256), 0, st, jobs_dev);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
