// The packed operand images of a ConvNeXt / metadata / fusion handle (btsbot_ctx::extra): image_walk() is the one list of
// them, pack_layout() reserves their slots, pack_params() writes them (btsbot_pack_params / btsbot_pack_params_train).
// Also the generic packing kernels: casts (plain, scaled per column or row, the stem's im2col), transposes, the downsample
// re-orderings and the job table that runs them as one launch.  The packers tied to one stage kernel's fragment layout live in that kernel's file.
// (A MaxViT image branch lays out and packs its own images: maxvit.hip.)
#include "ctx.h"
#include "head16.h"
#include "maxvit.h"
#include "stage3.h"

namespace {

template <typename T>
__global__ void cast_kernel(const float* __restrict__ s, T* __restrict__ d, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    d[i] = (T)s[i];
}

// four values per thread (16-byte loads, 8-byte stores): the scalar form moved 2 TB/s on the 10-100 MB operands the
// 16-bit MaxViT training casts per GEMM
template <typename T>
__global__ void cast4_kernel(const float4* __restrict__ s, T* __restrict__ d, int64_t n4) {
  typedef __attribute__((ext_vector_type(4))) T t4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = s[i];
    *reinterpret_cast<t4*>(d + 4 * i) = t4{(T)v.x, (T)v.y, (T)v.z, (T)v.w};
  }
}

__global__ void transpose_kernel(const float* __restrict__ s, float* __restrict__ d, int R, int Cc) {
  const int64_t n = (int64_t)R * Cc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i / R), r = (int)(i - (int64_t)c * R);  // d[c][r]
    d[i] = s[(int64_t)r * Cc + c];
  }
}

template <typename T>
__global__ void pack_down_kernel(const float* __restrict__ s, T* __restrict__ d, int Cout, int Cin) {
  const int64_t n = (int64_t)Cout * Cin * 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    // d[co][q][ci] <- s[co][ci][q],  q = ky*2 + kx
    const int ci = (int)(i % Cin);
    const int q = (int)((i / Cin) & 3);
    const int co = (int)(i / (4 * (int64_t)Cin));
    d[i] = (T)s[((int64_t)co * Cin + ci) * 4 + q];
  }
}

// split mode: the same order as pack_down_kernel, f16 heads in dh and f16 remainders in dl
__global__ void pack_down_split_kernel(const float* __restrict__ s, f16_t* __restrict__ dh, f16_t* __restrict__ dl,
                                       int Cout, int Cin) {
  const int64_t n = (int64_t)Cout * Cin * 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin);
    const int q = (int)((i / Cin) & 3);
    const int co = (int)(i / (4 * (int64_t)Cin));
    f16_t hi, lo;
    split_f16(s[((int64_t)co * Cin + ci) * 4 + q], hi, lo);
    dh[i] = hi;
    dl[i] = lo;
  }
}

template <typename T>
__global__ void transpose_cast_kernel(const float* __restrict__ s, const float* __restrict__ rowscale,
                                      T* __restrict__ d, int R, int Cc) {
  const int64_t n = (int64_t)R * Cc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i / R), r = (int)(i - (int64_t)c * R);  // d[c][r]
    d[i] = (T)(s[(int64_t)r * Cc + c] * (rowscale != nullptr ? rowscale[r] : 1.f));
  }
}

// downsample filter [Cout][Cin][2][2] fp32 -> [(q*Cin + ci)][Cout] (the dgrad GEMM's "W" operand)
template <typename T>
__global__ void pack_down_t_kernel(const float* __restrict__ s, T* __restrict__ d, int Cout, int Cin) {
  const int64_t n = (int64_t)Cout * Cin * 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cout);
    const int k = (int)(i / Cout);          // q*Cin + ci
    const int q = k / Cin, ci = k - q * Cin;
    d[i] = (T)s[((int64_t)co * Cin + ci) * 4 + q];
  }
}

// (g is the accumulator of the filter-gradient GEMM in front: read exactly once here and left zero for its next user)
__global__ void unpack_down_grad_kernel(float* __restrict__ g, float* __restrict__ d, int Cout,
                                        int Cin) {
  const int64_t n = (int64_t)Cout * Cin * 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(i & 3);
    const int ci = (int)((i >> 2) % Cin);
    const int co = (int)(i / (4 * (int64_t)Cin));
    const int64_t j = ((int64_t)co * 4 + q) * Cin + ci;
    d[i] = g[j];                                     // d[co][ci][q] = g[co][q][ci]
    g[j] = 0.f;
  }
}

__global__ void bn_fold_kernel(const float* w, const float* b, const float* rm, const float* rv,
                               float* scale, float* shift, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float s = w[i] / sqrtf(rv[i] + 1e-5f);
    scale[i] = s;
    shift[i] = b[i] - rm[i] * s;
  }
}

// the five element maps above behind one launch: see PackJob in launchers.h
template <typename T>
__global__ __launch_bounds__(256) void pack_jobs_kernel(const PackJob* __restrict__ jobs, int njobs) {
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {   // last job whose first block is <= this block (uniform: scalar loads)
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const PackJob jb = jobs[lo];
  const int nblk = (lo + 1 < njobs ? jobs[lo + 1].blk0 : (int)gridDim.x) - jb.blk0;
  const float* __restrict__ s = jb.src;
  const int R = jb.R, Cc = jb.Cc;
  const int64_t n = jb.op == PACK_DOWN || jb.op == PACK_DOWN_T || jb.op == PACK_FRAG_DOWN ? (int64_t)R * Cc * 4 : (int64_t)R * Cc;
  const int64_t i0 = (int64_t)((int)blockIdx.x - jb.blk0) * 256 + threadIdx.x, step = (int64_t)nblk * 256;
  switch (jb.op) {
    case PACK_CAST: {
      T* d = reinterpret_cast<T*>(jb.dst);
      for (int64_t i = i0; i < n; i += step) d[i] = (T)s[i];
      break;
    }
    case PACK_TRANSPOSE_F32: {
      float* d = reinterpret_cast<float*>(jb.dst);
      for (int64_t i = i0; i < n; i += step) {
        const int c = (int)(i / R), r = (int)(i - (int64_t)c * R);
        d[i] = s[(int64_t)r * Cc + c];
      }
      break;
    }
    case PACK_TRANSPOSE_CAST: {
      T* d = reinterpret_cast<T*>(jb.dst);
      for (int64_t i = i0; i < n; i += step) {
        const int c = (int)(i / R), r = (int)(i - (int64_t)c * R);
        d[i] = (T)(s[(int64_t)r * Cc + c] * (jb.scale != nullptr ? jb.scale[r] : 1.f));
      }
      break;
    }
    case PACK_TFRAG: {   // d = fragments of t[c][r] = s[r][c] * scale[r]: lane l of fragment (tile, k-step) holds t[16 tile + (l & 15)][32 k-step + 8 (l >> 4) + 0..7]
      T* d = reinterpret_cast<T*>(jb.dst);
      const int ksteps = R / 32;
      for (int64_t i = i0; i < n; i += step) {
        const int j = (int)(i & 7), l = (int)((i >> 3) & 63);
        const int64_t fs = i >> 9;
        const int ks = (int)(fs % ksteps), tile = (int)(fs / ksteps);
        const int c = 16 * tile + (l & 15), r = 32 * ks + 8 * (l >> 4) + j;
        d[i] = (T)(s[(int64_t)r * Cc + c] * (jb.scale != nullptr ? jb.scale[r] : 1.f));
      }
      break;
    }
    case PACK_FRAG:
    case PACK_FRAG_DOWN: {   // lane l of fragment (tile, k-step) holds w[16 tile + (l & 15)][32 k-step + 8 (l >> 4) + 0..7] (stage2p.hip: pack_frag_kernel)
      T* d = reinterpret_cast<T*>(jb.dst);
      const bool down = jb.op == PACK_FRAG_DOWN;
      const int K = down ? 4 * Cc : Cc, ksteps = K / 32;
      for (int64_t i = i0; i < n; i += step) {
        const int j = (int)(i & 7), l = (int)((i >> 3) & 63);
        const int64_t fs = i >> 9;
        const int ks = (int)(fs % ksteps), tile = (int)(fs / ksteps);
        const int row = 16 * tile + (l & 15), k = 32 * ks + 8 * (l >> 4) + j;
        float v;
        if (down) {
          const int q = k / Cc, c = k - q * Cc;
          v = s[((int64_t)row * Cc + c) * 4 + q];
        } else {
          v = s[(int64_t)row * K + k];
        }
        // (the product is rounded to fp32 BEFORE the conversion, as in stage2p.hip's pack_frag_kernel, which writes the same
        //  image in the full pack: left alone hipcc fuses the two into v_fma_mixlo_f16 -- one rounding instead of two, other
        //  bits in a few entries, and the first training step after a full pack would differ from the ones behind a re-pack)
        float pr = v * (jb.scale != nullptr ? jb.scale[row] : 1.f);
        asm volatile("" : "+v"(pr));
        d[i] = (T)pr;
      }
      break;
    }
    case PACK_DOWN: {   // d[co][q][ci] <- s[co][ci][q]
      T* d = reinterpret_cast<T*>(jb.dst);
      for (int64_t i = i0; i < n; i += step) {
        const int ci = (int)(i % Cc);
        const int q = (int)((i / Cc) & 3);
        const int co = (int)(i / (4 * (int64_t)Cc));
        d[i] = (T)s[((int64_t)co * Cc + ci) * 4 + q];
      }
      break;
    }
    default: {          // PACK_DOWN_T: d[q*Cin + ci][co] <- s[co][ci][q]
      T* d = reinterpret_cast<T*>(jb.dst);
      for (int64_t i = i0; i < n; i += step) {
        const int co = (int)(i % R);
        const int k = (int)(i / R);
        const int q = k / Cc, ci = k - q * Cc;
        d[i] = (T)s[((int64_t)co * Cc + ci) * 4 + q];
      }
    }
  }
}

// ---- operand casts of the training step and of the packs with a scale folded in

// out[m][c] = (T)(in[m][c] * scale[c])   (scale may be null)
template <typename T>
__global__ __launch_bounds__(256) void scale_cast_kernel(const float* __restrict__ in,
                                                         const float* __restrict__ scale,
                                                         T* __restrict__ out, long n, int C) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    out[i] = (T)(in[i] * (scale != nullptr ? scale[i % C] : 1.f));
}

// out[r][c] = (T)(in[r][c] * rowscale[r])
template <typename T>
__global__ __launch_bounds__(256) void rowscale_cast_kernel(const float* __restrict__ in,
                                                            const float* __restrict__ rowscale,
                                                            T* __restrict__ out, long n, int cols) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    out[i] = (T)(in[i] * rowscale[i / cols]);
}

template <typename T>
__global__ __launch_bounds__(256) void stem_im2col_kernel(const float* __restrict__ img,
                                                          T* __restrict__ patches, int B) {
  const long n = (long)B * 225 * 48;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int k = (int)(i % 48);
    const long r = i / 48;
    const int p = (int)(r % 225), b = (int)(r / 225);
    const int ci = k >> 4, ky = (k >> 2) & 3, kx = k & 3;
    const int py = p / 15, px = p - py * 15;
    patches[i] = (T)img[((size_t)b * 3 + ci) * 3969 + (4 * py + ky) * 63 + 4 * px + kx];
  }
}

inline int nblocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}
inline int gridn(long n) {   // (the casts above)
  long b = (n + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

// The by-precision ladder of the launchers below: launch(T* out) runs with `out` in the operand type of `prec`, and the
// launch is checked; any other `prec` is the error "<who>: bad precision".
template <typename Launch>
int by_prec(int prec, const char* who, void* out, Launch launch) {
  switch (prec) {
    case BTSBOT_F32: launch(reinterpret_cast<float*>(out)); break;
    case BTSBOT_BF16: launch(reinterpret_cast<bf16_t*>(out)); break;
    case BTSBOT_F16: launch(reinterpret_cast<f16_t*>(out)); break;
    default:
      btsbot_set_error("%s: bad precision %d", who, prec);
      return BTSBOT_ERR_INVALID_ARG;
  }
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
template <typename P> using pointee = typename std::remove_pointer<P>::type;

}  // namespace

int pack_job_blocks(const PackJob& j) {
  const int64_t n = (j.op == PACK_DOWN || j.op == PACK_DOWN_T || j.op == PACK_FRAG_DOWN ? 4 : 1) * (int64_t)j.R * j.Cc;
  const int64_t b = (n + 1023) / 1024;   // four elements per thread
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

int launch_pack_jobs(int prec, const PackJob* dev_jobs, int njobs, int total_blocks, hipStream_t st) {
  if (njobs <= 0) return BTSBOT_OK;
  return by_prec(prec, "pack_jobs", nullptr, [&](auto* d) {   // (every job brings its own destination)
    hipLaunchKernelGGL(pack_jobs_kernel<pointee<decltype(d)>>, dim3(total_blocks), dim3(256), 0, st, dev_jobs, njobs);
  });
}

int launch_cast(int prec, const float* src, void* dst, int64_t n, hipStream_t st) {
  if (n <= 0) return BTSBOT_OK;
  switch (prec) {
    case BTSBOT_F32:
      HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
      return BTSBOT_OK;
    case BTSBOT_BF16:
      if (n >= 4096 && n % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 8 == 0)
        hipLaunchKernelGGL(cast4_kernel<bf16_t>, dim3(nblocks(n / 4)), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(src), reinterpret_cast<bf16_t*>(dst), n / 4);
      else
      hipLaunchKernelGGL(cast_kernel<bf16_t>, dim3(nblocks(n)), dim3(256), 0, st, src,
                         reinterpret_cast<bf16_t*>(dst), n);
      break;
    case BTSBOT_F16:
      if (n >= 4096 && n % 4 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 8 == 0)
        hipLaunchKernelGGL(cast4_kernel<f16_t>, dim3(nblocks(n / 4)), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(src), reinterpret_cast<f16_t*>(dst), n / 4);
      else
      hipLaunchKernelGGL(cast_kernel<f16_t>, dim3(nblocks(n)), dim3(256), 0, st, src,
                         reinterpret_cast<f16_t*>(dst), n);
      break;
    default:
      btsbot_set_error("cast: bad precision %d", prec);
      return BTSBOT_ERR_INVALID_ARG;
  }
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int launch_transpose_f32(const float* src, float* dst, int R, int Cc, hipStream_t st) {
  hipLaunchKernelGGL(transpose_kernel, dim3(nblocks((int64_t)R * Cc)), dim3(256), 0, st, src, dst,
                     R, Cc);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int launch_pack_down(int prec, const float* src, void* dst, int Cout, int Cin, hipStream_t st) {
  const int64_t n = (int64_t)Cout * Cin * 4;
  return by_prec(prec, "pack_down", dst, [&](auto* d) {
    hipLaunchKernelGGL(pack_down_kernel<pointee<decltype(d)>>, dim3(nblocks(n)), dim3(256), 0, st, src, d, Cout, Cin);
  });
}

int launch_pack_down_split(const float* src, void* hi, void* lo, int Cout, int Cin, hipStream_t st) {
  const int64_t n = (int64_t)Cout * Cin * 4;
  hipLaunchKernelGGL(pack_down_split_kernel, dim3(nblocks(n)), dim3(256), 0, st, src, reinterpret_cast<f16_t*>(hi),
                     reinterpret_cast<f16_t*>(lo), Cout, Cin);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int launch_bn_fold(const float* w, const float* b, const float* rm, const float* rv, float* scale,
                   float* shift, int n, hipStream_t st) {
  hipLaunchKernelGGL(bn_fold_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w, b, rm, rv, scale,
                     shift, n);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

// dst[c][r] = src[r][c] * (rowscale ? rowscale[r] : 1)
int launch_transpose_cast(int prec, const float* src, const float* rowscale, void* dst, int R, int Cc,
                          hipStream_t st) {
  const int64_t n = (int64_t)R * Cc;
  return by_prec(prec, "transpose_cast", dst, [&](auto* d) {
    hipLaunchKernelGGL(transpose_cast_kernel<pointee<decltype(d)>>, dim3(nblocks(n)), dim3(256), 0, st, src, rowscale, d, R, Cc);
  });
}

int launch_scale_cast(int prec, const float* in, const float* scale, void* out, long n, int C,
                      hipStream_t st) {
  if (n <= 0) return BTSBOT_OK;
  return by_prec(prec, "scale_cast", out, [&](auto* o) {
    hipLaunchKernelGGL(scale_cast_kernel<pointee<decltype(o)>>, dim3(gridn(n)), dim3(256), 0, st, in, scale, o, n, C);
  });
}

int launch_rowscale_cast(int prec, const float* in, const float* rowscale, void* out, int rows,
                         int cols, hipStream_t st) {
  const long n = (long)rows * cols;
  if (n <= 0) return BTSBOT_OK;
  return by_prec(prec, "rowscale_cast", out, [&](auto* o) {
    hipLaunchKernelGGL(rowscale_cast_kernel<pointee<decltype(o)>>, dim3(gridn(n)), dim3(256), 0, st, in, rowscale, o, n, cols);
  });
}

__global__ __launch_bounds__(256) void rowscale_cast_lo_kernel(const float* __restrict__ in, const float* __restrict__ rowscale,
                                                              f16_t* __restrict__ out, long n, int cols) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = rowscale != nullptr ? in[i] * rowscale[i / cols] : in[i];
  const f16_t hi = (f16_t)v;
  out[i] = (f16_t)(v - (float)hi);
}

int launch_rowscale_cast_lo(const float* in, const float* rowscale, void* out, int rows, int cols, hipStream_t st) {
  const long n = (long)rows * cols;
  if (n <= 0) return BTSBOT_OK;
  hipLaunchKernelGGL(rowscale_cast_lo_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, rowscale,
                     reinterpret_cast<f16_t*>(out), n, cols);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int launch_stem_im2col(int prec, const float* img, void* patches, int B, hipStream_t st) {
  const long n = (long)B * 225 * 48;
  if (n <= 0) return BTSBOT_OK;
  return by_prec(prec, "stem_im2col", patches, [&](auto* p) {
    hipLaunchKernelGGL(stem_im2col_kernel<pointee<decltype(p)>>, dim3(gridn(n)), dim3(256), 0, st, img, p, B);
  });
}

int launch_unpack_down_grad(float* Gd, float* dst, int Cout, int Cin, hipStream_t st) {
  hipLaunchKernelGGL(unpack_down_grad_kernel, dim3(nblocks((int64_t)Cout * Cin * 4)), dim3(256), 0,
                     st, Gd, dst, Cout, Cin);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int launch_pack_down_t(int prec, const float* src, void* dst, int Cout, int Cin, hipStream_t st) {
  const int64_t n = (int64_t)Cout * Cin * 4;
  return by_prec(prec, "pack_down_t", dst, [&](auto* d) {
    hipLaunchKernelGGL(pack_down_t_kernel<pointee<decltype(d)>>, dim3(nblocks(n)), dim3(256), 0, st, src, d, Cout, Cin);
  });
}

// ---------------------------------------------------------------------------------------
// the image list
// ---------------------------------------------------------------------------------------
namespace {

// Every packed image of the handle, in the order the packs write them: stem, then per stage the downsample and the
// blocks, the split-training planes, metadata, fusion, head16.  THE place that decides that an image exists (an entry
// with bytes) and which packs write it (`when`), from the handle's resolved schedule (schedule.h): a stage kernel's images
// exist where that kernel runs.  The schedule is fixed from btsbot_create on, except train_split (btsbot_set_option,
// before the first pack) and train_packs (btsbot_reserve_train: pack_invalidate()), which only changes `when`.  An entry
// comes behind the image it reads.
void image_walk(btsbot_ctx* h) {
  const btsbot_config& c = h->cfg;
  const size_t esz = h->esz();
  const int prec = c.precision;
  const Schedule& sc = h->sched;
  const bool tp = sc.train_packs;
  const unsigned F = IN_FULL, FT = IN_FULL | IN_TRAIN, if_tp = tp ? FT : 0;
  std::vector<ImageEntry>& v = h->images;
  v.clear();
  // a PackJob of the batch table: dst = op(master[src] (x master[scale] per row)), [R][Cc]
  auto job = [&](const char* name, size_t* slot, size_t bytes, unsigned when, bool early, int op, int64_t src, int64_t scale,
                 int R, int Cc) -> ImageEntry& {
    v.push_back(ImageEntry{name, slot, bytes, when, early, nullptr, op, src, scale, R, Cc, 0, nullptr});
    return v.back();
  };
  // a dedicated packer (nullptr: the second output of the entry in front)
  auto own = [&](const char* name, size_t* slot, size_t bytes, unsigned when, bool early, const size_t* reads,
                 std::function<int(hipStream_t)> launch) {
    v.push_back(ImageEntry{name, slot, bytes, when, early, reads, -1, -1, -1, 0, 0, 0, std::move(launch)});
  };
  auto split = [&](const char* name, size_t* slot, const size_t* reads, long n) {
    v.push_back(ImageEntry{name, slot, (size_t)n * 4, if_tp, false, reads, -1, -1, -1, 0, 0, n, nullptr});
  };
  if (h->has_image && !h->is_maxvit) {
    const int c0 = c.dims[0];
    const bool x2_s0 = h->x2 && sc.stage0;
    // what stage0b_kernel's keeping form reads goes first in the training re-pack
    const bool early = sc.s0_keep;
    // stem filter in the operand type
    job("p_stem16", &h->p_stem16, (size_t)c0 * 48 * esz, sc.stage0 || tp ? FT : 0, early, PACK_CAST, h->stem_w, -1, c0 * 48, 1);
    if (x2_s0) {   // split mode: its f16 heads / remainders
      own("p_x2_stem", &h->p_x2_stem, (size_t)c0 * 48 * 2, F, false, nullptr, [=](hipStream_t st) {
        return launch_cast(BTSBOT_F16, h->mirror + h->stem_w, IMG(h, h->p_x2_stem), (int64_t)c0 * 48, st);
      });
      own("p_x2_stemlo", &h->p_x2_stemlo, (size_t)c0 * 48 * 2, F, false, nullptr, [=](hipStream_t st) {
        return launch_rowscale_cast_lo(h->mirror + h->stem_w, nullptr, IMG(h, h->p_x2_stemlo), c0, 48, st);
      });
    }
    for (int i = 0; i < 4; ++i) {
      const int ch = c.dims[i];
      const size_t wb = (size_t)4 * ch * ch;   // elements of a block's fc1 / fc2 filter
      if (i > 0) {
        DownPk* d = &h->down[i];
        const int cin = c.dims[i - 1];
        const size_t n = (size_t)ch * cin * 4;
        // (training re-pack with stage 2's forward through stage2p_kernel: the last downsample's fragments ride in the table)
        if (i == 3 && sc.stage2p)
          job("down.p_wp", &d->p_wp, n * esz, sc.s2_keep ? IN_TRAIN : 0, false, PACK_FRAG_DOWN, d->w, -1, ch, cin).launch =
              [=](hipStream_t st) {
                return launch_pack_s2p(h->prec_down3(), h->mirror + d->w, nullptr, IMG(h, d->p_wp), ch, 4 * cin, 1, cin, nullptr, st);
              };
        job("down.p_w", &d->p_w, n * esz, FT, early && i == 1, PACK_DOWN, d->w, -1, ch, cin);
        job("down.p_wt", &d->p_wt, n * esz, if_tp, false, PACK_DOWN_T, d->w, -1, ch, cin);
        if (i == 3 && sc.stage2p)   // ... and stage2p.hip's own packer writes them in the full pack
          own("down.p_wp", &d->p_wp, 0, F, false, nullptr, [=](hipStream_t st) {
            return launch_pack_s2p(h->prec_down3(), h->mirror + d->w, nullptr, IMG(h, d->p_wp), ch, 4 * cin, 1, cin, nullptr, st);
          });
        if (i == 2 && sc.stage1)
          own("down.p_wp", &d->p_wp, n * esz, sc.s1_keep ? FT : F, false, nullptr, [=](hipStream_t st) {
            return launch_pack_frag32(h->prec_s01(), h->mirror + d->w, IMG(h, d->p_wp), ch, cin, st);
          });
        if (i == 1 && x2_s0) {   // split mode, stage0b's downsample: heads and remainders from one launch
          own("down.p_x2_w", &d->p_x2_w, n * 2, F, false, nullptr, [=](hipStream_t st) {
            return launch_pack_down_split(h->mirror + d->w, IMG(h, d->p_x2_w), IMG(h, d->p_x2_wlo), ch, cin, st);
          });
          own("down.p_x2_wlo", &d->p_x2_wlo, n * 2, F, false, nullptr, nullptr);
        }
      }
      for (BlockPk& blk : h->blocks[i]) {
        BlockPk* b = &blk;
        const bool b_early = early && i == 0;
        job("p_dw", &b->p_dw, (size_t)49 * ch * 4, FT, b_early, PACK_TRANSPOSE_F32, b->dw_w, -1, ch, 49);
        job("p_fc1", &b->p_fc1, wb * esz, FT, b_early, PACK_CAST, b->fc1_w, -1, 4 * ch * ch, 1);
        job("p_fc2", &b->p_fc2, wb * esz, FT, false, PACK_CAST, b->fc2_w, -1, 4 * ch * ch, 1);
        const bool frag = (i == 2 && sc.stage2p) || (i == 3 && sc.stage3);   // stage2p.hip / stage3.hip: filters as MFMA A fragments
        if (i == 2 && sc.stage2p) {
          // (training re-pack with stage 2's forward through stage2p_kernel: its filters as MFMA fragments ride in the table,
          //  beside the row-major images the per-op forward reads -- large batches take that one, backbone_train.hip)
          const unsigned t = sc.s2_keep ? IN_TRAIN : 0;
          job("p_w1p", &b->p_w1p, wb * esz, t, false, PACK_FRAG, b->fc1_w, -1, 4 * ch, ch).launch = [=](hipStream_t st) {
            return launch_pack_s2p(h->prec_tail(), h->mirror + b->fc1_w, nullptr, IMG(h, b->p_w1p), 4 * ch, ch, 0, 0,
                                   reinterpret_cast<float*>(IMG(h, b->p_scales)), st);
          };
          job("p_w2p", &b->p_w2p, wb * esz, t, false, PACK_FRAG, b->fc2_w, b->gamma, ch, 4 * ch).launch = [=](hipStream_t st) {
            return launch_pack_s2p(h->prec_tail(), h->mirror + b->fc2_w, h->mirror + b->gamma, IMG(h, b->p_w2p), ch, 4 * ch, 0, 0,
                                   reinterpret_cast<float*>(IMG(h, b->p_scales)) + 2, st);
          };
        }
        // W1^T [C][4C] and (diag(gamma) W2)^T [4C][C] for the dgrad GEMMs
        job("p_fc1t", &b->p_fc1t, wb * esz, if_tp, false, PACK_TRANSPOSE_CAST, b->fc1_w, -1, 4 * ch, ch);
        job("p_fc2t", &b->p_fc2t, wb * esz, if_tp, false, PACK_TRANSPOSE_CAST, b->fc2_w, b->gamma, ch, 4 * ch);
        if (!h->x2 && s2mlp_bwd_supported(prec, ch)) {   // the same two as MFMA A fragments for s2mlp_bwd_kernel
          const unsigned t = tp && sc.s2mlp ? FT : 0;
          ImageEntry& e1 = job("p_w1tp", &b->p_w1tp, wb * 2, t, false, PACK_TFRAG, b->fc1_w, -1, 4 * ch, ch);
          e1.reads = &b->p_fc1t;   // (the single-operand launch; the table's job reads the mirror)
          e1.launch = [=](hipStream_t st) { return launch_pack_frag16(IMG(h, b->p_fc1t), IMG(h, b->p_w1tp), ch, 4 * ch, st); };
          ImageEntry& e2 = job("p_w2tp", &b->p_w2tp, wb * 2, t, false, PACK_TFRAG, b->fc2_w, b->gamma, ch, 4 * ch);
          e2.reads = &b->p_fc2t;
          e2.launch = [=](hipStream_t st) { return launch_pack_frag16(IMG(h, b->p_fc2t), IMG(h, b->p_w2tp), 4 * ch, ch, st); };
        }
        // diag(gamma) W2 in the operand type (the megakernels fold the layer scale); the training re-pack writes it for
        // the stages whose forward is a keeping form
        own("p_fc2g", &b->p_fc2g, wb * esz, F | ((i == 0 && sc.s0_keep) || (i == 1 && sc.s1_keep) ? IN_TRAIN : 0), b_early, nullptr,
            [=](hipStream_t st) {
              return launch_rowscale_cast(h->cfg.precision, h->mirror + b->fc2_w, h->mirror + b->gamma, IMG(h, b->p_fc2g), ch, 4 * ch, st);
            });
        // the same in f16 for stage0b.hip's bf16 inference form (stage 0 of an fp8 handle too), whose hidden type is f16
        if (i == 0 && sc.stage0 && h->prec_s01() == BTSBOT_BF16)
          own("p_fc2g_h", &b->p_fc2g_h, wb * 2, F, false, nullptr, [=](hipStream_t st) {
            return launch_rowscale_cast(BTSBOT_F16, h->mirror + b->fc2_w, h->mirror + b->gamma, IMG(h, b->p_fc2g_h), ch, 4 * ch, st);
          });
        if (frag) {
          const bool s3 = i == 3;   // (stage 2's two are reserved above, with their table jobs)
          own("p_scales", &b->p_scales, 64, 0, false, nullptr, nullptr);   // fp8 mode: {S1, 1/S1, S2, 1/S2}, written with the two below
          own("p_w1p", &b->p_w1p, s3 ? wb * esz : 0, F, false, nullptr, [=](hipStream_t st) {
            float* sc = reinterpret_cast<float*>(IMG(h, b->p_scales));
            const float* w = h->mirror + b->fc1_w;
            return s3 ? launch_pack_s3(h->prec_tail(), w, nullptr, IMG(h, b->p_w1p), 4 * ch, ch, 1, sc, st)
                      : launch_pack_s2p(h->prec_tail(), w, nullptr, IMG(h, b->p_w1p), 4 * ch, ch, 0, 0, sc, st);
          });
          own("p_w2p", &b->p_w2p, s3 ? wb * esz : 0, F, false, nullptr, [=](hipStream_t st) {
            float* sc = reinterpret_cast<float*>(IMG(h, b->p_scales)) + 2;
            const float *w = h->mirror + b->fc2_w, *g = h->mirror + b->gamma;
            return s3 ? launch_pack_s3(h->prec_tail(), w, g, IMG(h, b->p_w2p), ch, 4 * ch, 0, sc, st)
                      : launch_pack_s2p(h->prec_tail(), w, g, IMG(h, b->p_w2p), ch, 4 * ch, 0, 0, sc, st);
          });
        }
        // the parameter images of stage0b.hip / stage1b.hip (they read the tap-major taps) ...
        if (i == 1 && sc.stage1)
          own("p_s0par", &b->p_s0par, s1par_bytes(), F, false, &b->p_dw, [=](hipStream_t st) {
            const float* m = h->mirror;
            return launch_pack_s1par(h->prec_s01(), IMG_F32(h, b->p_dw), m + b->dw_b, m + b->ln_w, m + b->ln_b, IMG(h, b->p_s0par), st);
          });
        if (i == 0 && sc.stage0)
          own("p_s0par", &b->p_s0par, s0par_bytes(), F, false, &b->p_dw, [=](hipStream_t st) {
            const float* m = h->mirror;
            return launch_pack_s0par(h->prec_s01(), IMG_F32(h, b->p_dw), m + b->dw_b, m + b->ln_w, m + b->ln_b, m + b->fc1_b,
                                     m + b->fc2_b, m + b->gamma, IMG(h, b->p_s0par), st);
          });
        // ... and of their keeping forms (f16 taps in every mode), in the full pack too: the first training forward follows one
        if (i == 1 && sc.s1_keep)
          own("p_s0par_t", &b->p_s0par_t, s1par_bytes(), if_tp, false, &b->p_dw, [=](hipStream_t st) {
            const float* m = h->mirror;
            return launch_pack_s1par(BTSBOT_F16, IMG_F32(h, b->p_dw), m + b->dw_b, m + b->ln_w, m + b->ln_b, IMG(h, b->p_s0par_t), st);
          });
        if (i == 0 && sc.s0_keep)
          own("p_s0par_t", &b->p_s0par_t, s0par_bytes(), if_tp, b_early, &b->p_dw, [=](hipStream_t st) {
            const float* m = h->mirror;
            return launch_pack_s0par(BTSBOT_F16, IMG_F32(h, b->p_dw), m + b->dw_b, m + b->ln_w, m + b->ln_b, m + b->fc1_b,
                                     m + b->fc2_b, m + b->gamma, IMG(h, b->p_s0par_t), st);
          });
        if (h->x2 && ((i == 0 && sc.stage0) || (i == 1 && sc.stage1))) {   // split mode, stages 0-1: the pointwise filters as f16 heads + remainders
          own("p_x2_w1", &b->p_x2_w1, wb * 2, F, false, nullptr, [=](hipStream_t st) {
            return launch_cast(BTSBOT_F16, h->mirror + b->fc1_w, IMG(h, b->p_x2_w1), (int64_t)4 * ch * ch, st);
          });
          own("p_x2_w2g", &b->p_x2_w2g, wb * 2, F, false, nullptr, [=](hipStream_t st) {
            return launch_rowscale_cast(BTSBOT_F16, h->mirror + b->fc2_w, h->mirror + b->gamma, IMG(h, b->p_x2_w2g), ch, 4 * ch, st);
          });
          own("p_x2_w1lo", &b->p_x2_w1lo, wb * 2, F, false, nullptr, [=](hipStream_t st) {
            return launch_rowscale_cast_lo(h->mirror + b->fc1_w, nullptr, IMG(h, b->p_x2_w1lo), 4 * ch, ch, st);
          });
          own("p_x2_w2glo", &b->p_x2_w2glo, wb * 2, F, false, nullptr, [=](hipStream_t st) {
            return launch_rowscale_cast_lo(h->mirror + b->fc2_w, h->mirror + b->gamma, IMG(h, b->p_x2_w2glo), ch, 4 * ch, st);
          });
        }
        // (the training forward of the blocks whose backward is mlp_bwd_kernel runs the fused MLP too)
        if (sc.fused_mlp[i])
          own("p_fused", &b->p_fused, fused_mlp_packed_bytes(ch), sc.mlp_bwd[i] ? FT : F, false, nullptr, [=](hipStream_t st) {
            return launch_pack_fused_mlp(h->cfg.precision, ch, h->mirror + b->fc1_w, h->mirror + b->fc2_w, IMG(h, b->p_fused), st);
          });
      }
    }
    // split training ("train_split"): the f16 head + remainder planes of the fp32 images above, one launch behind them
    if (sc.train_split)
      for (int i = 0; i < 4; ++i) {
        const long ch = c.dims[i];
        if (i > 0) {
          split("down.p_s_w", &h->down[i].p_s_w, &h->down[i].p_w, ch * c.dims[i - 1] * 4);
          split("down.p_s_wt", &h->down[i].p_s_wt, &h->down[i].p_wt, ch * c.dims[i - 1] * 4);
        }
        for (BlockPk& b : h->blocks[i]) {
          split("p_s_fc1", &b.p_s_fc1, &b.p_fc1, 4 * ch * ch);
          split("p_s_fc2", &b.p_s_fc2, &b.p_fc2, 4 * ch * ch);
          split("p_s_fc1t", &b.p_s_fc1t, &b.p_fc1t, 4 * ch * ch);
          split("p_s_fc2t", &b.p_s_fc2t, &b.p_fc2t, 4 * ch * ch);
        }
      }
  }
  if (h->has_meta) {
    job("p_m1", &h->p_m1, (size_t)c.meta_fc1 * c.n_meta * 4, FT, false, PACK_TRANSPOSE_F32, h->m1_w, -1, c.meta_fc1, c.n_meta);
    job("p_m2", &h->p_m2, (size_t)c.meta_fc2 * c.meta_fc1 * 4, FT, false, PACK_TRANSPOSE_F32, h->m2_w, -1, c.meta_fc2, c.meta_fc1);
  }
  for (int i = 0; i < h->n_comb; ++i)
    job("p_comb", &h->p_comb[i], (size_t)h->comb_dims[i + 1] * h->comb_dims[i] * 4, FT, false, PACK_TRANSPOSE_F32, h->comb_w[i], -1,
        h->comb_dims[i + 1], h->comb_dims[i]);
  if (sc.head16) {   // head16.hip: the Linear filters as split A fragments
    auto h16 = [&](const char* name, size_t* slot, int64_t w, int N, int K) {
      own(name, slot, head16_packed_bytes(N, K), F, false, nullptr,
          [=](hipStream_t st) { return launch_pack_h16(h->prec_head(), h->mirror + w, IMG(h, *slot), N, K, st); });
    };
    if (h->has_meta) {
      h16("p_m1h", &h->p_m1h, h->m1_w, c.meta_fc1, c.n_meta);
      h16("p_m2h", &h->p_m2h, h->m2_w, c.meta_fc2, c.meta_fc1);
    }
    for (int i = 0; i < h->n_comb; ++i) h16("p_combh", &h->p_combh[i], h->comb_w[i], h->comb_dims[i + 1], h->comb_dims[i]);
  }
  if (h->has_meta) {   // BatchNorm1d folded to scale / shift, one launch
    own("p_bn_scale", &h->p_bn_scale, (size_t)c.n_meta * 4, FT, false, nullptr, [=](hipStream_t st) {
      const float* m = h->mirror;
      return launch_bn_fold(m + h->bn_w, m + h->bn_b, m + h->bn_rm, m + h->bn_rv, reinterpret_cast<float*>(IMG(h, h->p_bn_scale)),
                            reinterpret_cast<float*>(IMG(h, h->p_bn_shift)), h->cfg.n_meta, st);
    });
    own("p_bn_shift", &h->p_bn_shift, (size_t)c.n_meta * 4, FT, false, nullptr, nullptr);
  }
}

// the entry's image and the one it reads were laid out (layout and packing come from one list, so this cannot fail:
// it costs two comparisons and guards the list's order)
int entry_ok(const ImageEntry& e) {
  if (*e.slot == 0 || (e.reads != nullptr && *e.reads == 0)) {
    btsbot_set_error("pack: operand image %s %s", e.name, *e.slot == 0 ? "has no slot" : "reads an image listed behind it");
    return BTSBOT_ERR_STATE;
  }
  return BTSBOT_OK;
}

// BTSBOT_AMD_PACK_UNBATCHED=1: a table job as a launch of its own
int launch_job(const btsbot_ctx* h, const ImageEntry& e, hipStream_t st) {
  if (e.launch) return e.launch(st);
  const int prec = h->cfg.precision;
  const float* src = h->mirror + e.src;
  const float* scale = e.scale >= 0 ? h->mirror + e.scale : nullptr;
  void* dst = h->extra + *e.slot;
  switch (e.op) {
    case PACK_CAST: return launch_cast(prec, src, dst, e.R, st);
    case PACK_TRANSPOSE_F32: return launch_transpose_f32(src, reinterpret_cast<float*>(dst), e.R, e.Cc, st);
    case PACK_TRANSPOSE_CAST: return launch_transpose_cast(prec, src, scale, dst, e.R, e.Cc, st);
    case PACK_DOWN: return launch_pack_down(prec, src, dst, e.R, e.Cc, st);
    default: return launch_pack_down_t(prec, src, dst, e.R, e.Cc, st);
  }
}

// the device table of the jobs pack `kind` (0 full, 1 training re-pack) runs; the re-pack's early jobs go to table [2]
int build_job_tables(btsbot_ctx* h, int kind) {
  std::vector<PackJob> jobs[2];
  for (const ImageEntry& e : h->images) {
    if (e.op < 0 || !(e.when & (kind == 1 ? IN_TRAIN : IN_FULL))) continue;
    TRY(entry_ok(e));
    jobs[kind == 1 && e.early].push_back(PackJob{h->mirror + e.src, e.scale >= 0 ? h->mirror + e.scale : nullptr,
                                                 h->extra + *e.slot, e.R, e.Cc, e.op, 0});
  }
  for (int early = 0; early < 2; ++early) {
    std::vector<PackJob>& v = jobs[early];
    const int t = early ? 2 : kind;
    if (v.empty()) continue;
    int nb = 0;
    for (PackJob& j : v) {
      j.blk0 = nb;
      nb += pack_job_blocks(j);
    }
    HIP_TRY(hipMalloc(&h->pack_jobs[t], v.size() * sizeof(PackJob)));
    HIP_TRY(hipMemcpy(h->pack_jobs[t], v.data(), v.size() * sizeof(PackJob), hipMemcpyHostToDevice));
    h->pack_njobs[t] = (int)v.size();
    h->pack_blocks[t] = nb;
  }
  return BTSBOT_OK;
}

int launch_table(const btsbot_ctx* h, int t, hipStream_t st) {
  return launch_pack_jobs(h->cfg.precision, reinterpret_cast<const PackJob*>(h->pack_jobs[t]), h->pack_njobs[t], h->pack_blocks[t], st);
}

// every split plane the list holds, as one launch
int launch_split_planes(btsbot_ctx* h, hipStream_t st) {
  if (h->split_jobs == nullptr) {
    std::vector<SplitJob> sj;
    for (const ImageEntry& e : h->images)
      if (e.split_n > 0) {
        TRY(entry_ok(e));
        sj.push_back(SplitJob{reinterpret_cast<const float*>(h->extra + *e.reads), h->extra + *e.slot, e.split_n});
      }
    HIP_TRY(hipMalloc(&h->split_jobs, sj.size() * sizeof(SplitJob)));
    HIP_TRY(hipMemcpy(h->split_jobs, sj.data(), sj.size() * sizeof(SplitJob), hipMemcpyHostToDevice));
    h->split_njobs = (int)sj.size();
  }
  return launch_split_jobs(reinterpret_cast<const SplitJob*>(h->split_jobs), h->split_njobs, st);
}

void free_tables(btsbot_ctx* h) {
  for (int t = 0; t < 3; ++t) {
    if (h->pack_jobs[t]) (void)hipFree(h->pack_jobs[t]);
    h->pack_jobs[t] = nullptr;
    h->pack_njobs[t] = h->pack_blocks[t] = 0;
  }
  if (h->split_jobs) (void)hipFree(h->split_jobs);
  h->split_jobs = nullptr;
  h->split_njobs = 0;
}

}  // namespace

int pack_layout(btsbot_ctx* h) {
  image_walk(h);
  for (ImageEntry& e : h->images) *e.slot = 0;
  size_t cur = h->extra_fixed;
  for (ImageEntry& e : h->images) {
    if (e.bytes > 0) *e.slot = bump(cur, e.bytes);
    TRY(entry_ok(e));
  }
  h->extra_bytes = cur;
  return BTSBOT_OK;
}

int pack_invalidate(btsbot_ctx* h) {
  if (h->pack_jobs[0] || h->pack_jobs[1] || h->pack_jobs[2] || h->split_jobs) HIP_TRY(hipDeviceSynchronize());
  free_tables(h);
  h->packed = false;
  return pack_layout(h);   // (the same slots: no image's existence depends on what changes after the first pack)
}

void pack_release(btsbot_ctx* h) {
  free_tables(h);
  if (h->pack_early_ev) (void)hipEventDestroy(h->pack_early_ev);
  h->pack_early_ev = nullptr;
}

int pack_sync(btsbot_ctx* h, hipStream_t st) {
  if (!h->pack_on_side) return BTSBOT_OK;
  h->pack_on_side = false;
  h->pack_early = false;
  return side_join(h, st);
}
// `st` waits for the stem / stage-0 operand images only (the re-pack queues them first and records an event behind them);
// the rest of the re-pack runs on under the stage-0 megakernel and pack_sync() joins it in front of stage 1
int pack_sync_early(btsbot_ctx* h, hipStream_t st) {
  if (!h->pack_on_side) return BTSBOT_OK;
  if (!h->pack_early) return pack_sync(h, st);
  HIP_TRY(hipStreamWaitEvent(st, h->pack_early_ev, 0));
  return BTSBOT_OK;
}

// train_only: skip the operand images only the fused inference kernels read (gamma-scaled fc2 filters and
// their chunk-major form, the megakernels' parameter images, the fused-MLP image): the per-op training
// schedule (backbone_train.hip) and the backward never touch them, and they are re-packed after every
// optimiser step
int pack_params(btsbot_ctx* h, const float* master, hipStream_t st, bool train_only) {
  if (h == nullptr || master == nullptr) {
    btsbot_set_error("pack_params: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (h->mirror == nullptr) {  // first pack on this handle: allocate the operand arenas
    HIP_TRY(hipMalloc(&h->mirror, (size_t)h->total_floats * 4));
    HIP_TRY(hipMalloc(&h->extra, h->extra_bytes));
  }
  TRY(pack_sync(h, st));   // (a pack nobody consumed yet still reads the mirror on the side stream)
  TRY(launch_copy_f32(h->mirror, master, (size_t)h->total_floats, st));
  if (train_only && h->has_image && !h->is_maxvit && h->sched.side_stream && h->side != nullptr) {
    hipStream_t sp = st;
    TRY(side_fork(h, st, &sp));   // behind the mirror copy
    st = sp;
    h->pack_on_side = true;
  }
  // The plain element maps (casts, transposes, the downsample re-orderings) run as ONE launch over a job
  // table built on the first pack of each kind: mirror and extra never move, so the table is static.
  // BTSBOT_AMD_PACK_UNBATCHED=1 keeps one launch per operand (A/B and parity).
  static const bool unbatched = switch_on(SW_PACK_UNBATCHED);
  const int kind = train_only ? 1 : 0;
  const unsigned bit = train_only ? IN_TRAIN : IN_FULL;
  if (!unbatched && h->pack_jobs[kind] == nullptr) TRY(build_job_tables(h, kind));
  // training re-pack with the stage-0 megakernel in the forward (s0_keep): what it reads first -- its table, then the
  // stage-0 blocks' gamma-scaled fc2 filters and parameter images (they read the tap-major taps the table wrote), then the
  // event pack_sync_early() waits for
  const bool early = train_only && !unbatched && h->pack_jobs[2] != nullptr;
  h->pack_early = false;
  if (early) {
    TRY(launch_table(h, 2, st));
    for (const ImageEntry& e : h->images)
      if (e.early && (e.when & bit) && e.op < 0 && e.launch) {
        TRY(entry_ok(e));
        TRY(e.launch(st));
      }
    if (h->pack_early_ev == nullptr) HIP_TRY(hipEventCreateWithFlags(&h->pack_early_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->pack_early_ev, st));
    h->pack_early = true;
  }
  if (!unbatched) {
    TRY(launch_table(h, kind, st));
  } else {
    for (const ImageEntry& e : h->images)
      if (e.op >= 0 && (e.when & bit)) {
        TRY(entry_ok(e));
        TRY(launch_job(h, e, st));
      }
  }
  // ... then the images that read the packed taps or have maps of their own
  if (h->has_image && h->is_maxvit) TRY(maxvit_pack(h, st));
  bool split_done = false;
  for (const ImageEntry& e : h->images) {
    if (e.op >= 0 || !(e.when & bit) || (early && e.early)) continue;
    TRY(entry_ok(e));
    if (e.launch) {
      TRY(e.launch(st));
    } else if (e.split_n > 0 && !split_done) {
      TRY(launch_split_planes(h, st));
      split_done = true;
    }
  }
  h->packed = true;
  h->packed_full = !train_only || !h->has_image || h->is_maxvit;
  return BTSBOT_OK;
}
