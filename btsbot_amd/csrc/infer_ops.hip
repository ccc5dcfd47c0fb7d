// Op-level entry points of the inference kernels (include/btsbot_hip.h, btsbot_op_*): one launcher at a time on the
// caller's tensors and stream, for the per-kernel tests.  Nothing here is on the product path.
#include <string.h>

#include "maxvit.h"
#include "stage2p.h"
#include "stage3.h"

extern "C" int btsbot_op_gemm(int prec, int epi, const void* X, const void* W, const float* bias,
                              const float* gamma, const float* resid, void* out, int M, int N,
                              int K, void* stream) {
  if (X == nullptr || W == nullptr || bias == nullptr || out == nullptr || M < 0 || N < 1 ||
      K < 1 || (epi == EPI_RESID && (gamma == nullptr || resid == nullptr))) {
    btsbot_set_error("op_gemm: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((epi == EPI_GELU_SAVE || epi == EPI_DGELU) && resid == nullptr) {   // (every precision: the pre-activation's buffer)
    btsbot_set_error("op_gemm: this epilogue needs resid (the pre-activation)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (prec == BTSBOT_F16X2) {   // fp32 X and W: W split into its f16 head and remainder planes here, stream-ordered
    hipStream_t st = (hipStream_t)stream;
    if (M == 0) return BTSBOT_OK;
    // (the training epilogues whose X is a gradient: X's largest magnitude sets its power-of-two scale, as in the step)
    const bool grad_x = epi == EPI_DGELU || epi == EPI_PLAIN;
    StreamScratch sc(st, "op_gemm");
    const size_t o_w = sc.reserve((size_t)N * K * 4), o_amax = sc.reserve(AMAX_WORDS * 4);   // both planes, then X's record
    TRY(sc.alloc());
    void* wsplit = sc.at(o_w);
    unsigned* xamax = grad_x ? sc.at<unsigned>(o_amax) : nullptr;
    const float* w = reinterpret_cast<const float*>(W);
    TRY(launch_cast(BTSBOT_F16, w, wsplit, (int64_t)N * K, st));
    TRY(launch_rowscale_cast_lo(w, nullptr, reinterpret_cast<f16_t*>(wsplit) + (size_t)N * K, N, K, st));
    if (grad_x) {
      HIP_TRY(hipMemsetAsync(xamax, 0, AMAX_WORDS * 4, st));
      TRY(launch_copy_amax(reinterpret_cast<const float*>(X), nullptr, (long)M * K, xamax, st));
    }
    return launch_gemm_x2_train(epi, reinterpret_cast<const float*>(X), wsplit, bias, gamma, resid,
                                reinterpret_cast<float*>(out), M, N, K, xamax, nullptr, st);
  }
  return launch_gemm(prec, epi, X, W, bias, gamma, resid, out, M, N, K, (hipStream_t)stream);
}

extern "C" int btsbot_op_wgrad(int prec, const void* Dv, const void* Av, float* out, float* colsum, int M, int N, int K,
                               void* stream) {
  if (Dv == nullptr || Av == nullptr || out == nullptr || M < 0 || N < 1 || K < 1) {
    btsbot_set_error("op_wgrad: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return BTSBOT_OK;
  if (prec == BTSBOT_BF16 || prec == BTSBOT_F16) {
    // 16-bit D and A, the training step's form: slice partials in a stream-ordered scratch + the two-pass reduction
    if ((N & 7) || (K & 7) || ((uintptr_t)Dv & 15) || ((uintptr_t)Av & 15)) {
      btsbot_set_error("op_wgrad: N=%d K=%d must be multiples of 8 and D, A 16-byte aligned", N, K);
      return BTSBOT_ERR_INVALID_ARG;
    }
    const size_t part_floats = (size_t)16 << 20;
    StreamScratch sc(st, "op_wgrad");
    const size_t o_part = sc.reserve(part_floats * 4);
    TRY(sc.alloc());
    return launch_wgrad16(prec, Dv, Av, out, colsum, M, N, K, K, st, sc.at<float>(o_part), part_floats);
  }
  const float* D = reinterpret_cast<const float*>(Dv);
  const float* A = reinterpret_cast<const float*>(Av);
  if (prec == BTSBOT_F32) return launch_wgrad_cs_f32(D, A, out, colsum, M, N, K, K, st);
  if (prec != BTSBOT_F16X2) {
    btsbot_set_error("op_wgrad: precision %d (BTSBOT_F32, BTSBOT_BF16, BTSBOT_F16 or BTSBOT_F16X2)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  // split operands as in the split training step's stem: the largest magnitudes of D and of A set their power-of-two
  // scales (for an O(1) A, as the other products of the step have, the scale changes nothing but the exponents); slice
  // partials + fixed-order sum
  if ((N & 15) || (K & 15)) {
    btsbot_set_error("op_wgrad: N=%d K=%d must be multiples of 16", N, K);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const size_t part_floats = (size_t)16 << 20;
  StreamScratch sc(st, "op_wgrad");
  const size_t o_part = sc.reserve(part_floats * 4), o_amax = sc.reserve(2 * AMAX_WORDS * 4);   // D's record, then A's
  TRY(sc.alloc());
  float* part = sc.at<float>(o_part);
  unsigned* damax = sc.at<unsigned>(o_amax);
  unsigned* aamax = damax + AMAX_WORDS;
  HIP_TRY(hipMemsetAsync(damax, 0, 2 * AMAX_WORDS * 4, st));
  TRY(launch_copy_amax(D, nullptr, (long)M * N, damax, st));
  TRY(launch_copy_amax(A, nullptr, (long)M * K, aamax, st));
  return launch_wgrad_x2(D, A, out, colsum, M, N, K, K, damax, aamax, st, part, part_floats, nullptr);
}

extern "C" int btsbot_op_gemm_gated(int prec, const void* X, const float* gate, int rows_per_alert, const void* W,
                                    const float* resid, float* out, int M, int N, int K, void* stream) {
  if (X == nullptr || gate == nullptr || W == nullptr || resid == nullptr || out == nullptr || M < 0 || N < 1 ||
      K < 1 || rows_per_alert < 1) {
    btsbot_set_error("op_gemm_gated: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return BTSBOT_OK;
  if (prec != BTSBOT_F16X2)
    return launch_gemm_gated(prec, X, gate, rows_per_alert, W, resid, out, M, N, K, st);
  // fp32 X and W: W split into its f16 head and remainder planes here, stream-ordered (as btsbot_op_gemm does)
  StreamScratch sc(st, "op_gemm_gated");
  const size_t o_w = sc.reserve((size_t)N * K * 4);
  TRY(sc.alloc());
  void* wsplit = sc.at(o_w);
  const float* w = reinterpret_cast<const float*>(W);
  TRY(launch_cast(BTSBOT_F16, w, wsplit, (int64_t)N * K, st));
  TRY(launch_rowscale_cast_lo(w, nullptr, reinterpret_cast<f16_t*>(wsplit) + (size_t)N * K, N, K, st));
  return launch_gemm_x2_gated(reinterpret_cast<const float*>(X), gate, rows_per_alert, wsplit, resid, out, M, N, K, st);
}

extern "C" int btsbot_op_gemm_resid_ln(int prec, const void* X, const void* W, const float* resid, float* out, int batch,
                                       int M, int N, int K, const float* ln_w, const float* ln_b, void* ln_out,
                                       void* stream) {
  if (X == nullptr || W == nullptr || resid == nullptr || out == nullptr || batch < 1 || M < 1 || N < 1 || K < 1 ||
      (ln_out != nullptr && (ln_w == nullptr || ln_b == nullptr))) {
    btsbot_set_error("op_gemm_resid_ln: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  // the kernel reads a bias and a layer scale; this form has neither: zeros and ones, stream-ordered
  StreamScratch sc(st, "op_gemm_resid_ln");
  const size_t o = sc.reserve((size_t)N * 8);
  TRY(sc.alloc());
  float* zero_bias = sc.at<float>(o);
  float* one_gamma = zero_bias + N;
  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(zero_bias), 0, N, st));
  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(one_gamma), 0x3f800000, N, st));   // 1.0f
  return launch_gemm2_batched_resid(prec, X, W, zero_bias, one_gamma, resid, out, batch, M, N, K, st, ln_w, ln_b, ln_out);
}

extern "C" int btsbot_op_dwconv_ln(int prec, const float* x, const float* w, const float* bias,
                                   const float* ln_w, const float* ln_b, void* xn, int B, int HW,
                                   int C, void* stream) {
  if (x == nullptr || w == nullptr || bias == nullptr || ln_w == nullptr || ln_b == nullptr ||
      xn == nullptr || B < 0) {
    btsbot_set_error("op_dwconv_ln: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_dwconv_ln(prec, x, w, bias, ln_w, ln_b, xn, B, HW, C, (hipStream_t)stream);
}

extern "C" int btsbot_op_stem(const float* img, const float* w, const float* bias,
                              const float* ln_w, const float* ln_b, float* out, int B, int C0,
                              void* stream) {
  if (img == nullptr || w == nullptr || bias == nullptr || ln_w == nullptr || ln_b == nullptr ||
      out == nullptr || B < 0) {
    btsbot_set_error("op_stem: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_stem(img, w, bias, ln_w, ln_b, out, B, C0, (hipStream_t)stream);
}

extern "C" int btsbot_op_ln_patch(int prec, const float* x, const float* ln_w, const float* ln_b,
                                  void* patches, int B, int HW, int Cin, void* stream) {
  if (x == nullptr || ln_w == nullptr || ln_b == nullptr || patches == nullptr || B < 0 ||
      HW < 2) {
    btsbot_set_error("op_ln_patch: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_ln_patch(prec, x, ln_w, ln_b, patches, B, HW, Cin, (hipStream_t)stream);
}

// ---- MaxViT kernels one at a time.  Parameters come in the state-dict layout (fp32); the operand images are built in a
// stream-ordered scratch by the pack launchers the handle uses (maxvit_pack), so those are exercised as well.
namespace {

bool mv_prec16(int prec) { return prec == BTSBOT_BF16 || prec == BTSBOT_F16; }
bool mv_prec_any(int prec) { return prec == BTSBOT_F32 || mv_prec16(prec); }

int mv_op_bad(const char* who, const char* what) {
  btsbot_set_error("%s: %s", who, what);
  return BTSBOT_ERR_INVALID_ARG;
}

}  // namespace

extern "C" int btsbot_op_mv_attn(int prec, int impl, const void* qkv, const float* table, void* out, int B, int H, int C,
                                 int grid_mode, void* stream) {
  if (qkv == nullptr || table == nullptr || out == nullptr) return mv_op_bad("op_mv_attn", "null pointer");
  if (B < 0 || H < 7 || H % 7 != 0 || C < 32 || C % 32 != 0 || (grid_mode != 0 && grid_mode != 1) || (impl != 0 && impl != 1)) {
    btsbot_set_error("op_mv_attn: bad shape B=%d H=%d C=%d grid_mode=%d impl=%d (H a multiple of 7, C of 32)", B, H, C,
                     grid_mode, impl);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (impl == 0 ? !mv_prec_any(prec) : !mv_prec16(prec)) {
    btsbot_set_error("op_mv_attn: precision %d (impl 0: BTSBOT_F32 / BF16 / F16; impl 1: BF16 / F16)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int heads = C / 32;
  if ((long)B * (H / 7) * (H / 7) * heads > 0x7fffffffL) return mv_op_bad("op_mv_attn", "too many (alert, partition, head) units");
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mv_attn");
  const size_t o_bias = sc.reserve((size_t)heads * (impl == 0 ? 2401 : 4096) * 4);
  TRY(sc.alloc());
  float* bias = sc.at<float>(o_bias);
  if (impl == 0) {
    TRY(launch_mv_pack_relbias(table, bias, heads, st));
    return launch_mv_attn(prec, qkv, bias, out, B, H, C, grid_mode, st);
  }
  TRY(launch_mv_pack_relbias64(table, bias, heads, st));
  return launch_mv_attn_mfma(prec, qkv, bias, out, B, H, C, grid_mode, st);
}

extern "C" int btsbot_op_mv_attn_block(int prec, const void* xn, float* x, void* xn2, const float* qkv_w, const float* qkv_b,
                                       const float* proj_w, const float* proj_b, const float* table, const float* ln2_w,
                                       const float* ln2_b, int B, int H, int grid_mode, void* stream) {
  if (xn == nullptr || x == nullptr || xn2 == nullptr || qkv_w == nullptr || qkv_b == nullptr || proj_w == nullptr ||
      proj_b == nullptr || table == nullptr || ln2_w == nullptr || ln2_b == nullptr)
    return mv_op_bad("op_mv_attn_block", "null pointer");
  if (B < 0 || H < 7 || H % 7 != 0 || (grid_mode != 0 && grid_mode != 1)) {
    btsbot_set_error("op_mv_attn_block: bad shape B=%d H=%d grid_mode=%d (H a multiple of 7)", B, H, grid_mode);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int c = 64, heads = 2;
  if (!mv_attn_block_supported(prec, c)) {
    btsbot_set_error("op_mv_attn_block: precision %d (BTSBOT_BF16 or BTSBOT_F16)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((long)B * (H / 7) * (H / 7) > 0x7fffffffL) return mv_op_bad("op_mv_attn_block", "too many partitions");
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mv_attn_block");
  const size_t o_qkv = sc.reserve((size_t)3 * c * c * 2), o_proj = sc.reserve((size_t)c * c * 2);
  const size_t o_bias = sc.reserve((size_t)heads * 4096 * 4);
  TRY(sc.alloc());
  // (as maxvit_pack builds p_qkv / p_proj / p_bias64)
  TRY(launch_cast(prec, qkv_w, sc.at(o_qkv), (int64_t)3 * c * c, st));
  TRY(launch_cast(prec, proj_w, sc.at(o_proj), (int64_t)c * c, st));
  TRY(launch_mv_pack_relbias64(table, sc.at<float>(o_bias), heads, st));
  return launch_mv_attn_block(prec, xn, x, xn2, sc.at(o_qkv), qkv_b, sc.at(o_proj), proj_b, sc.at<float>(o_bias), ln2_w,
                              ln2_b, B, H, c, grid_mode, st);
}

extern "C" int btsbot_op_mv_part(int prec, float* x, const float* ln1_w, const float* ln1_b, const float* qkv_w,
                                 const float* qkv_b, const float* proj_w, const float* proj_b, const float* table,
                                 const float* ln2_w, const float* ln2_b, const float* fc1_w, const float* fc1_b,
                                 const float* fc2_w, const float* fc2_b, const float* post_s, const float* post_b,
                                 void* post_out, int B, int H, int C, int grid_mode, void* stream) {
  if (x == nullptr || ln1_w == nullptr || ln1_b == nullptr || qkv_w == nullptr || qkv_b == nullptr || proj_w == nullptr ||
      proj_b == nullptr || table == nullptr)
    return mv_op_bad("op_mv_part", "null pointer");
  const bool mlp = fc1_w != nullptr;
  if (mlp ? (ln2_w == nullptr || ln2_b == nullptr || fc1_b == nullptr || fc2_w == nullptr || fc2_b == nullptr)
          : (ln2_w != nullptr || ln2_b != nullptr || fc1_b != nullptr || fc2_w != nullptr || fc2_b != nullptr))
    return mv_op_bad("op_mv_part", "norm2 / fc1 / fc2: all six pointers (both halves) or none (the attention half)");
  if (post_out != nullptr && (post_s == nullptr || post_b == nullptr)) return mv_op_bad("op_mv_part", "post_out needs post_s and post_b");
  if (B < 0 || H < 7 || H % 7 != 0 || (grid_mode != 0 && grid_mode != 1)) {
    btsbot_set_error("op_mv_part: bad shape B=%d H=%d grid_mode=%d (H a multiple of 7)", B, H, grid_mode);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!mv_part_supported(prec, C)) {
    btsbot_set_error("op_mv_part: unsupported (prec %d, C %d): BTSBOT_BF16 / BTSBOT_F16, C 64 / 128 / 256", prec, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int c = C, heads = C / 32;
  StreamScratch sc(st, "op_mv_part");
  const size_t o_qkv = sc.reserve((size_t)3 * c * c * 2), o_proj = sc.reserve((size_t)c * c * 2);
  const size_t o_biasl = sc.reserve((size_t)heads * 4096 * 4);
  const size_t o_w1 = sc.reserve(mlp ? (size_t)4 * c * c * 2 : 0), o_w2 = sc.reserve(mlp ? (size_t)4 * c * c * 2 : 0);
  TRY(sc.alloc());
  // (maxvit_pack's calls for a block that runs as mv_part_kernel)
  TRY(launch_pack_s2p(prec, qkv_w, nullptr, sc.at(o_qkv), 3 * c, c, 0, 0, nullptr, st));
  TRY(launch_pack_s2p(prec, proj_w, nullptr, sc.at(o_proj), c, c, 0, 0, nullptr, st));
  TRY(launch_mv_pack_relbias_lanes(table, sc.at<float>(o_biasl), heads, st));
  if (mlp) {
    TRY(launch_pack_s2p(prec, fc1_w, nullptr, sc.at(o_w1), 4 * c, c, 0, 0, nullptr, st));
    TRY(launch_pack_s2p(prec, fc2_w, nullptr, sc.at(o_w2), c, 4 * c, 0, 0, nullptr, st));
  }
  MvPartW pw;
  memset(&pw, 0, sizeof(pw));
  pw.ln1w = ln1_w;
  pw.ln1b = ln1_b;
  pw.wqkvp = sc.at(o_qkv);
  pw.bqkv = qkv_b;
  pw.wprojp = sc.at(o_proj);
  pw.bproj = proj_b;
  pw.biasl = sc.at<float>(o_biasl);
  if (mlp) {
    pw.ln2w = ln2_w;
    pw.ln2b = ln2_b;
    pw.w1p = sc.at(o_w1);
    pw.b1 = fc1_b;
    pw.w2p = sc.at(o_w2);
    pw.b2 = fc2_b;
  }
  if (post_out != nullptr) {
    pw.post_s = post_s;
    pw.post_b = post_b;
    pw.post_out = post_out;
  }
  pw.stamps = nullptr;
  return launch_mv_part(prec, x, pw, B, H, C, grid_mode, st);
}

extern "C" int btsbot_op_mv_dw3_groups(int H, int C, int stride) {
  if (H < 1 || C < 8 || C % 8 != 0 || (stride != 1 && stride != 2) || (H / stride) % 7 != 0 || H / stride < 7) {
    btsbot_set_error("op_mv_dw3_groups: bad shape H=%d C=%d stride=%d", H, C, stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return mv_dw3s_groups(H, C, stride);
}

extern "C" int btsbot_op_mv_dw3(int prec, int impl, const void* in, const float* w, const float* scale, const float* bias,
                                void* out, float* part, int B, int H, int C, int stride, void* stream) {
  if (in == nullptr || w == nullptr || scale == nullptr || bias == nullptr || out == nullptr || (impl == 1 && part == nullptr))
    return mv_op_bad("op_mv_dw3", "null pointer");
  if (B < 0 || H < 1 || C < 4 || (stride != 1 && stride != 2) || H % stride != 0 || (impl != 0 && impl != 1)) {
    btsbot_set_error("op_mv_dw3: bad shape B=%d H=%d C=%d stride=%d impl=%d", B, H, C, stride, impl);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (impl == 0 ? !mv_prec_any(prec) : !mv_prec16(prec)) {
    btsbot_set_error("op_mv_dw3: precision %d (impl 0: BTSBOT_F32 / BF16 / F16; impl 1: BF16 / F16)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (impl == 0 ? C % 4 != 0 : (C % 8 != 0 || (H / stride) % 7 != 0 || H / stride < 7)) {
    btsbot_set_error("op_mv_dw3: impl %d cannot run H=%d C=%d stride=%d", impl, H, C, stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mv_dw3");
  const size_t o_w9 = sc.reserve((size_t)9 * C * 4);
  TRY(sc.alloc());
  TRY(launch_mv_pack_dw(w, scale, sc.at<float>(o_w9), C, st));
  if (impl == 0) return launch_mv_dw3(prec, in, sc.at<float>(o_w9), bias, out, B, H, C, stride, st);
  return launch_mv_dw3s(prec, in, sc.at<float>(o_w9), bias, out, part, B, H, C, stride, st);
}

extern "C" int btsbot_op_mv_mbconv_front_tiles(int H, int stride) {
  if (H < 1 || (stride != 1 && stride != 2) || H % stride != 0 || (H / stride) % (stride == 2 ? 7 : 14) != 0) {
    btsbot_set_error("op_mv_mbconv_front_tiles: bad shape H=%d stride=%d", H, stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return mv_mbconv_front_tiles(H, stride);
}

extern "C" int btsbot_op_mv_mbconv_front(int prec, const void* xn, const float* conv1_w, const float* b1, const float* dw_w,
                                         const float* dw_scale, const float* b2, void* m2, float* part, int B, int H,
                                         int CIN, int MID, int stride, void* stream) {
  if (xn == nullptr || conv1_w == nullptr || b1 == nullptr || dw_w == nullptr || dw_scale == nullptr || b2 == nullptr ||
      m2 == nullptr || part == nullptr)
    return mv_op_bad("op_mv_mbconv_front", "null pointer");
  if (B < 0 || H < 1 || CIN < 1 || MID < 1) {
    btsbot_set_error("op_mv_mbconv_front: bad shape B=%d H=%d CIN=%d MID=%d", B, H, CIN, MID);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!mv_mbconv_front_supported(prec, H, CIN, MID, stride)) {
    btsbot_set_error("op_mv_mbconv_front: unsupported (prec %d, H %d, CIN %d, MID %d, stride %d): 16-bit modes, CIN 64, "
                     "MID a multiple of 64, output maps of 28x28 and up in whole tiles", prec, H, CIN, MID, stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mv_mbconv_front");
  const size_t o_w1 = sc.reserve((size_t)MID * CIN * 2), o_w9 = sc.reserve((size_t)9 * MID * 4);
  TRY(sc.alloc());
  TRY(launch_cast(prec, conv1_w, sc.at(o_w1), (int64_t)MID * CIN, st));
  TRY(launch_mv_pack_dw(dw_w, dw_scale, sc.at<float>(o_w9), MID, st));
  return launch_mv_mbconv_front(prec, xn, sc.at(o_w1), b1, sc.at<float>(o_w9), b2, m2, part, B, H, CIN, MID, stride, st);
}

extern "C" int btsbot_op_mv_se(int prec, const void* y, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                               const float* fc2_b, float* gate, int B, int HW, int C, int RD, float inv_count, void* stream) {
  if (y == nullptr || fc1_w == nullptr || fc1_b == nullptr || fc2_w == nullptr || fc2_b == nullptr || gate == nullptr)
    return mv_op_bad("op_mv_se", "null pointer");
  if (B < 0 || HW < 1 || C < 4 || C % 4 != 0 || RD < 1 || RD > 512) {
    btsbot_set_error("op_mv_se: bad shape B=%d HW=%d C=%d RD=%d (C a multiple of 4, RD 1..512)", B, HW, C, RD);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!mv_prec_any(prec)) {
    btsbot_set_error("op_mv_se: precision %d (BTSBOT_F32 rows of partials, or a BTSBOT_BF16 / BTSBOT_F16 map)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mv_se");
  const size_t o_w2t = sc.reserve((size_t)C * RD * 4), o_scr = sc.reserve((size_t)B * (C + RD) * 4);
  TRY(sc.alloc());
  TRY(launch_transpose_f32(fc2_w, sc.at<float>(o_w2t), C, RD, st));   // (as maxvit_pack builds p_se2t)
  return launch_mv_se(prec, y, fc1_w, fc1_b, sc.at<float>(o_w2t), fc2_b, gate, sc.at<float>(o_scr), B, HW, C, RD, inv_count,
                      st);
}

extern "C" int btsbot_op_mv_stem(int prec, const float* img, const float* conv1_w, const float* bn_scale,
                                 const float* bn_shift, const float* conv2_w, float* out, int pooled, void* xn,
                                 const float* pre_scale, const float* pre_shift, int B, void* stream) {
  if (img == nullptr || conv1_w == nullptr || bn_scale == nullptr || bn_shift == nullptr || conv2_w == nullptr ||
      out == nullptr || (xn != nullptr && (pre_scale == nullptr || pre_shift == nullptr)))
    return mv_op_bad("op_mv_stem", "null pointer");
  if (B < 0 || (pooled != 0 && pooled != 1)) {
    btsbot_set_error("op_mv_stem: bad argument B=%d pooled=%d", B, pooled);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!mv_prec16(prec)) {
    btsbot_set_error("op_mv_stem: precision %d (BTSBOT_BF16 or BTSBOT_F16)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mv_stem");
  const size_t o_w1 = sc.reserve((size_t)32 * 32 * 2), o_w2 = sc.reserve((size_t)64 * 288 * 2);
  const size_t o_mid = sc.reserve((size_t)B * 12544 * 32 * 2);
  TRY(sc.alloc());
  TRY(launch_mv_pack_stem1(prec, conv1_w, bn_scale, sc.at(o_w1), st));
  TRY(launch_mv_stem1(prec, img, sc.at(o_w1), bn_shift, sc.at(o_mid), B, st));
  TRY(launch_mv_pack_conv3(prec, conv2_w, sc.at(o_w2), 64, 32, st));
  return launch_mv_stem2(prec, sc.at(o_mid), sc.at(o_w2), out, pooled, xn, pre_scale, pre_shift, B, st);
}

// ---- ConvNeXt stage 3 (stage3.hip) alone: `depth` blocks in place on the caller's rows, and its packers on the caller's
// buffers.  Parameters come in the state-dict layout (fp32); the operand images are built in a stream-ordered scratch by
// the launchers the handle uses (pack.hip's calls for a stage-3 block, stage_args.hip's pointers into them).
namespace {

int s3_op_bad(const char* who, const char* what) {
  btsbot_set_error("%s: %s", who, what);
  return BTSBOT_ERR_INVALID_ARG;
}
bool s3_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool s3_frag_prec(int prec) { return prec == BTSBOT_BF16 || prec == BTSBOT_F16 || prec == BTSBOT_FP8 || prec == BTSBOT_F16X2; }
size_t s3_esz(int prec) { return prec == BTSBOT_FP8 ? 1 : prec == BTSBOT_F16X2 ? 4 : 2; }

}  // namespace

extern "C" int btsbot_op_cn_stage3_supported(int prec, int c3, int depth) { return stage3_supported(prec, c3, depth) ? 1 : 0; }

extern "C" int64_t btsbot_op_cn_stage3_hfrag_bytes(int prec, int c3, int B) {
  if (!s3_frag_prec(prec) || c3 < 1 || B < 0) {
    btsbot_set_error("op_cn_stage3_hfrag_bytes: bad argument prec=%d c3=%d B=%d", prec, c3, B);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return (int64_t)stage3_hfrag_bytes(prec, c3, B);
}

extern "C" int btsbot_op_cn_stage3(int prec, int c3, int depth, int wide, float* x, int B, const float* const* dw_w,
                                   const float* const* dw_b, const float* const* ln_w, const float* const* ln_b,
                                   const float* const* fc1_w, const float* const* fc1_b, const float* const* fc2_w,
                                   const float* const* fc2_b, const float* const* gamma, void* stream) {
  const char* who = "op_cn_stage3";
  if (!stage3_supported(prec, c3, depth)) {
    btsbot_set_error("op_cn_stage3: unsupported (prec %d, width %d, depth %d): BTSBOT_BF16 / F16 / FP8 / F16X2, 512 or 640 "
                     "channels, 1 to %d blocks", prec, c3, depth, S3_MAX_DEPTH);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (wide != 0 && wide != 1) return s3_op_bad(who, "wide must be 0 or 1");
  if (wide && prec == BTSBOT_F16X2) return s3_op_bad(who, "the split mode has no wide tiles");
  if (B < 0) return s3_op_bad(who, "negative row count");
  const float* const* lists[9] = {dw_w, dw_b, ln_w, ln_b, fc1_w, fc1_b, fc2_w, fc2_b, gamma};
  if (x == nullptr) return s3_op_bad(who, "null pointer");
  for (const float* const* l : lists) {
    if (l == nullptr) return s3_op_bad(who, "null pointer");
    for (int j = 0; j < depth; ++j)
      if (l[j] == nullptr) return s3_op_bad(who, "null pointer");
  }
  if (!s3_al16(x)) return s3_op_bad(who, "x must be 16-byte aligned");
  for (int j = 0; j < depth; ++j)
    if (!s3_al16(dw_b[j]) || !s3_al16(ln_w[j]) || !s3_al16(ln_b[j]) || !s3_al16(fc1_b[j]) || !s3_al16(fc2_b[j]) ||
        !s3_al16(gamma[j]))
      return s3_op_bad(who, "the parameter vectors must be 16-byte aligned");
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int ch = c3;
  const size_t wb = (size_t)4 * ch * ch * s3_esz(prec), hbytes = stage3_hfrag_bytes(prec, ch, B);
  StreamScratch sc(st, who);   // per block: tap-major taps | fc1 fragments | gamma * fc2 fragments | scales; then hfrag
  size_t o_dw[S3_MAX_DEPTH], o_w1[S3_MAX_DEPTH], o_w2[S3_MAX_DEPTH], o_sc[S3_MAX_DEPTH];
  for (int j = 0; j < depth; ++j) {
    o_dw[j] = sc.reserve((size_t)49 * ch * 4);
    o_w1[j] = sc.reserve(wb);
    o_w2[j] = sc.reserve(wb);
    o_sc[j] = sc.reserve(64);
  }
  const size_t o_h = sc.reserve(hbytes);
  TRY(sc.alloc());
  Stage3Args a;
  memset(&a, 0, sizeof(a));
  a.x = x;
  a.depth = depth;
  a.hfrag = sc.at(o_h);
  a.B = B;
  a.stamps = nullptr;
  for (int j = 0; j < depth; ++j) {
    float* scales = sc.at<float>(o_sc[j]);
    TRY(launch_transpose_f32(dw_w[j], sc.at<float>(o_dw[j]), ch, 49, st));   // (pack.hip's p_dw: tap-major [49][C])
    TRY(launch_pack_s3(prec, fc1_w[j], nullptr, sc.at(o_w1[j]), 4 * ch, ch, 1, scales, st));
    TRY(launch_pack_s3(prec, fc2_w[j], gamma[j], sc.at(o_w2[j]), ch, 4 * ch, 0, scales + 2, st));
    Stage3Blk& k = a.blk[j];
    k.dw_c = sc.at<float>(o_dw[j]) + 24 * ch;   // the centre row (stage_args.hip)
    k.dw_b = dw_b[j];
    k.ln_w = ln_w[j];
    k.ln_b = ln_b[j];
    k.w1p = sc.at(o_w1[j]);
    k.b1 = fc1_b[j];
    k.w2p = sc.at(o_w2[j]);
    k.b2 = fc2_b[j];
    k.gamma = gamma[j];
    k.scales = prec == BTSBOT_FP8 ? scales : nullptr;
  }
  // 0xFF bytes are NaN in bf16, f16 and e4m3: a block of hfrag that no fc1 tile wrote shows if it reaches a live row
  HIP_TRY(hipMemsetAsync(a.hfrag, 0xFF, hbytes, st));
  for (int j = 0; j < depth; ++j) {
    TRY(launch_stage3(prec, ch, a, j, 0, wide != 0, st));
    TRY(launch_stage3(prec, ch, a, j, 1, wide != 0, st));
  }
  return BTSBOT_OK;
}

extern "C" int btsbot_op_cn_pack_s3(int prec, const float* src, const float* rowscale, int rows, int K, int swap23, void* dst,
                                    float* scale, void* stream) {
  const char* who = "op_cn_pack_s3";
  if (src == nullptr || dst == nullptr) return s3_op_bad(who, "null pointer");
  if (!s3_frag_prec(prec)) return s3_op_bad(who, "precision must be bf16, f16, fp8 or f16x2");
  if (prec == BTSBOT_FP8 && scale == nullptr) return s3_op_bad(who, "the fp8 mode needs a scale slot");
  const int kstep = prec == BTSBOT_FP8 ? 64 : 16;
  if (rows < 32 || rows % 32 != 0 || K < kstep || K % kstep != 0 || (long)rows * K >= (1L << 31)) {
    btsbot_set_error("op_cn_pack_s3: bad shape rows=%d K=%d (rows a multiple of 32, K of %d)", rows, K, kstep);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (swap23 != 0 && swap23 != 1) return s3_op_bad(who, "swap23 must be 0 or 1");
  return launch_pack_s3(prec, src, rowscale, dst, rows, K, swap23, scale, (hipStream_t)stream);
}

extern "C" int btsbot_op_cn_fp8_scale(const float* src, const float* rowscale, int64_t n, int K, float* scale, void* stream) {
  const char* who = "op_cn_fp8_scale";
  if (src == nullptr || scale == nullptr) return s3_op_bad(who, "null pointer");
  if (n < 1 || K < 1 || (rowscale != nullptr && n % K != 0)) {
    btsbot_set_error("op_cn_fp8_scale: bad shape n=%ld K=%d (n >= 1; whole rows of K where rowscale is given)", (long)n, K);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_fp8_scale(src, rowscale, (long)n, K, scale, (hipStream_t)stream);
}

// ---- ConvNeXt stage 2 (+ stages[3].downsample) alone: stage2p_kernel in every form it is launched in, on the caller's
// buffers.  Parameters in state-dict layout (fp32); the operand images are built in a stream-ordered scratch by the calls
// pack.hip makes for a stage-2 block and the downsample behind it (stage_args.hip's pointers into them).
extern "C" int btsbot_op_cn_stage2_supported(int prec, int cw, int depth) { return stage2p_supported(prec, cw, 2 * cw, depth) ? 1 : 0; }

extern "C" int btsbot_op_cn_stage2_alerts(int B, int hint) {
  if (B < 0 || (hint != 0 && hint != 4 && hint != 5 && hint != 7)) {
    btsbot_set_error("op_cn_stage2_alerts: bad argument B=%d hint=%d (hint 0, 4, 5 or 7)", B, hint);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return stage2p_alerts_per_workgroup(B, hint);
}

extern "C" int btsbot_op_cn_stage2(int prec, int cw, int depth, int alerts_hint, const float* x_in, int B,
                                   const float* const* dw_w, const float* const* dw_b, const float* const* ln_w,
                                   const float* const* ln_b, const float* const* fc1_w, const float* const* fc1_b,
                                   const float* const* fc2_w, const float* const* fc2_b, const float* const* gamma,
                                   const float* ds_ln_w, const float* ds_ln_b, const float* ds_w, const float* ds_b, float* out,
                                   float* tap_stage, float* const* keep_xin, void* const* keep_xn, void* const* keep_a,
                                   void* const* keep_hh, void* ds_patches, void* stream) {
  const char* who = "op_cn_stage2";
  if (!stage2p_supported(prec, cw, 2 * cw, depth)) {
    btsbot_set_error("op_cn_stage2: unsupported (prec %d, width %d, depth %d): BTSBOT_BF16 / F16 / FP8 / F16X2 at 256 channels, "
                     "BF16 / F16 at 320, 1 to %d blocks", prec, cw, depth, S2P_MAX_DEPTH);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (alerts_hint != 0 && alerts_hint != 4 && alerts_hint != 5 && alerts_hint != 7)
    return s3_op_bad(who, "alerts_hint must be 0, 4, 5 or 7");
  if (B < 0) return s3_op_bad(who, "negative alert count");
  const int nkeep = (keep_xin != nullptr) + (keep_xn != nullptr) + (keep_a != nullptr) + (keep_hh != nullptr) + (ds_patches != nullptr);
  if (nkeep != 0 && nkeep != 5) return s3_op_bad(who, "the keep buffers (xin, xn, a, hh, ds_patches) are given all or none");
  const bool train = nkeep == 5;
  if (train && (cw != 256 || (prec != BTSBOT_BF16 && prec != BTSBOT_F16)))
    return s3_op_bad(who, "the keeping form runs in the bf16 / f16 modes at 256 channels");
  if (train && tap_stage == nullptr) return s3_op_bad(who, "the keeping form needs tap_stage (the stage output)");
  const float* const* lists[9] = {dw_w, dw_b, ln_w, ln_b, fc1_w, fc1_b, fc2_w, fc2_b, gamma};
  if (x_in == nullptr || out == nullptr || ds_ln_w == nullptr || ds_ln_b == nullptr || ds_w == nullptr || ds_b == nullptr)
    return s3_op_bad(who, "null pointer");
  for (const float* const* l : lists) {
    if (l == nullptr) return s3_op_bad(who, "null pointer");
    for (int j = 0; j < depth; ++j)
      if (l[j] == nullptr) return s3_op_bad(who, "null pointer");
  }
  if (train)
    for (int j = 0; j < depth; ++j)
      if (keep_xin[j] == nullptr || keep_xn[j] == nullptr || keep_a[j] == nullptr || keep_hh[j] == nullptr)
        return s3_op_bad(who, "null pointer");
  if (!s3_al16(x_in) || !s3_al16(out) || !s3_al16(tap_stage)) return s3_op_bad(who, "x_in, out and tap_stage must be 16-byte aligned");
  if (!s3_al16(ds_ln_w) || !s3_al16(ds_ln_b) || !s3_al16(ds_b)) return s3_op_bad(who, "the parameter vectors must be 16-byte aligned");
  for (int j = 0; j < depth; ++j)
    if (!s3_al16(dw_b[j]) || !s3_al16(ln_w[j]) || !s3_al16(ln_b[j]) || !s3_al16(fc1_b[j]) || !s3_al16(fc2_b[j]) ||
        !s3_al16(gamma[j]))
      return s3_op_bad(who, "the parameter vectors must be 16-byte aligned");
  if (train) {
    if (!s3_al16(ds_patches)) return s3_op_bad(who, "the keep buffers must be 16-byte aligned");
    for (int j = 0; j < depth; ++j)
      if (!s3_al16(keep_xin[j]) || !s3_al16(keep_xn[j]) || !s3_al16(keep_a[j]) || !s3_al16(keep_hh[j]))
        return s3_op_bad(who, "the keep buffers must be 16-byte aligned");
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int precd = prec == BTSBOT_FP8 ? BTSBOT_BF16 : prec;   // (prec_down3: the downsample keeps 16-bit operands)
  const size_t wb = (size_t)4 * cw * cw * s3_esz(prec), wdb = (size_t)8 * cw * cw * s3_esz(precd);
  StreamScratch sc(st, who);   // per block: tap-major taps | fc1 fragments | gamma * fc2 fragments | scales; then the downsample's
  size_t o_dw[S2P_MAX_DEPTH], o_w1[S2P_MAX_DEPTH], o_w2[S2P_MAX_DEPTH], o_sc[S2P_MAX_DEPTH];
  for (int j = 0; j < depth; ++j) {
    o_dw[j] = sc.reserve((size_t)49 * cw * 4);
    o_w1[j] = sc.reserve(wb);
    o_w2[j] = sc.reserve(wb);
    o_sc[j] = sc.reserve(64);
  }
  const size_t o_ds = sc.reserve(wdb);
  TRY(sc.alloc());
  Stage2pArgs a;
  memset(&a, 0, sizeof(a));
  a.x_in = x_in;
  a.depth = depth;
  a.ds_lnw = ds_ln_w;
  a.ds_lnb = ds_ln_b;
  a.ds_wp = sc.at(o_ds);
  a.ds_b = ds_b;
  a.out = out;
  a.tap_stage = tap_stage;
  a.B = B;
  a.cw = cw;
  a.alerts_hint = alerts_hint;
  a.train = train ? 1 : 0;
  a.ds_patches = ds_patches;
  for (int j = 0; j < depth; ++j) {
    float* scales = sc.at<float>(o_sc[j]);
    TRY(launch_transpose_f32(dw_w[j], sc.at<float>(o_dw[j]), cw, 49, st));   // (pack.hip's p_dw: tap-major [49][C])
    TRY(launch_pack_s2p(prec, fc1_w[j], nullptr, sc.at(o_w1[j]), 4 * cw, cw, 0, 0, scales, st));
    TRY(launch_pack_s2p(prec, fc2_w[j], gamma[j], sc.at(o_w2[j]), cw, 4 * cw, 0, 0, scales + 2, st));
    Stage2pBlk& k = a.blk[j];
    k.dw_w = sc.at<float>(o_dw[j]);
    k.dw_b = dw_b[j];
    k.ln_w = ln_w[j];
    k.ln_b = ln_b[j];
    k.b1 = fc1_b[j];
    k.b2 = fc2_b[j];
    k.gamma = gamma[j];
    k.w1p = sc.at(o_w1[j]);
    k.w2p = sc.at(o_w2[j]);
    k.scales = prec == BTSBOT_FP8 ? scales : nullptr;
    if (train) a.keep[j] = Stage2pKeep{keep_xin[j], keep_xn[j], keep_a[j], keep_hh[j]};
  }
  TRY(launch_pack_s2p(precd, ds_w, nullptr, sc.at(o_ds), 2 * cw, 4 * cw, 1, cw, nullptr, st));
  return launch_stage2p(prec, a, st);
}

extern "C" int btsbot_op_cn_stage2_rows(int prec, float* x, int64_t rows, const float* ln_w, const float* ln_b,
                                        const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                                        const float* gamma, void* stream) {
  const char* who = "op_cn_stage2_rows";
  if (!stage2p_rows_supported(prec, 256)) return s3_op_bad(who, "unsupported: the row-tile form runs in the bf16 / f16 modes");
  if (rows < 0 || rows > 0x7fffffffL / 256) return s3_op_bad(who, "bad row count");
  if (x == nullptr || ln_w == nullptr || ln_b == nullptr || fc1_w == nullptr || fc1_b == nullptr || fc2_w == nullptr ||
      fc2_b == nullptr || gamma == nullptr)
    return s3_op_bad(who, "null pointer");
  if (!s3_al16(x)) return s3_op_bad(who, "x must be 16-byte aligned");
  if (!s3_al16(ln_w) || !s3_al16(ln_b) || !s3_al16(fc1_b) || !s3_al16(fc2_b) || !s3_al16(gamma))
    return s3_op_bad(who, "the parameter vectors must be 16-byte aligned");
  if (rows == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int c = 256;
  const size_t wb = (size_t)4 * c * c * 2;
  StreamScratch sc(st, who);   // fc1 fragments | gamma * fc2 fragments
  const size_t o_w1 = sc.reserve(wb), o_w2 = sc.reserve(wb);
  TRY(sc.alloc());
  TRY(launch_pack_s2p(prec, fc1_w, nullptr, sc.at(o_w1), 4 * c, c, 0, 0, nullptr, st));
  TRY(launch_pack_s2p(prec, fc2_w, gamma, sc.at(o_w2), c, 4 * c, 0, 0, nullptr, st));
  Stage2pBlk sb;
  memset(&sb, 0, sizeof(sb));
  sb.ln_w = ln_w;
  sb.ln_b = ln_b;
  sb.b1 = fc1_b;
  sb.b2 = fc2_b;
  sb.gamma = gamma;
  sb.w1p = sc.at(o_w1);
  sb.w2p = sc.at(o_w2);
  return launch_stage2p_rows(prec, x, (long)rows, sb, st);
}

extern "C" int btsbot_op_cn_pack_s2p(int prec, const float* src, const float* rowscale, int rows, int K, int reorder_down,
                                     int cin, void* dst, float* scale, void* stream) {
  const char* who = "op_cn_pack_s2p";
  if (src == nullptr || dst == nullptr) return s3_op_bad(who, "null pointer");
  if (!s3_frag_prec(prec)) return s3_op_bad(who, "precision must be bf16, f16, fp8 or f16x2");
  if (prec == BTSBOT_FP8 && scale == nullptr) return s3_op_bad(who, "the fp8 mode needs a scale slot");
  const int kstep = prec == BTSBOT_FP8 ? 128 : 32;
  if (rows < 16 || rows % 16 != 0 || K < kstep || K % kstep != 0 || (long)rows * K >= (1L << 31)) {
    btsbot_set_error("op_cn_pack_s2p: bad shape rows=%d K=%d (rows a multiple of 16, K of %d)", rows, K, kstep);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (reorder_down != 0 && reorder_down != 1) return s3_op_bad(who, "reorder_down must be 0 or 1");
  if (reorder_down && (cin < 1 || K != 4 * cin)) return s3_op_bad(who, "reorder_down: K must be 4 cin");
  return launch_pack_s2p(prec, src, rowscale, dst, rows, K, reorder_down, cin, scale, (hipStream_t)stream);
}
