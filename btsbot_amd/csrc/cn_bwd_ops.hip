// Op-level entry points of the ConvNeXt training step's LayerNorm / depthwise backward (include/btsbot_hip.h,
// btsbot_op_cnt_*): the launchers of dwln_bwd.hip, ln_dw_bwd.hip and stem_dgrad.hip one at a time, on the caller's tensors and stream,
// for the per-kernel tests.  Nothing here is on the product path: backbone_train_backward calls the same launchers.
// Every entry point checks its arguments before it allocates or launches anything; what its launcher has no kernel for
// comes back as BTSBOT_ERR_INVALID_ARG with a message.
#include "common.h"

namespace {

constexpr size_t LDS_MAX = 160 * 1024;   // dynamic LDS one gfx950 workgroup can ask for

int cnt_bad(const char* who, const char* what) {
  btsbot_set_error("%s: %s", who, what);
  return BTSBOT_ERR_INVALID_ARG;
}
bool out16_ok(const void* out16, int prec16) { return out16 == nullptr || prec16 == BTSBOT_BF16 || prec16 == BTSBOT_F16; }

// the arguments dwln_bwd and dw3ln_bwd share (P = pixels of a map)
int cnt_planes(const char* who, int B, int P, int C, int nplanes, int64_t pstride) {
  if (B < 0 || nplanes < 1 || (nplanes > 1 && pstride < (int64_t)B * P * C)) {
    btsbot_set_error("%s: bad shape B=%d nplanes=%d pstride=%lld (B >= 0, nplanes >= 1, planes at least B*P*C floats apart)",
                     who, B, nplanes, (long long)pstride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

// the depthwise kernels of ln_dw_bwd.hip: a map side they are instantiated for, 16-byte pixel rows, maps that fit LDS
int cnt_dw_shape(const char* who, int B, int HW, int C, size_t lds) {
  if (B < 0 || (HW != 15 && HW != 7 && HW != 3 && HW != 1) || C < 4 || C % 4 != 0 || lds > LDS_MAX) {
    btsbot_set_error("%s: bad shape B=%d HW=%d C=%d (HW 15, 7, 3 or 1; C a multiple of 4; %zu bytes of LDS, at most %zu)", who,
                     B, HW, C, lds, LDS_MAX);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

}  // namespace

extern "C" int btsbot_op_cnt_dwln_bwd_rows(int HW, int C, int B) {
  if (!dwln_bwd_supported(HW, C) || B < 0) return cnt_bad("op_cnt_dwln_bwd_rows", "no kernel for this map, or B < 0");
  return dwln_bwd_grid(HW, C, B);
}
extern "C" int btsbot_op_cnt_dw3ln_bwd_rows(int B) {
  if (B < 0) return cnt_bad("op_cnt_dw3ln_bwd_rows", "B < 0");
  return B == 0 ? 0 : dw3_rows(B);
}

extern "C" int btsbot_op_cnt_dwln_bwd(const float* d, const float* dxn, const float* g, const float* xin, const float* w,
                                      float* dy, void* out16, int prec16, float* arena, int B, int HW, int C, int nplanes,
                                      int64_t pstride, void* stream) {
  if (d == nullptr || dxn == nullptr || g == nullptr || xin == nullptr || w == nullptr || dy == nullptr || arena == nullptr)
    return cnt_bad("op_cnt_dwln_bwd", "null pointer");
  if (!out16_ok(out16, prec16)) return cnt_bad("op_cnt_dwln_bwd", "out16 needs prec16 = BTSBOT_BF16 or BTSBOT_F16");
  if (!dwln_bwd_supported(HW, C)) {
    btsbot_set_error("op_cnt_dwln_bwd: no kernel for a %dx%d map of %d channels", HW, HW, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  TRY(cnt_planes("op_cnt_dwln_bwd", B, HW * HW, C, nplanes, pstride));
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int rows = dwln_bwd_grid(HW, C, B);
  StreamScratch part(st, "op_cnt");   // partial rows of this call
  part.reserve((size_t)rows * 52 * C * 4);
  TRY(part.alloc());
  TRY(launch_dwln_bwd(d, dxn, g, xin, w, dy, out16, prec16, part.at<float>(0), B, HW, C, st, nplanes, (size_t)pstride));
  return launch_colsum(BTSBOT_F32, part.at<float>(0), arena, rows, 52 * C, st);
}

extern "C" int btsbot_op_cnt_dw3ln_bwd(const float* dwb, const float* dxn, const float* g, const float* xin, const float* w,
                                       float* dy, void* out16, int prec16, float* arena, int B, int HW, int C, int nplanes,
                                       int64_t pstride, void* stream) {
  if (dwb == nullptr || dxn == nullptr || g == nullptr || xin == nullptr || w == nullptr || dy == nullptr || arena == nullptr)
    return cnt_bad("op_cnt_dw3ln_bwd", "null pointer");
  if (!out16_ok(out16, prec16)) return cnt_bad("op_cnt_dw3ln_bwd", "out16 needs prec16 = BTSBOT_BF16 or BTSBOT_F16");
  if (HW != 3 || C != 256) {
    btsbot_set_error("op_cnt_dw3ln_bwd: no kernel for a %dx%d map of %d channels (3x3 maps of 256)", HW, HW, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  TRY(cnt_planes("op_cnt_dw3ln_bwd", B, 9, C, nplanes, pstride));
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int rows = dw3_rows(B);
  StreamScratch part(st, "op_cnt");   // partial rows of this call
  part.reserve((size_t)rows * 28 * C * 4);
  TRY(part.alloc());   // compact rows: 25 live taps | bias | LayerNorm weight | bias, per channel
  TRY(launch_dw3ln_bwd(dwb, dxn, g, xin, w, dy, out16, prec16, part.at<float>(0), B, st, nplanes, (size_t)pstride));
  return launch_dw3_rows(part.at<float>(0), arena, rows, st);
}

extern "C" int btsbot_op_cnt_ln_bwd(const float* d, const float* dxn, const float* g, float* dd, float* dg, float* dbeta,
                                    int64_t rows, int C, void* out16, int prec16, int patch_hw, void* stream) {
  if (d == nullptr || dxn == nullptr || g == nullptr || dd == nullptr || dg == nullptr || dbeta == nullptr)
    return cnt_bad("op_cnt_ln_bwd", "null pointer");
  if (!out16_ok(out16, prec16)) return cnt_bad("op_cnt_ln_bwd", "out16 needs prec16 = BTSBOT_BF16 or BTSBOT_F16");
  if (rows < 0 || C < 1 || C > 640 || patch_hw < 0 || patch_hw == 1 ||
      (patch_hw != 0 && rows % ((int64_t)patch_hw * patch_hw) != 0)) {
    btsbot_set_error("op_cnt_ln_bwd: bad shape rows=%lld C=%d patch_hw=%d (C at most 640; patch_hw 0 or the side >= 2 of whole maps)",
                     (long long)rows, C, patch_hw);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (patch_hw != 0 && dd == dxn) return cnt_bad("op_cnt_ln_bwd", "the patch matrix cannot be overwritten in place");
  return launch_ln_bwd(d, dxn, g, dd, dg, dbeta, (long)rows, C, (hipStream_t)stream, out16, prec16, patch_hw);
}

extern "C" int btsbot_op_cnt_ln_dw1_bwd(const float* d, const float* dxn, const float* g, const float* xin, const float* w,
                                        float* dy, void* out16, int prec16, float* dg, float* dbeta, float* dw, float* dbias,
                                        int64_t rows, int C, void* stream) {
  if (d == nullptr || dxn == nullptr || g == nullptr || xin == nullptr || w == nullptr || dy == nullptr || dg == nullptr ||
      dbeta == nullptr || dw == nullptr || dbias == nullptr)
    return cnt_bad("op_cnt_ln_dw1_bwd", "null pointer");
  if (!out16_ok(out16, prec16)) return cnt_bad("op_cnt_ln_dw1_bwd", "out16 needs prec16 = BTSBOT_BF16 or BTSBOT_F16");
  if (rows < 0 || C < 1 || C > 640) {
    btsbot_set_error("op_cnt_ln_dw1_bwd: bad shape rows=%lld C=%d (C at most 640)", (long long)rows, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_ln_dw1_bwd(d, dxn, g, xin, w, dy, out16, prec16, dg, dbeta, dw, dbias, (long)rows, C, (hipStream_t)stream);
}

extern "C" int btsbot_op_cnt_dw_plain(const float* x, const float* w, int flip, const float* bias, const float* addend,
                                      float* out, void* out16, int prec16, int B, int HW, int C, void* stream) {
  if (x == nullptr || w == nullptr || out == nullptr) return cnt_bad("op_cnt_dw_plain", "null pointer");
  if (!out16_ok(out16, prec16)) return cnt_bad("op_cnt_dw_plain", "out16 needs prec16 = BTSBOT_BF16 or BTSBOT_F16");
  if (flip != 0 && flip != 1) return cnt_bad("op_cnt_dw_plain", "flip is 0 or 1");
  TRY(cnt_dw_shape("op_cnt_dw_plain", B, HW, C, ((size_t)HW * HW + 49) * (size_t)(C > 0 ? C : 0) * sizeof(float)));
  return launch_dw_plain(x, w, flip, bias, addend, out, B, HW, C, (hipStream_t)stream, out16, prec16);
}

extern "C" int btsbot_op_cnt_dw_wgrad(const float* x, const float* dd, float* dw, float* dbias, int B, int HW, int C,
                                      void* stream) {
  if (x == nullptr || dd == nullptr || dw == nullptr || dbias == nullptr) return cnt_bad("op_cnt_dw_wgrad", "null pointer");
  TRY(cnt_dw_shape("op_cnt_dw_wgrad", B, HW, C, 2 * (size_t)HW * HW * (size_t)(C > 0 ? C : 0) * sizeof(float)));
  if (dbias != dw + (size_t)49 * C) return cnt_bad("op_cnt_dw_wgrad", "filter and bias gradients must be adjacent (dbias = dw + 49 C)");
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  // one partial row [C*49 | C] per workgroup (<= 256) and row group (256 / C of them where C < 256)
  StreamScratch part(st, "op_cnt");   // partial rows of this call
  part.reserve((size_t)256 * 50 * (C < 256 ? 256 : C) * 4);
  TRY(part.alloc());
  return launch_dw_wgrad(x, dd, dw, dbias, part.at<float>(0), B, HW, C, st);
}

extern "C" int btsbot_op_cnt_colsum_f32(const float* in, float* out, int M, int N, void* stream) {
  if (in == nullptr || out == nullptr) return cnt_bad("op_cnt_colsum_f32", "null pointer");
  if (M < 0 || N < 1) {
    btsbot_set_error("op_cnt_colsum_f32: bad shape M=%d N=%d", M, N);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_colsum(BTSBOT_F32, in, out, M, N, (hipStream_t)stream);
}

extern "C" int btsbot_op_cnt_stem_dgrad(const float* dxn, const float* w, float* dimg, int B, int C0, void* stream) {
  if (dxn == nullptr || w == nullptr || dimg == nullptr) return cnt_bad("op_cnt_stem_dgrad", "null pointer");
  if (B < 0 || B > (1 << 17) || (C0 != 64 && C0 != 80)) {
    btsbot_set_error("op_cnt_stem_dgrad: bad shape B=%d C0=%d (0 <= B <= 131072; C0 64 or 80)", B, C0);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_stem_dgrad(dxn, w, dimg, B, C0, (hipStream_t)stream);
}
