// Op-level entry points of the MaxViT training kernels (include/btsbot_hip.h, btsbot_op_mvt_*): the launchers of
// maxvit_train_kernels.hip, one kernel group at a time, on the caller's tensors and a stream-ordered scratch
#include "maxvit.h"

namespace {

int mvt_bad(const char* who, const char* what) {
  btsbot_set_error("%s: %s", who, what);
  return BTSBOT_ERR_INVALID_ARG;
}
// the depthwise ops' shape rule: C a multiple of 4, stride 1 or 2 dividing H
int mvt_dw3_shape(const char* who, int B, int H, int C, int stride) {
  if (B < 0 || H < 1 || C < 4 || C % 4 != 0 || (stride != 1 && stride != 2) || H % stride != 0) {
    btsbot_set_error("%s: bad shape B=%d H=%d C=%d stride=%d (C a multiple of 4, stride 1 or 2 dividing H)", who, B, H, C, stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}
// taps [9][C] of w [C][1][3][3] as the engine packs them (scale = 1)
int mvt_pack_taps(const float* w, float* ones, float* w9, int C, hipStream_t st) {
  TRY(launch_mv_fill(ones, 1.0f, C, st));
  return launch_mv_pack_dw(w, ones, w9, C, st);
}

}  // namespace

extern "C" int btsbot_op_mvt_bn_row_blocks(int64_t M) {
  if (M < 1) return mvt_bad("op_mvt_bn_row_blocks", "M < 1");
  return (int)bn_row_blocks((long)M);
}
extern "C" int btsbot_op_mvt_dw3_bwd_w_row_blocks(int64_t npix) {
  if (npix < 1) return mvt_bad("op_mvt_dw3_bwd_w_row_blocks", "npix < 1");
  return (int)dw3_bwd_w_row_blocks((long)npix);
}
extern "C" int btsbot_op_mvt_attn_bwd_groups_per_head(int64_t units, int heads) {
  if (units < 1 || units > 0x7fffffffL || heads < 1 || heads > 16) return mvt_bad("op_mvt_attn_bwd_groups_per_head", "units < 1 or heads outside 1..16");
  return (int)attn_bwd_groups_per_head((long)units, heads);
}

extern "C" int btsbot_op_mvt_bn_fwd(const float* x, const float* w, const float* b, float* run_mean, float* run_var, float* y,
                                    float* stat, int64_t M, int C, int act, void* stream) {
  if (x == nullptr || w == nullptr || b == nullptr || y == nullptr || stat == nullptr || (run_mean == nullptr) != (run_var == nullptr))
    return mvt_bad("op_mvt_bn_fwd", "null pointer (run_mean and run_var: both or neither)");
  if (M < 1 || C < 4 || C % 4 != 0 || (act != 0 && act != 1)) {
    btsbot_set_error("op_mvt_bn_fwd: bad shape M=%lld C=%d act=%d (C a multiple of 4, act 0 or 1)", (long long)M, C, act);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mvt");
  const size_t o0 = sc.reserve(2 * (size_t)C * 4), o1 = sc.reserve(2 * (size_t)C * 4);
  TRY(sc.alloc());
  HIP_TRY(hipMemsetAsync(sc.base, 0, sc.total, st));
  return launch_bn_train(x, w, b, stat, sc.at<float>(o0), sc.at<float>(o1), run_mean, run_var, y, (long)M, C, act, st);
}

extern "C" int btsbot_op_mvt_bn_bwd(const float* x, const float* dy, const float* stat, const float* w, const float* b, float* dx,
                                    float* dw, float* db, int64_t M, int C, int act, int accumulate, void* stream) {
  if (x == nullptr || dy == nullptr || stat == nullptr || w == nullptr || b == nullptr || dx == nullptr || dw == nullptr ||
      db == nullptr)
    return mvt_bad("op_mvt_bn_bwd", "null pointer");
  if (M < 1 || C < 4 || C % 4 != 0 || (act != 0 && act != 1) || (accumulate != 0 && accumulate != 1)) {
    btsbot_set_error("op_mvt_bn_bwd: bad shape M=%lld C=%d act=%d accumulate=%d (C a multiple of 4, flags 0 or 1)", (long long)M, C,
                     act, accumulate);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mvt");
  const size_t o = sc.reserve(2 * (size_t)C * 4);
  TRY(sc.alloc());
  HIP_TRY(hipMemsetAsync(sc.base, 0, sc.total, st));
  return launch_bn_train_bwd(x, dy, stat, w, b, sc.at<float>(o), dx, dw, db, (long)M, C, act, accumulate, st);
}

extern "C" int btsbot_op_mvt_dw3_fwd(const float* in, const float* w, const float* bias, float* out, int B, int H, int C,
                                     int stride, void* stream) {
  if (in == nullptr || w == nullptr || bias == nullptr || out == nullptr) return mvt_bad("op_mvt_dw3_fwd", "null pointer");
  TRY(mvt_dw3_shape("op_mvt_dw3_fwd", B, H, C, stride));
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mvt");
  const size_t o1 = sc.reserve(C * 4), o9 = sc.reserve(9 * (size_t)C * 4);
  TRY(sc.alloc());
  TRY(mvt_pack_taps(w, sc.at<float>(o1), sc.at<float>(o9), C, st));
  return launch_dw3_fwd(in, sc.at<float>(o9), bias, out, B, H, C, stride, st);
}

extern "C" int btsbot_op_mvt_dw3_bwd_in(const float* dout, const float* w, float* din, int B, int H, int C, int stride,
                                        void* stream) {
  if (dout == nullptr || w == nullptr || din == nullptr) return mvt_bad("op_mvt_dw3_bwd_in", "null pointer");
  TRY(mvt_dw3_shape("op_mvt_dw3_bwd_in", B, H, C, stride));
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mvt");
  const size_t o1 = sc.reserve(C * 4), o9 = sc.reserve(9 * (size_t)C * 4);
  TRY(sc.alloc());
  TRY(mvt_pack_taps(w, sc.at<float>(o1), sc.at<float>(o9), C, st));
  return launch_dw3_bwd_in(dout, sc.at<float>(o9), din, B, H, C, stride, st);
}

extern "C" int btsbot_op_mvt_dw3_bwd_w(const float* in, const float* dout, float* dw, float* dbias, int B, int H, int C,
                                       int stride, void* stream) {
  if (in == nullptr || dout == nullptr || dw == nullptr || dbias == nullptr) return mvt_bad("op_mvt_dw3_bwd_w", "null pointer");
  TRY(mvt_dw3_shape("op_mvt_dw3_bwd_w", B, H, C, stride));
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mvt");
  const size_t o = sc.reserve(10 * (size_t)C * 4);
  TRY(sc.alloc());
  return launch_dw3_bwd_w(in, dout, sc.at<float>(o), dw, dbias, B, H, C, stride, st);
}

extern "C" int btsbot_op_mvt_attn_bwd(const float* qkv, const float* table, const float* dout, float* dqkv, float* dtable, int B,
                                      int H, int C, int grid_mode, void* stream) {
  if (qkv == nullptr || table == nullptr || dout == nullptr || dqkv == nullptr || dtable == nullptr)
    return mvt_bad("op_mvt_attn_bwd", "null pointer");
  if (B < 0 || H < 7 || H % 7 != 0 || C < 32 || C % 32 != 0 || C / 32 > 16 || (grid_mode != 0 && grid_mode != 1)) {
    btsbot_set_error("op_mvt_attn_bwd: bad shape B=%d H=%d C=%d grid_mode=%d (H a multiple of 7, C of 32, at most 16 heads)", B, H,
                     C, grid_mode);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((long)B * (H / 7) * (H / 7) > 0x7fffffffL) return mvt_bad("op_mvt_attn_bwd", "too many (alert, partition) units");
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mvt");
  const size_t o = sc.reserve((size_t)32 * 2401 * 4);
  TRY(sc.alloc());
  return launch_attn_bwd(qkv, table, dout, dqkv, sc.at<float>(o), dtable, B, H, C, grid_mode, st);
}

// (the small dense kernels index [B][C] and [RD][C] with an int)
static int mvt_se_shape(const char* who, int B, int P, int C, int RD) {
  if (B < 0 || P < 1 || C < 4 || C % 4 != 0 || RD < 1 || (long)B * C > 0x7fffffffL || (long)RD * C > 0x7fffffffL) {
    btsbot_set_error("%s: bad shape B=%d P=%d C=%d RD=%d (C a multiple of 4)", who, B, P, C, RD);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

extern "C" int btsbot_op_mvt_se_fwd(const float* a2, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                                    const float* fc2_b, float* pool, float* rpre, float* r, float* gate, float* gated, int B,
                                    int P, int C, int RD, void* stream) {
  if (a2 == nullptr || fc1_w == nullptr || fc1_b == nullptr || fc2_w == nullptr || fc2_b == nullptr || pool == nullptr ||
      rpre == nullptr || r == nullptr || gate == nullptr || gated == nullptr)
    return mvt_bad("op_mvt_se_fwd", "null pointer");
  TRY(mvt_se_shape("op_mvt_se_fwd", B, P, C, RD));
  if (B == 0) return BTSBOT_OK;
  return launch_se_fwd(a2, fc1_w, fc1_b, fc2_w, fc2_b, pool, rpre, r, gate, gated, B, P, C, RD, (hipStream_t)stream);
}

extern "C" int btsbot_op_mvt_se_bwd(const float* d_gated, const float* a2, const float* pool, const float* rpre, const float* r,
                                    const float* gate, const float* fc1_w, const float* fc2_w, float* d_a2, float* d_fc1_w,
                                    float* d_fc1_b, float* d_fc2_w, float* d_fc2_b, int B, int P, int C, int RD, void* stream) {
  if (d_gated == nullptr || a2 == nullptr || pool == nullptr || rpre == nullptr || r == nullptr || gate == nullptr ||
      fc1_w == nullptr || fc2_w == nullptr || d_a2 == nullptr || d_fc1_w == nullptr || d_fc1_b == nullptr || d_fc2_w == nullptr ||
      d_fc2_b == nullptr)
    return mvt_bad("op_mvt_se_bwd", "null pointer");
  TRY(mvt_se_shape("op_mvt_se_bwd", B, P, C, RD));
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_mvt");
  const size_t bc = (size_t)B * C;
  const size_t o_dgate = sc.reserve(bc * 4), o_dr = sc.reserve((size_t)B * RD * 4), o_dpool = sc.reserve(bc * 4),
               o_dgpre = sc.reserve(bc * 4);
  TRY(sc.alloc());
  // (the engine's chain runs in place on d(gated))
  if (d_a2 != d_gated) HIP_TRY(hipMemcpyAsync(d_a2, d_gated, (size_t)B * P * C * 4, hipMemcpyDeviceToDevice, st));
  return launch_se_bwd(d_a2, a2, pool, rpre, r, gate, fc1_w, fc2_w, d_fc1_w, d_fc1_b, d_fc2_w, d_fc2_b, sc.at<float>(o_dgate), sc.at<float>(o_dr),
                       sc.at<float>(o_dpool), sc.at<float>(o_dgpre), B, P, C, RD, st);
}

extern "C" int btsbot_op_mvt_avgpool2_bwd(const float* g, float* dx, int B, int H, int C, int accumulate, void* stream) {
  if (g == nullptr || dx == nullptr) return mvt_bad("op_mvt_avgpool2_bwd", "null pointer");
  if (B < 0 || H < 2 || H % 2 != 0 || C < 1 || (accumulate != 0 && accumulate != 1)) {
    btsbot_set_error("op_mvt_avgpool2_bwd: bad shape B=%d H=%d C=%d accumulate=%d (H even)", B, H, C, accumulate);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  return launch_avgpool2_bwd(g, dx, B, H, C, accumulate, (hipStream_t)stream);
}

extern "C" int btsbot_op_mvt_col2im3(const float* dcol, float* din, int B, int H, int C, void* stream) {
  if (dcol == nullptr || din == nullptr) return mvt_bad("op_mvt_col2im3", "null pointer");
  if (B < 0 || H < 1 || C < 1) {
    btsbot_set_error("op_mvt_col2im3: bad shape B=%d H=%d C=%d", B, H, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  return launch_col2im3(dcol, din, B, H, C, (hipStream_t)stream);
}

extern "C" int btsbot_op_mvt_unpack_conv3_grad(const float* gp, float* g, int O, int C, int ldp, void* stream) {
  if (gp == nullptr || g == nullptr) return mvt_bad("op_mvt_unpack_conv3_grad", "null pointer");
  if (O < 1 || C < 1 || ldp < 9 * C || (long)O * C * 9 > 0x7fffffffL) {
    btsbot_set_error("op_mvt_unpack_conv3_grad: bad shape O=%d C=%d ldp=%d (ldp >= 9 C)", O, C, ldp);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_unpack_conv3_grad(gp, g, O, C, ldp, (hipStream_t)stream);
}

extern "C" int btsbot_op_mvt_gelu_fwd(const float* pre, float* out, int64_t n, void* stream) {
  if (pre == nullptr || out == nullptr) return mvt_bad("op_mvt_gelu_fwd", "null pointer");
  if (n < 0 || n % 4 != 0) return mvt_bad("op_mvt_gelu_fwd", "n is not a multiple of 4");
  if (n == 0) return BTSBOT_OK;
  return launch_gelu_fwd(pre, out, (long)(n / 4), (hipStream_t)stream);
}

extern "C" int btsbot_op_mvt_gelu_bwd(const float* pre, float* d, int64_t n, void* stream) {
  if (pre == nullptr || d == nullptr) return mvt_bad("op_mvt_gelu_bwd", "null pointer");
  if (n < 0 || n % 4 != 0) return mvt_bad("op_mvt_gelu_bwd", "n is not a multiple of 4");
  if (n == 0) return BTSBOT_OK;
  return launch_gelu_bwd(pre, d, (long)(n / 4), (hipStream_t)stream);
}

extern "C" int btsbot_op_mvt_bcast_set(const float* v, float* d, int B, int P, int C, float scale, void* stream) {
  if (v == nullptr || d == nullptr) return mvt_bad("op_mvt_bcast_set", "null pointer");
  if (B < 0 || P < 1 || C < 1) {
    btsbot_set_error("op_mvt_bcast_set: bad shape B=%d P=%d C=%d", B, P, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  return launch_bcast_set(d, v, B, P, C, scale, (hipStream_t)stream);
}
