// Op-level entry points of the MLP half of the ConvNeXt 16-bit training step (include/btsbot_hip.h, btsbot_op_cnt_*):
// the launchers of mlp_bwd.hip, s2mlp_bwd.hip, fused_mlp.hip and fc2_grads (ln_dw_bwd.hip) one at a time, on the caller's
// tensors and stream, for the per-kernel tests.  Nothing here is on the product path: backbone_train.hip calls the same
// launchers.  Every entry point checks its arguments before it allocates or launches anything; what its launcher has no
// kernel for comes back as BTSBOT_ERR_INVALID_ARG with a message.
#include "common.h"

namespace {

constexpr int ROWS_MAX = 1 << 30;   // row counts the kernels' 32-bit row arithmetic (tile * 64 + row, + a grid stride) holds

int mlp_bad(const char* who, const char* what) {
  btsbot_set_error("%s: %s", who, what);
  return BTSBOT_ERR_INVALID_ARG;
}
// the kernels move rows in 16-byte pieces
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int btsbot_op_cnt_mlp_bwd_planes(int C) {
  if (C != 64 && C != 128) return mlp_bad("op_cnt_mlp_bwd_planes", "no kernel for this width (64 or 128)");
  return mlp_bwd_planes(C);
}
extern "C" int btsbot_op_cnt_mlp_bwd_slices(int C, int R) {
  if ((C != 64 && C != 128) || R < 0 || R > ROWS_MAX) return mlp_bad("op_cnt_mlp_bwd_slices", "no kernel for this width, or bad R");
  return R == 0 ? 0 : mlp_bwd_slices(C, R);
}
extern "C" int btsbot_op_cnt_s2mlp_bwd_rows(void) { return s2mlp_bwd_rows(); }

extern "C" int btsbot_op_cnt_mlp_bwd(int prec, int C, const void* xn, const void* dy, const void* w1, const void* w2g,
                                     const float* b1, float* dxn, float* G, float* S, float* dW1, float* db1, int R,
                                     int deterministic, void* stream) {
  if (xn == nullptr || dy == nullptr || w1 == nullptr || w2g == nullptr || b1 == nullptr || dxn == nullptr || G == nullptr ||
      S == nullptr || dW1 == nullptr || db1 == nullptr)
    return mlp_bad("op_cnt_mlp_bwd", "null pointer");
  if (!mlp_bwd_supported(prec, C)) {
    btsbot_set_error("op_cnt_mlp_bwd: no kernel for precision %d at %d channels (bf16 / f16; 64 or 128)", prec, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (R < 0 || R > ROWS_MAX) return mlp_bad("op_cnt_mlp_bwd", "bad row count (0 .. 2^30)");
  if (!al16(xn) || !al16(dy) || !al16(w1) || !al16(w2g)) return mlp_bad("op_cnt_mlp_bwd", "operand tensors must be 16-byte aligned");
  if (R == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int gx = mlp_bwd_slices(C, R);
  StreamScratch sc(st, "op_cnt");   // partial filter-gradient tiles | the deterministic mode's partial rows
  const size_t o_part = sc.reserve(mlp_bwd_part_floats(C, R) * 4);
  // (det_alloc hands out multiples of 64 floats: one partial row per slice for db1 [4 C] and one for colsum(dy) [C])
  const size_t det_floats = deterministic ? ((size_t)gx * 4 * C + 63) / 64 * 64 + ((size_t)gx * C + 63) / 64 * 64 : 0;
  const size_t o_det = sc.reserve(det_floats * 4);
  TRY(sc.alloc());
  WgradReduceJob jobs[2];
  (void)det_fell_short();
  if (deterministic) det_begin(sc.at<float>(o_det), det_floats);
  int rc = launch_mlp_bwd(prec, C, xn, dy, w1, w2g, b1, dxn, sc.at<float>(o_part), G, S, dW1, db1, R, st, jobs);
  if (rc == BTSBOT_OK) rc = launch_wgrad_reduce(jobs, 2, st);
  if (deterministic) det_end();
  if (det_fell_short() && rc == BTSBOT_OK) {
    btsbot_set_error("op_cnt_mlp_bwd: the deterministic mode's scratch (%zu floats for %d slices) fell short", det_floats, gx);
    return BTSBOT_ERR_STATE;
  }
  return rc;
}

extern "C" int btsbot_op_cnt_s2mlp_bwd(int prec, int C, const void* dy, const void* a, const void* w2gt, const void* w1t,
                                       void* da, float* dxn, int R, void* stream) {
  if (dy == nullptr || a == nullptr || w2gt == nullptr || w1t == nullptr || da == nullptr || dxn == nullptr)
    return mlp_bad("op_cnt_s2mlp_bwd", "null pointer");
  if (!s2mlp_bwd_supported(prec, C)) {
    btsbot_set_error("op_cnt_s2mlp_bwd: no kernel for precision %d at %d channels (bf16 / f16; 256)", prec, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  // (da is addressed with 32-bit byte offsets: R + 48 rows of 2 KiB)
  if (R < 0 || R > (1 << 20) - 48) return mlp_bad("op_cnt_s2mlp_bwd", "bad row count (0 .. 2^20 - 48)");
  if (!al16(dy) || !al16(a) || !al16(da) || !al16(dxn)) return mlp_bad("op_cnt_s2mlp_bwd", "dy, a, da and dxn must be 16-byte aligned");
  if (R == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int H = 4 * C;
  StreamScratch sc(st, "op_cnt");   // both filters as MFMA A fragments
  const size_t o_w2 = sc.reserve((size_t)H * C * 2), o_w1 = sc.reserve((size_t)C * H * 2);
  TRY(sc.alloc());
  TRY(launch_pack_frag16(w2gt, sc.at<void>(o_w2), H, C, st));
  TRY(launch_pack_frag16(w1t, sc.at<void>(o_w1), C, H, st));
  return launch_s2mlp_bwd(prec, dy, a, sc.at<void>(o_w2), sc.at<void>(o_w1), da, dxn, R, st);
}

extern "C" int btsbot_op_cnt_fused_mlp(int prec, int C, const void* xn, const float* w1, const float* w2, const float* b1,
                                       const float* b2, const float* gamma, const float* xres, float* x, int M, void* stream) {
  if (xn == nullptr || w1 == nullptr || w2 == nullptr || b1 == nullptr || b2 == nullptr || gamma == nullptr || x == nullptr)
    return mlp_bad("op_cnt_fused_mlp", "null pointer");
  if (!fused_mlp_supported(prec, C)) {
    btsbot_set_error("op_cnt_fused_mlp: no kernel for precision %d at %d channels (bf16 / f16; 64, 80, 128 or 160)", prec, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (M < 0 || M > ROWS_MAX) return mlp_bad("op_cnt_fused_mlp", "bad row count (0 .. 2^30)");
  if (!al16(xn) || !al16(b2) || !al16(gamma) || !al16(xres) || !al16(x))
    return mlp_bad("op_cnt_fused_mlp", "xn, b2, gamma, xres and x must be 16-byte aligned");
  if (M == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamScratch sc(st, "op_cnt");   // the packed filter image
  const size_t o_pk = sc.reserve(fused_mlp_packed_bytes(C));
  TRY(sc.alloc());
  TRY(launch_pack_fused_mlp(prec, C, w1, w2, sc.at<void>(o_pk), st));
  return launch_fused_mlp(prec, C, xn, sc.at<void>(o_pk), b1, b2, gamma, x, M, st, nullptr, nullptr, nullptr, 0, xres);
}

extern "C" int btsbot_op_cnt_fc2_grads(float* G, float* S, const float* w2, const float* b2, const float* gamma, float* dW2,
                                       float* db2, float* dgamma, int C, int H, void* stream) {
  if (G == nullptr || S == nullptr || w2 == nullptr || b2 == nullptr || gamma == nullptr || dW2 == nullptr || db2 == nullptr ||
      dgamma == nullptr)
    return mlp_bad("op_cnt_fc2_grads", "null pointer");
  if (C < 1 || H < 1 || C > 65535) {
    btsbot_set_error("op_cnt_fc2_grads: bad shape C=%d H=%d (1 <= C <= 65535, H >= 1)", C, H);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_fc2_grads(G, S, w2, b2, gamma, dW2, db2, dgamma, C, H, (hipStream_t)stream);
}
