// Op-level entry points of the classifier heads (include/btsbot_hip.h, btsbot_op_head*, btsbot_op_ht_*): the fused
// inference heads of head.hip / head16.hip on given rows, and the training kernels of head_train.hip one launcher at a
// time, on the caller's tensors and stream, for the per-kernel tests.  Nothing here is on the product path: forward.hip and
// head_train.hip call the same launchers.  Parameters arrive in state-dict layout, fp32; the operand images a handle keeps
// packed (K-major transposes, the BatchNorm fold, the split A fragments) are built in the call's own scratch by the
// launchers the handle uses.  Every entry point checks its arguments before it allocates or launches anything.
#include <string.h>

#include "common.h"
#include "head16.h"

namespace {

int head_bad(const char* who, const char* what) {
  btsbot_set_error("%s: %s", who, what);
  return BTSBOT_ERR_INVALID_ARG;
}
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool act_ok(int act) { return act == ACT_NONE || act == ACT_GELU || act == ACT_RELU; }
// the kernels index [M][N] with 32-bit element numbers
bool fits(long a, long b) { return a > 0 && b > 0 && a * b < (1L << 31); }

}  // namespace

extern "C" int btsbot_op_head16_supported(int prec, int feat_dim, int n_meta, int f1, int f2, int n_layers, const int* dims) {
  if (dims == nullptr || n_layers < 1 || n_layers > 3) return 0;
  return head16_supported(prec, feat_dim, n_meta, f1, f2, n_layers, dims) ? 1 : 0;
}

extern "C" int btsbot_op_head(int prec, const float* feat, int feat_dim, const float* hn_w, const float* hn_b,
                              const float* meta, int n_meta, const float* bn_w, const float* bn_b, const float* bn_rm,
                              const float* bn_rv, const float* m1_w, const float* m1_b, int f1, const float* m2_w,
                              const float* m2_b, int f2, int meta_trailing_act, int n_layers, const int* dims,
                              const float* const* comb_w, const float* const* comb_b, int act, float* logits, float* scores,
                              float* features, float* hidden, int B, void* stream) {
  const char* who = "op_head";
  if (prec != BTSBOT_F32 && prec != BTSBOT_BF16 && prec != BTSBOT_F16) return head_bad(who, "precision must be f32, bf16 or f16");
  if (dims == nullptr || comb_w == nullptr || comb_b == nullptr || logits == nullptr) return head_bad(who, "null pointer");
  if (n_layers < 1 || n_layers > 3) return head_bad(who, "n_layers must be 1, 2 or 3");
  if (feat_dim < 0 || n_meta < 0 || (feat_dim == 0 && n_meta == 0)) return head_bad(who, "neither an image feature nor metadata");
  if (feat_dim > 0 && feat == nullptr) return head_bad(who, "feat_dim > 0 without feat");
  if ((hn_w == nullptr) != (hn_b == nullptr) || (hn_w != nullptr && feat_dim == 0))
    return head_bad(who, "the head LayerNorm takes weight and bias, and an image feature");
  if (n_meta > 0) {
    if (meta == nullptr || bn_w == nullptr || bn_b == nullptr || bn_rm == nullptr || bn_rv == nullptr || m1_w == nullptr ||
        m1_b == nullptr || m2_w == nullptr || m2_b == nullptr)
      return head_bad(who, "n_meta > 0 with a null metadata-branch pointer");
    if (f1 < 1 || f2 < 1) return head_bad(who, "metadata widths must be positive");
  } else {
    f1 = f2 = 0;
  }
  if (!act_ok(act) || act == ACT_NONE) return head_bad(who, "activation must be GELU or ReLU");
  for (int i = 0; i <= n_layers; ++i)
    if (dims[i] < 1) return head_bad(who, "layer widths must be positive");
  for (int i = 0; i < n_layers; ++i)
    if (comb_w[i] == nullptr || comb_b[i] == nullptr) return head_bad(who, "null fusion-layer pointer");
  if (dims[0] != feat_dim + f2) {
    btsbot_set_error("op_head: dims[0] = %d is not the concat width %d + %d", dims[0], feat_dim, f2);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B < 0) return head_bad(who, "negative row count");
  hipStream_t st = (hipStream_t)stream;

  if (prec != BTSBOT_F32) {
    if (!head16_supported(prec, feat_dim, n_meta, f1, f2, n_layers, dims)) {
      // (the predicate decides; this only words the refusal)
      int wide = 0;
      for (int i = 1; i <= n_layers; ++i) wide = dims[i] > wide ? dims[i] : wide;
      wide = f1 > wide ? f1 : wide;
      wide = f2 > wide ? f2 : wide;
      if (feat_dim % 8 != 0 || feat_dim > 768)
        btsbot_set_error("op_head: head16 has no kernel for feature width %d (a multiple of 8, at most 768)", feat_dim);
      else if (n_meta > 32)
        btsbot_set_error("op_head: head16 has no kernel for n_meta %d (at most 32)", n_meta);
      else if (dims[n_layers] != 1)
        btsbot_set_error("op_head: head16 has no kernel for a last width of %d (1)", dims[n_layers]);
      else
        btsbot_set_error("op_head: head16 has no kernel for these layer widths (widest %d; one row tile per wave)", wide);
      return BTSBOT_ERR_INVALID_ARG;
    }
    if (B == 0) return BTSBOT_OK;
    StreamScratch sc(st, "op_head");   // BatchNorm fold | the split A fragments of every Linear
    size_t o_sc = 0, o_sh = 0, o_m1 = 0, o_m2 = 0, o_c[3] = {0, 0, 0};
    if (n_meta > 0) {
      o_sc = sc.reserve((size_t)n_meta * 4);
      o_sh = sc.reserve((size_t)n_meta * 4);
      o_m1 = sc.reserve(head16_packed_bytes(f1, n_meta));
      o_m2 = sc.reserve(head16_packed_bytes(f2, f1));
    }
    for (int i = 0; i < n_layers; ++i) o_c[i] = sc.reserve(head16_packed_bytes(dims[i + 1], dims[i]));
    TRY(sc.alloc());
    Head16Args g;
    memset(&g, 0, sizeof(g));
    g.feat = feat_dim > 0 ? feat : nullptr;
    g.feat_dim = feat_dim;
    g.hn_w = hn_w;
    g.hn_b = hn_b;
    if (n_meta > 0) {
      TRY(launch_bn_fold(bn_w, bn_b, bn_rm, bn_rv, sc.at<float>(o_sc), sc.at<float>(o_sh), n_meta, st));
      TRY(launch_pack_h16(prec, m1_w, sc.at<void>(o_m1), f1, n_meta, st));
      TRY(launch_pack_h16(prec, m2_w, sc.at<void>(o_m2), f2, f1, st));
      g.meta = meta;
      g.n_meta = n_meta;
      g.bn_scale = sc.at<float>(o_sc);
      g.bn_shift = sc.at<float>(o_sh);
      g.m1 = H16Layer{sc.at<void>(o_m1), m1_b, n_meta, f1, act};
      g.m2 = H16Layer{sc.at<void>(o_m2), m2_b, f1, f2, meta_trailing_act ? act : ACT_NONE};
    }
    g.n_layers = n_layers;
    for (int i = 0; i < n_layers; ++i) {
      TRY(launch_pack_h16(prec, comb_w[i], sc.at<void>(o_c[i]), dims[i + 1], dims[i], st));
      g.comb[i] = H16Layer{sc.at<void>(o_c[i]), comb_b[i], dims[i], dims[i + 1], i + 1 < n_layers ? act : ACT_NONE};
    }
    g.logits = logits;
    g.scores = scores;
    g.features = features;
    g.hidden = hidden;
    g.B = B;
    return launch_head16(prec, g, st);
  }

  if (dims[n_layers] != 1) return head_bad(who, "the last width must be 1 (one logit per row)");
  if (B == 0) return BTSBOT_OK;
  StreamScratch sc(st, "op_head");   // BatchNorm fold | the K-major transpose of every Linear
  size_t o_sc = 0, o_sh = 0, o_m1 = 0, o_m2 = 0, o_c[3] = {0, 0, 0};
  if (n_meta > 0) {
    o_sc = sc.reserve((size_t)n_meta * 4);
    o_sh = sc.reserve((size_t)n_meta * 4);
    o_m1 = sc.reserve((size_t)f1 * n_meta * 4);
    o_m2 = sc.reserve((size_t)f2 * f1 * 4);
  }
  for (int i = 0; i < n_layers; ++i) o_c[i] = sc.reserve((size_t)dims[i + 1] * dims[i] * 4);
  TRY(sc.alloc());
  HeadArgs a;
  memset(&a, 0, sizeof(a));
  a.feat = feat_dim > 0 ? feat : nullptr;
  a.feat_dim = feat_dim;
  a.hn_w = hn_w;
  a.hn_b = hn_b;
  if (n_meta > 0) {
    TRY(launch_bn_fold(bn_w, bn_b, bn_rm, bn_rv, sc.at<float>(o_sc), sc.at<float>(o_sh), n_meta, st));
    TRY(launch_transpose_f32(m1_w, sc.at<float>(o_m1), f1, n_meta, st));
    TRY(launch_transpose_f32(m2_w, sc.at<float>(o_m2), f2, f1, st));
    a.meta = meta;
    a.n_meta = n_meta;
    a.f1 = f1;
    a.f2 = f2;
    a.bn_scale = sc.at<float>(o_sc);
    a.bn_shift = sc.at<float>(o_sh);
    a.m1_wt = sc.at<float>(o_m1);
    a.m1_b = m1_b;
    a.m2_wt = sc.at<float>(o_m2);
    a.m2_b = m2_b;
    a.meta_act = act;
    a.meta_trailing_act = meta_trailing_act ? 1 : 0;
  }
  a.n_layers = n_layers;
  for (int i = 0; i <= n_layers; ++i) a.dims[i] = dims[i];
  for (int i = 0; i < n_layers; ++i) {
    TRY(launch_transpose_f32(comb_w[i], sc.at<float>(o_c[i]), dims[i + 1], dims[i], st));
    a.wt[i] = sc.at<float>(o_c[i]);
    a.b[i] = comb_b[i];
  }
  a.comb_act = act;
  a.logits = logits;
  a.scores = scores;
  a.features = features;
  a.hidden = hidden;
  a.B = B;
  return launch_head(a, st);
}

// ---- head_train.hip, one launcher at a time

extern "C" int btsbot_op_ht_lin_is_wide(int M, int N, int K, int ldi) {
  if (M < 1 || N < 1 || K < 1 || ldi < K) return head_bad("op_ht_lin_is_wide", "bad shape");
  return head_train_lin_is_wide(M, N, K, ldi) ? 1 : 0;
}

extern "C" int btsbot_op_ht_lin_fwd(const float* in, int ldi, const float* w, const float* bias, float* pre, float* outa,
                                    int ldo, int M, int N, int K, int act, const uint8_t* mask, float keep_scale,
                                    void* stream) {
  const char* who = "op_ht_lin_fwd";
  if (in == nullptr || w == nullptr || bias == nullptr || outa == nullptr) return head_bad(who, "null pointer");
  if (!fits(M, N) || K < 1 || ldi < K || ldo < N || !fits(N, K)) return head_bad(who, "bad shape (M, N, K >= 1, ldi >= K, ldo >= N)");
  if (!act_ok(act)) return head_bad(who, "bad activation");
  hipStream_t st = (hipStream_t)stream;
  const bool wide = head_train_lin_is_wide(M, N, K, ldi);
  if (wide && (!al16(in) || !al16(w) || !al16(pre))) return head_bad(who, "the wide path takes 16-byte aligned in, w and pre");
  StreamScratch sc(st, who);   // the K-major transpose | a pre-activation buffer for the wide path when the caller keeps none
  const size_t o_wt = sc.reserve((size_t)N * K * 4);
  const size_t o_pre = sc.reserve(wide && pre == nullptr ? (size_t)M * N * 4 : 0);
  TRY(sc.alloc());
  TRY(launch_transpose_f32(w, sc.at<float>(o_wt), N, K, st));
  return launch_ht_layer_fwd(in, ldi, w, sc.at<float>(o_wt), bias, wide && pre == nullptr ? sc.at<float>(o_pre) : pre, outa, ldo,
                             M, N, K, act, mask, keep_scale, st);
}

extern "C" int btsbot_op_ht_act_bwd(const float* dout, int ldd, const float* pre, float* dpre, int M, int N, int act,
                                    const uint8_t* mask, float keep_scale, void* stream) {
  const char* who = "op_ht_act_bwd";
  if (dout == nullptr || pre == nullptr || dpre == nullptr) return head_bad(who, "null pointer");
  if (!fits(M, N) || ldd < N) return head_bad(who, "bad shape (M, N >= 1, ldd >= N)");
  if (!act_ok(act)) return head_bad(who, "bad activation");
  return launch_ht_act_bwd(dout, ldd, pre, dpre, M, N, act, mask, keep_scale, (hipStream_t)stream);
}

extern "C" int btsbot_op_ht_lin_bwd_in(const float* dpre, const float* w, float* din, int ldi, int M, int N, int K,
                                       void* stream) {
  const char* who = "op_ht_lin_bwd_in";
  if (dpre == nullptr || w == nullptr || din == nullptr) return head_bad(who, "null pointer");
  if (!fits(M, K) || N < 1 || ldi < K || !fits(N, K) || !fits(M, N)) return head_bad(who, "bad shape (M, N, K >= 1, ldi >= K)");
  hipStream_t st = (hipStream_t)stream;
  if (ldi != K) return launch_ht_lin_bwd_in(dpre, w, din, ldi, M, N, K, st);   // (only the per-output kernel strides din)
  const bool wide = head_train_lin_is_wide(M, K, N, N);
  if (wide && (!al16(dpre) || !al16(din))) return head_bad(who, "the wide path takes 16-byte aligned dpre and din");
  StreamScratch sc(st, who);   // the transposed image [K][N] the wide path reads
  const size_t o_wt = sc.reserve((size_t)N * K * 4);
  TRY(sc.alloc());
  TRY(launch_transpose_f32(w, sc.at<float>(o_wt), N, K, st));
  return launch_ht_layer_bwd_in(dpre, w, sc.at<float>(o_wt), din, M, N, K, st);
}

extern "C" int btsbot_op_ht_lin_bwd_w_kind(const float* in, int ldi, const float* dw, int N, int K) {
  if (in == nullptr || dw == nullptr || N < 1 || K < 1 || ldi < K) return head_bad("op_ht_lin_bwd_w_kind", "bad argument");
  return head_train_lin_bwd_w_kind(in, ldi, dw, N, K);
}

extern "C" int btsbot_op_ht_lin_bwd_w(const float* dpre, const float* in, int ldi, float* dw, float* db, int M, int N, int K,
                                      void* stream) {
  const char* who = "op_ht_lin_bwd_w";
  if (dpre == nullptr || in == nullptr || dw == nullptr || db == nullptr) return head_bad(who, "null pointer");
  if (!fits(M, N) || K < 1 || ldi < K || !fits(M, ldi) || !fits(N, K + 1L)) return head_bad(who, "bad shape (M, N, K >= 1, ldi >= K)");
  return launch_ht_lin_bwd_w(dpre, in, ldi, dw, db, M, N, K, (hipStream_t)stream);
}

extern "C" int btsbot_op_ht_bn_fwd(const float* x, int M, int n, const float* w, const float* b, float* run_mean,
                                   float* run_var, float* xhat, float* out, float* rstd, void* stream) {
  const char* who = "op_ht_bn_fwd";
  if (x == nullptr || w == nullptr || b == nullptr || xhat == nullptr || out == nullptr || rstd == nullptr)
    return head_bad(who, "null pointer");
  if ((run_mean == nullptr) != (run_var == nullptr)) return head_bad(who, "running mean and variance come together");
  if (!fits(M, n)) return head_bad(who, "bad shape (M, n >= 1)");
  return launch_ht_bn_fwd(x, M, n, w, b, run_mean, run_var, xhat, out, rstd, (hipStream_t)stream);
}

extern "C" int btsbot_op_ht_bn_bwd(const float* dy, int M, int n, const float* w, const float* xhat, const float* rstd,
                                   float* dw, float* db, void* stream) {
  const char* who = "op_ht_bn_bwd";
  if (dy == nullptr || w == nullptr || xhat == nullptr || rstd == nullptr || dw == nullptr || db == nullptr)
    return head_bad(who, "null pointer");
  if (!fits(M, n)) return head_bad(who, "bad shape (M, n >= 1)");
  return launch_ht_bn_bwd(dy, M, n, w, xhat, rstd, dw, db, (hipStream_t)stream);
}

extern "C" int btsbot_op_ht_bn_eval_fwd(const float* x, int M, int n, const float* w, const float* b, const float* run_mean,
                                        const float* run_var, float* xhat, float* out, float* rstd, void* stream) {
  const char* who = "op_ht_bn_eval_fwd";
  if (x == nullptr || w == nullptr || b == nullptr || run_mean == nullptr || run_var == nullptr || xhat == nullptr ||
      out == nullptr || rstd == nullptr)
    return head_bad(who, "null pointer");
  if (!fits(M, n)) return head_bad(who, "bad shape (M, n >= 1)");
  return launch_ht_bn_eval_fwd(x, M, n, w, b, run_mean, run_var, xhat, out, rstd, (hipStream_t)stream);
}

extern "C" int btsbot_op_ht_bn_bwd_in(const float* dy, int M, int n, const float* w, const float* xhat, const float* rstd,
                                      const float* sum_dy, const float* sum_dyx, float* dx, int eval, void* stream) {
  const char* who = "op_ht_bn_bwd_in";
  if (dy == nullptr || w == nullptr || xhat == nullptr || rstd == nullptr || dx == nullptr) return head_bad(who, "null pointer");
  if (!eval && (sum_dy == nullptr || sum_dyx == nullptr)) return head_bad(who, "the batch-statistics form reads both column sums");
  if (!fits(M, n)) return head_bad(who, "bad shape (M, n >= 1)");
  return launch_ht_bn_bwd_in(dy, M, n, w, xhat, rstd, sum_dy, sum_dyx, dx, eval ? 1 : 0, (hipStream_t)stream);
}

extern "C" int btsbot_op_ht_feat_rows(const float* feat, int F, const float* hw, const float* hb, float* z, int ldz, int M,
                                      void* stream) {
  const char* who = "op_ht_feat_rows";
  if (feat == nullptr || z == nullptr) return head_bad(who, "null pointer");
  if ((hw == nullptr) != (hb == nullptr)) return head_bad(who, "the LayerNorm takes weight and bias");
  if (!fits(M, F) || ldz < F || !fits(M, ldz)) return head_bad(who, "bad shape (M, F >= 1, ldz >= F)");
  return launch_ht_feat_rows(feat, F, hw, hb, z, ldz, M, (hipStream_t)stream);
}

extern "C" int btsbot_op_ht_logits(const float* in, float* logits, float* scores, int M, void* stream) {
  if (in == nullptr || logits == nullptr) return head_bad("op_ht_logits", "null pointer");
  if (M < 1) return head_bad("op_ht_logits", "bad row count");
  return launch_ht_logits(in, logits, scores, M, (hipStream_t)stream);
}

extern "C" int btsbot_op_ht_copy_cols(float* dst, int ldd, const float* src, int lds, int cols, int M, void* stream) {
  const char* who = "op_ht_copy_cols";
  if (dst == nullptr || src == nullptr) return head_bad(who, "null pointer");
  if (!fits(M, cols) || ldd < cols || lds < cols || !fits(M, ldd) || !fits(M, lds)) return head_bad(who, "bad shape (ldd, lds >= cols >= 1)");
  return launch_ht_copy_cols(dst, ldd, src, lds, cols, M, (hipStream_t)stream);
}
