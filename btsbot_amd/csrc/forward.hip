// The inference forward of the C ABI: the ConvNeXt schedule of one chunk (backbone_chunk; MaxViT handles: maxvit.hip), the
// heads, chunking, and btsbot_forward / btsbot_forward_embed / btsbot_read_tap.
#include <string.h>

#include "ctx.h"
#include "maxvit.h"
#include "stage0.h"
#include "stage2p.h"
#include "stage3.h"
#include "head16.h"

// a stage kernel's per-workgroup wall-clock region: nullptr without a stamp buffer or when `grid` workgroups do not fit
static unsigned long long* stamp_wgt(const btsbot_ctx* h, size_t off, int max_wg, int grid) {
  return h->stamps != nullptr && grid <= max_wg ? h->stamps + off : nullptr;
}

// image branch of one chunk; *feat_out = [nb][dims[3]] fp32 features inside the workspace
int backbone_chunk(btsbot_ctx* h, const float* img, int nb, hipStream_t st, float** feat_out) {
  const btsbot_config& c = h->cfg;
  const float* m = h->mirror;
  float* x = reinterpret_cast<float*>(h->ws + h->o_x);
  float* x2 = reinterpret_cast<float*>(h->ws + h->o_x2);
  void* xn = h->ws + h->o_xn;
  void* hb = h->ws + h->o_h;
  if (h->is_maxvit) return maxvit_chunk(h, img, nb, st, feat_out);
  if (h->has_image) {
    const Schedule& sc = h->sched;
    if (sc.stage0) {
      Stage0Args a;
      TRY(stage0_args(h, false, &a));
      a.img = img;
      a.out = x;
      a.tap_stem = h->debug ? h->taps[0] : nullptr;
      a.tap_stage = h->debug ? h->taps[1] : nullptr;
      a.B = nb;
      a.diag = sc.s0_diag;
      a.stamps = h->stamps ? h->stamps + STAMP_S0 : nullptr;
      a.wgt = stamp_wgt(h, STAMP_S0_WG, STAMP_S0_MAX_WG, nb);
      TRY(timed(h, CAT_STAGE0, st, [&] {
        return launch_stage0b(h->prec_s01(), a, st);
      }));
    } else {
      TRY(timed(h, CAT_STEM, st, [&] {
        if (sc.stem16)
          return launch_stem16(c.precision, img, m + h->stem_w, m + h->stem_b, m + h->stem_lnw, m + h->stem_lnb, x, nb,
                               c.dims[0], st);
        return launch_stem(img, m + h->stem_w, m + h->stem_b, m + h->stem_lnw, m + h->stem_lnb, x,
                           nb, c.dims[0], st);
      }));
      if (h->debug)
        HIP_TRY(hipMemcpyAsync(h->taps[0], x, (size_t)nb * 225 * c.dims[0] * 4,
                               hipMemcpyDeviceToDevice, st));
    }
    bool down_done = sc.stage0;      // the previous stage's kernel already applied stage i's downsample
    for (int i = sc.stage0 ? 1 : 0; i < 4; ++i) {
      const int ch = c.dims[i], hw = STAGE_HW[i], rows = nb * hw * hw;
      if (i > 0 && !down_done) {
        const int cin = c.dims[i - 1];
        TRY(timed(h, CAT_LNPATCH, st, [&] {
          return launch_ln_patch(c.precision, x, m + h->down[i].ln_w, m + h->down[i].ln_b, xn, nb,
                                 STAGE_HW[i - 1], cin, st);
        }));
        TRY(timed(h, CAT_DOWN, st, [&] {
          return launch_gemm(c.precision, EPI_BIAS, xn, IMG(h, h->down[i].p_w),
                             m + h->down[i].b, nullptr, nullptr, x2, rows, ch, 4 * cin, st);
        }));
        float* t = x;
        x = x2;
        x2 = t;
      }
      down_done = false;
      if (i == 1 && sc.stage1) {
        Stage1Args a;
        TRY(stage1_args(h, false, &a));
        a.x_in = x;
        a.out = x2;
        a.scratch = x2 + (((size_t)nb * 9 * c.dims[2] + 63) / 64) * 64;   // behind the output rows (x2 holds 225 * 64 floats per alert)
        a.tap_stage = h->debug ? h->taps[2] : nullptr;
        a.B = nb;
        a.diag = sc.s0_diag;
        a.stamps = h->stamps ? h->stamps + STAMP_S1 : nullptr;
        a.wgt = stamp_wgt(h, STAMP_S1_WG, STAMP_S1_MAX_WG, (nb + 1) / 2);
        TRY(timed(h, CAT_STAGE1, st, [&] {
          return launch_stage1b(h->prec_s01(), a, sc.s1_g5, st);
        }));
        float* t = x;
        x = x2;
        x2 = t;
        down_done = true;
        continue;
      }
      if (i == 2 && sc.stage2p) {
        // every block of the 3x3 stage and the last downsample in one launch: x [nb][9][256] -> x2 [nb][512]
        Stage2pArgs a;
        TRY(stage2p_args(h, false, &a));
        a.x_in = x;
        a.out = x2;
        a.tap_stage = h->debug ? h->taps[3] : nullptr;
        a.B = nb;
        a.diag = sc.s2p_diag;
        a.stamps = h->stamps ? h->stamps + STAMP_S2 : nullptr;
        TRY(timed(h, CAT_STAGE2, st, [&] { return launch_stage2p(h->prec_tail(), a, st); }));
        float* t = x;
        x = x2;
        x2 = t;
        down_done = true;
        continue;
      }
      if (i == 3 && hw == 1 && sc.stage3) {
        // the 1x1 stage: two launches per block, x updated in place
        Stage3Args a;
        TRY(stage3_args(h, &a));
        a.x = x;
        a.hfrag = hb;
        a.B = nb;
        a.stamps = h->stamps ? h->stamps + STAMP_S3 : nullptr;
        for (int j = 0; j < a.depth; ++j) {
          TRY(timed(h, CAT_S3FC1, st, [&] { return launch_stage3(h->prec_tail(), ch, a, j, 0, sc.s3_wide, st); }));
          TRY(timed(h, CAT_S3FC2, st, [&] { return launch_stage3(h->prec_tail(), ch, a, j, 1, sc.s3_wide, st); }));
        }
        if (h->debug)
          HIP_TRY(hipMemcpyAsync(h->taps[4], x, (size_t)rows * ch * 4, hipMemcpyDeviceToDevice, st));
        continue;
      }
      for (const BlockPk& b : h->blocks[i]) {
        TRY(timed(h, CAT_DWLN, st, [&] {
          return launch_dwconv_ln(c.precision, x, IMG_F32(h, b.p_dw), m + b.dw_b, m + b.ln_w, m + b.ln_b, xn, nb, hw,
                                  ch, st);
        }));
        if (sc.fused_mlp[i]) {
          TRY(timed(h, CAT_FUSED, st, [&] {
            return launch_fused_mlp(c.precision, ch, xn, IMG(h, b.p_fused), m + b.fc1_b,
                                    m + b.fc2_b, m + b.gamma, x, rows, st);
          }));
          continue;
        }
        TRY(timed(h, CAT_FC1, st, [&] {
          return launch_gemm(c.precision, EPI_GELU, xn, IMG(h, b.p_fc1), m + b.fc1_b, nullptr,
                             nullptr, hb, rows, 4 * ch, ch, st);
        }));
        TRY(timed(h, CAT_FC2, st, [&] {
          return launch_gemm(c.precision, EPI_RESID, hb, IMG(h, b.p_fc2), m + b.fc2_b,
                             m + b.gamma, x, x, rows, ch, 4 * ch, st);
        }));
      }
      if (h->debug)
        HIP_TRY(hipMemcpyAsync(h->taps[i + 1], x, (size_t)rows * ch * 4, hipMemcpyDeviceToDevice,
                               st));   // (stage 0's tap is written by the megakernel when fused)
    }
  }
  *feat_out = x;
  return BTSBOT_OK;
}

// `features` / `hidden`: the embedding outputs of btsbot_forward_embed (nullptr: the scoring call)
static int forward_chunk(btsbot_ctx* h, const float* img, const float* meta, float* logits,
                         float* scores, float* features, float* hidden, int nb, hipStream_t st) {
  const btsbot_config& c = h->cfg;
  const float* m = h->mirror;
  float* x = nullptr;
  if (h->has_image) TRY(backbone_chunk(h, img, nb, st, &x));
  if (h->sched.head16) {
    Head16Args g;
    memset(&g, 0, sizeof(g));
    g.feat = h->has_image ? x : nullptr;
    g.feat_dim = h->has_image ? c.dims[3] : 0;
    g.hn_w = h->hn_w >= 0 ? m + h->hn_w : nullptr;
    g.hn_b = h->hn_b >= 0 ? m + h->hn_b : nullptr;
    if (h->has_meta) {
      g.meta = meta;
      g.n_meta = c.n_meta;
      g.bn_scale = IMG_F32(h, h->p_bn_scale);
      g.bn_shift = IMG_F32(h, h->p_bn_shift);
      g.m1 = H16Layer{IMG(h, h->p_m1h), m + h->m1_b, c.n_meta, c.meta_fc1, h->act};
      g.m2 = H16Layer{IMG(h, h->p_m2h), m + h->m2_b, c.meta_fc1, c.meta_fc2, h->meta_trailing_act ? h->act : ACT_NONE};
    }
    g.n_layers = h->n_comb;
    for (int i = 0; i < h->n_comb; ++i)
      g.comb[i] = H16Layer{IMG(h, h->p_combh[i]), m + h->comb_b[i], h->comb_dims[i], h->comb_dims[i + 1],
                           i + 1 < h->n_comb ? h->act : ACT_NONE};
    g.logits = logits;
    g.scores = scores;
    g.features = features;
    g.hidden = hidden;
    g.B = nb;
    g.stamps = h->stamps ? h->stamps + STAMP_HEAD16 : nullptr;
    TRY(timed(h, CAT_HEAD16, st, [&] { return launch_head16(h->prec_head(), g, st); }));
    h->last_chunk = nb;
    return BTSBOT_OK;
  }
  HeadArgs a;
  memset(&a, 0, sizeof(a));
  a.feat = h->has_image ? x : nullptr;
  a.feat_dim = h->has_image ? c.dims[3] : 0;
  a.hn_w = h->hn_w >= 0 ? m + h->hn_w : nullptr;
  a.hn_b = h->hn_b >= 0 ? m + h->hn_b : nullptr;
  if (h->has_meta) {
    a.meta = meta;
    a.n_meta = c.n_meta;
    a.f1 = c.meta_fc1;
    a.f2 = c.meta_fc2;
    a.bn_scale = IMG_F32(h, h->p_bn_scale);
    a.bn_shift = IMG_F32(h, h->p_bn_shift);
    a.m1_wt = IMG_F32(h, h->p_m1);
    a.m1_b = m + h->m1_b;
    a.m2_wt = IMG_F32(h, h->p_m2);
    a.m2_b = m + h->m2_b;
    a.meta_act = h->act;
    a.meta_trailing_act = h->meta_trailing_act;
  }
  a.n_layers = h->n_comb;
  for (int i = 0; i <= h->n_comb; ++i) a.dims[i] = h->comb_dims[i];
  for (int i = 0; i < h->n_comb; ++i) {
    a.wt[i] = IMG_F32(h, h->p_comb[i]);
    a.b[i] = m + h->comb_b[i];
  }
  a.comb_act = h->act;
  a.logits = logits;
  a.scores = scores;
  a.features = features;
  a.hidden = hidden;
  a.B = nb;
  a.diag = h->sched.head_diag;
  TRY(timed(h, CAT_HEAD, st, [&] { return launch_head(a, st); }));
  h->last_chunk = nb;
  return BTSBOT_OK;
}

// btsbot_forward and btsbot_forward_embed: preconditions, chunking and stream rules in one place
static int forward_all(btsbot_ctx* h, const char* who, const float* triplets, const float* meta, float* logits,
                       float* scores, float* features, float* hidden, int batch, void* stream) {
  if (h == nullptr || logits == nullptr || batch < 0) {
    btsbot_set_error("%s: NULL handle/logits or negative batch", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!h->packed || !h->packed_full) {
    btsbot_set_error(h->packed ? "%s: the last pack was btsbot_pack_params_train(); call "
                                 "btsbot_pack_params() before an inference forward"
                               : "%s: btsbot_pack_params() has not been called", who);
    return BTSBOT_ERR_STATE;
  }
  if ((h->has_image && triplets == nullptr) || (h->has_meta && meta == nullptr)) {
    btsbot_set_error("%s: this wiring needs %s input", who,
                     h->has_image && triplets == nullptr ? "image" : "metadata");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (batch == 0) return BTSBOT_OK;
  if (h->ws == nullptr || h->max_chunk < 1) {
    btsbot_set_error("%s: btsbot_reserve() has not been called", who);
    return BTSBOT_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  TRY(pack_sync(h, st));
  const size_t wf = h->comb_dims[0], wh = h->comb_dims[h->n_comb - 1];   // btsbot_embed_width
  for (int b0 = 0; b0 < batch; b0 += h->max_chunk) {
    const int nb = batch - b0 < h->max_chunk ? batch - b0 : h->max_chunk;
    TRY(forward_chunk(h, triplets ? triplets + (size_t)b0 * 3 * 63 * 63 : nullptr,
                      meta ? meta + (size_t)b0 * h->cfg.n_meta : nullptr, logits + b0,
                      scores ? scores + b0 : nullptr, features ? features + b0 * wf : nullptr,
                      hidden ? hidden + b0 * wh : nullptr, nb, st));
  }
  return BTSBOT_OK;
}

extern "C" int btsbot_forward(btsbot_handle h, const float* triplets, const float* meta,
                              float* logits, float* scores, int batch, int training,
                              uint64_t dropout_seed, void* stream) {
  (void)dropout_seed;
  if (h != nullptr && logits != nullptr && batch >= 0 && training) {
    TRY(forward_all(h, "forward", triplets, meta, logits, scores, nullptr, nullptr, 0, stream));   // (its other refusals first)
    btsbot_set_error("forward: for training mode call btsbot_forward_train() (explicit dropout "
                     "keep-masks, BatchNorm batch statistics)");
    return BTSBOT_ERR_STATE;
  }
  return forward_all(h, "forward", triplets, meta, logits, scores, nullptr, nullptr, batch, stream);
}

extern "C" int btsbot_embed_width(btsbot_handle h, int which) {
  if (h == nullptr || (which != BTSBOT_EMBED_FEATURES && which != BTSBOT_EMBED_HIDDEN)) {
    btsbot_set_error("embed_width: NULL handle or unknown embedding %d", which);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return which == BTSBOT_EMBED_FEATURES ? h->comb_dims[0] : h->comb_dims[h->n_comb - 1];
}

extern "C" int btsbot_forward_embed(btsbot_handle h, const float* triplets, const float* meta, float* logits,
                                    float* scores, float* features, float* hidden, int batch, void* stream) {
  return forward_all(h, "forward_embed", triplets, meta, logits, scores, features, hidden, batch, stream);
}

extern "C" int64_t btsbot_read_tap(btsbot_handle h, const char* name, float* dst,
                                   int64_t capacity, void* stream) {
  if (h == nullptr || name == nullptr || dst == nullptr) {
    btsbot_set_error("read_tap: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!h->debug || h->taps[0] == nullptr || !h->has_image) {
    btsbot_set_error("read_tap: debug taps are off (btsbot_set_debug + btsbot_reserve first)");
    return BTSBOT_ERR_STATE;
  }
  int idx = -1;
  if (strcmp(name, "stem") == 0) idx = 0;
  else if (strncmp(name, "stage", 5) == 0 && name[5] >= '0' && name[5] <= '3' && name[6] == 0)
    idx = 1 + (name[5] - '0');
  if (idx < 0) {
    btsbot_set_error("read_tap: unknown tap '%s'", name);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int st_i = idx == 0 ? 0 : idx - 1;
  const int thw = h->is_maxvit ? (idx == 0 ? 112 : 56 >> st_i) : STAGE_HW[st_i];
  const int64_t n = (int64_t)h->last_chunk * thw * thw * h->cfg.dims[st_i];
  if (n > capacity) {
    btsbot_set_error("read_tap: need %lld floats, capacity %lld", (long long)n,
                     (long long)capacity);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipError_t e = hipMemcpyAsync(dst, h->taps[idx], (size_t)n * 4, hipMemcpyDeviceToDevice,
                                (hipStream_t)stream);
  if (e != hipSuccess) {
    btsbot_set_error("read_tap: %s", hipGetErrorString(e));
    return BTSBOT_ERR_HIP;
  }
  return n;
}
