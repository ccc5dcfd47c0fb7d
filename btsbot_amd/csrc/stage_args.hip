// Argument blocks of the ConvNeXt stage kernels (stage0.h, stage2p.h, stage3.h), shared by the inference forward
// (forward.hip: backbone_chunk) and the training forward (backbone_train.hip): the parameter pointers of every block and
// downsample.  The callers add their buffers, taps, stamps and the keeping form's keep_* / train.  BTSBOT_ERR_STATE:
// the handle has no such operand image (ctx.h: IMG).
#include <string.h>

#include "ctx.h"
#include "stage0.h"
#include "stage2p.h"
#include "stage3.h"

namespace {

// hid16: stage0b.hip's bf16 inference form takes gamma * W2 as f16 (its hidden type); the keeping form and stage 1 the bf16 image
int s01_blk(const btsbot_ctx* h, const BlockPk& b, bool keep, bool hid16, Stage0Blk* out) {
  const float* m = h->mirror;
  const bool x2 = h->x2 && !keep;
  Stage0Blk& k = *out;
  k.dw_w = IMG_F32(h, b.p_dw);
  k.dw_b = m + b.dw_b;
  k.ln_w = m + b.ln_w;
  k.ln_b = m + b.ln_b;
  k.b1 = m + b.fc1_b;
  k.b2 = m + b.fc2_b;
  k.gamma = m + b.gamma;
  k.w1 = x2 ? IMG(h, b.p_x2_w1) : IMG(h, b.p_fc1);
  k.par = keep ? IMG(h, b.p_s0par_t) : IMG(h, b.p_s0par);
  k.w2g = x2 ? IMG(h, b.p_x2_w2g) : hid16 ? IMG(h, b.p_fc2g_h) : IMG(h, b.p_fc2g);
  k.w1_lo = x2 ? IMG(h, b.p_x2_w1lo) : nullptr;
  k.w2g_lo = x2 ? IMG(h, b.p_x2_w2glo) : nullptr;
  return BTSBOT_OK;
}

}  // namespace

int stage0_args(const btsbot_ctx* h, bool keep, Stage0Args* out) {
  const float* m = h->mirror;
  const bool x2 = h->x2 && !keep;
  const DownPk& d = h->down[1];
  Stage0Args& a = *out;
  memset(&a, 0, sizeof(a));
  a.stem_w = x2 ? IMG(h, h->p_x2_stem) : IMG(h, h->p_stem16);
  a.stem_w_lo = x2 ? IMG(h, h->p_x2_stemlo) : nullptr;
  a.stem_b = m + h->stem_b;
  a.stem_lnw = m + h->stem_lnw;
  a.stem_lnb = m + h->stem_lnb;
  for (int j = 0; j < 2; ++j) {
    const int s = s01_blk(h, h->blocks[0][j], keep, !keep && h->prec_s01() == BTSBOT_BF16, &a.blk[j]);
    if (s != BTSBOT_OK) return s;
  }
  a.ds_lnw = m + d.ln_w;
  a.ds_lnb = m + d.ln_b;
  a.ds_w = x2 ? IMG(h, d.p_x2_w) : IMG(h, d.p_w);
  a.ds_w_lo = x2 ? IMG(h, d.p_x2_wlo) : nullptr;
  a.ds_b = m + d.b;
  return BTSBOT_OK;
}

int stage1_args(const btsbot_ctx* h, bool keep, Stage1Args* out) {
  const float* m = h->mirror;
  const DownPk& d = h->down[2];
  Stage1Args& a = *out;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < 2; ++j) {
    const int s = s01_blk(h, h->blocks[1][j], keep, false, &a.blk[j]);
    if (s != BTSBOT_OK) return s;
  }
  a.ds_lnw = m + d.ln_w;
  a.ds_lnb = m + d.ln_b;
  a.ds_w = IMG(h, d.p_wp);   // (split mode: heads and remainders in one fragment image)
  a.ds_b = m + d.b;
  return BTSBOT_OK;
}

int stage2p_args(const btsbot_ctx* h, bool keep, Stage2pArgs* out) {
  const float* m = h->mirror;
  const DownPk& d = h->down[3];
  Stage2pArgs& a = *out;
  memset(&a, 0, sizeof(a));
  a.depth = (int)h->blocks[2].size();
  for (int j = 0; j < a.depth; ++j) {
    const BlockPk& b = h->blocks[2][j];
    Stage2pBlk& k = a.blk[j];
    k.dw_w = IMG_F32(h, b.p_dw);
    k.dw_b = m + b.dw_b;
    k.ln_w = m + b.ln_w;
    k.ln_b = m + b.ln_b;
    k.b1 = m + b.fc1_b;
    k.b2 = m + b.fc2_b;
    k.gamma = m + b.gamma;
    k.w1p = IMG(h, b.p_w1p);
    k.w2p = IMG(h, b.p_w2p);
    k.scales = h->fp8 && !keep ? IMG_F32(h, b.p_scales) : nullptr;
  }
  a.ds_lnw = m + d.ln_w;
  a.ds_lnb = m + d.ln_b;
  a.ds_wp = IMG(h, d.p_wp);
  a.ds_b = m + d.b;
  a.cw = h->cfg.dims[2];
  a.alerts_hint = h->sched.s2p_alerts;
  return BTSBOT_OK;
}

int stage3_args(const btsbot_ctx* h, Stage3Args* out) {
  const float* m = h->mirror;
  const int ch = h->cfg.dims[3];
  Stage3Args& a = *out;
  memset(&a, 0, sizeof(a));
  a.depth = (int)h->blocks[3].size();
  for (int j = 0; j < a.depth; ++j) {
    const BlockPk& b = h->blocks[3][j];
    Stage3Blk& k = a.blk[j];
    k.dw_c = IMG_F32(h, b.p_dw) + 24 * ch;   // tap-major [49][C]: the centre row
    k.dw_b = m + b.dw_b;
    k.ln_w = m + b.ln_w;
    k.ln_b = m + b.ln_b;
    k.w1p = IMG(h, b.p_w1p);
    k.b1 = m + b.fc1_b;
    k.w2p = IMG(h, b.p_w2p);
    k.b2 = m + b.fc2_b;
    k.gamma = m + b.gamma;
    k.scales = h->fp8 ? IMG_F32(h, b.p_scales) : nullptr;
  }
  return BTSBOT_OK;
}
