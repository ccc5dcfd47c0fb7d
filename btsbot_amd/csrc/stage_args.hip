// Argument blocks of the ConvNeXt stage kernels (stage0.h, stage2p.h, stage3.h), shared by the inference forward
// (api.hip: backbone_chunk) and the training forward (backbone_train.hip): the parameter pointers of every block and
// downsample.  The callers add their buffers, taps, stamps and the keeping form's keep_* / train.
#include <string.h>

#include "ctx.h"
#include "stage0.h"
#include "stage2p.h"
#include "stage3.h"

namespace {

Stage0Blk s01_blk(const btsbot_ctx* h, const BlockPk& b, bool keep) {
  const float* m = h->mirror;
  const bool x2 = h->x2 && !keep;
  Stage0Blk k;
  k.dw_w = reinterpret_cast<const float*>(h->extra + b.p_dw);
  k.dw_b = m + b.dw_b;
  k.ln_w = m + b.ln_w;
  k.ln_b = m + b.ln_b;
  k.b1 = m + b.fc1_b;
  k.b2 = m + b.fc2_b;
  k.gamma = m + b.gamma;
  k.w1 = h->extra + (x2 ? b.p_x2_w1 : b.p_fc1);
  k.par = h->extra + (keep ? b.p_s0par_t : b.p_s0par);
  k.w2g = h->extra + (x2 ? b.p_x2_w2g : b.p_fc2g);
  k.w1_lo = x2 ? h->extra + b.p_x2_w1lo : nullptr;
  k.w2g_lo = x2 ? h->extra + b.p_x2_w2glo : nullptr;
  return k;
}

}  // namespace

Stage0Args stage0_args(const btsbot_ctx* h, bool keep) {
  const float* m = h->mirror;
  const bool x2 = h->x2 && !keep;
  const DownPk& d = h->down[1];
  Stage0Args a;
  memset(&a, 0, sizeof(a));
  a.stem_w = h->extra + (x2 ? h->p_x2_stem : h->p_stem16);
  a.stem_w_lo = x2 ? h->extra + h->p_x2_stemlo : nullptr;
  a.stem_b = m + h->stem_b;
  a.stem_lnw = m + h->stem_lnw;
  a.stem_lnb = m + h->stem_lnb;
  for (int j = 0; j < 2; ++j) a.blk[j] = s01_blk(h, h->blocks[0][j], keep);
  a.ds_lnw = m + d.ln_w;
  a.ds_lnb = m + d.ln_b;
  a.ds_w = h->extra + (x2 ? d.p_x2_w : d.p_w);
  a.ds_w_lo = x2 ? h->extra + d.p_x2_wlo : nullptr;
  a.ds_b = m + d.b;
  return a;
}

Stage1Args stage1_args(const btsbot_ctx* h, bool keep) {
  const float* m = h->mirror;
  const DownPk& d = h->down[2];
  Stage1Args a;
  memset(&a, 0, sizeof(a));
  for (int j = 0; j < 2; ++j) a.blk[j] = s01_blk(h, h->blocks[1][j], keep);
  a.ds_lnw = m + d.ln_w;
  a.ds_lnb = m + d.ln_b;
  a.ds_w = h->extra + d.p_wp;   // (split mode: heads and remainders in one fragment image)
  a.ds_b = m + d.b;
  return a;
}

Stage2pArgs stage2p_args(const btsbot_ctx* h, bool keep) {
  const float* m = h->mirror;
  const DownPk& d = h->down[3];
  Stage2pArgs a;
  memset(&a, 0, sizeof(a));
  a.depth = (int)h->blocks[2].size();
  for (int j = 0; j < a.depth; ++j) {
    const BlockPk& b = h->blocks[2][j];
    Stage2pBlk& k = a.blk[j];
    k.dw_w = reinterpret_cast<const float*>(h->extra + b.p_dw);
    k.dw_b = m + b.dw_b;
    k.ln_w = m + b.ln_w;
    k.ln_b = m + b.ln_b;
    k.b1 = m + b.fc1_b;
    k.b2 = m + b.fc2_b;
    k.gamma = m + b.gamma;
    k.w1p = h->extra + b.p_w1p;
    k.w2p = h->extra + b.p_w2p;
    k.scales = h->fp8 && !keep ? reinterpret_cast<const float*>(h->extra + b.p_scales) : nullptr;
  }
  a.ds_lnw = m + d.ln_w;
  a.ds_lnb = m + d.ln_b;
  a.ds_wp = h->extra + d.p_wp;
  a.ds_b = m + d.b;
  a.cw = h->cfg.dims[2];
  a.alerts_hint = h->s2p_alerts_hint;
  return a;
}

Stage3Args stage3_args(const btsbot_ctx* h) {
  const float* m = h->mirror;
  const int ch = h->cfg.dims[3];
  Stage3Args a;
  memset(&a, 0, sizeof(a));
  a.depth = (int)h->blocks[3].size();
  for (int j = 0; j < a.depth; ++j) {
    const BlockPk& b = h->blocks[3][j];
    Stage3Blk& k = a.blk[j];
    k.dw_c = reinterpret_cast<const float*>(h->extra + b.p_dw) + 24 * ch;   // tap-major [49][C]: the centre row
    k.dw_b = m + b.dw_b;
    k.ln_w = m + b.ln_w;
    k.ln_b = m + b.ln_b;
    k.w1p = h->extra + b.p_w1p;
    k.b1 = m + b.fc1_b;
    k.w2p = h->extra + b.p_w2p;
    k.b2 = m + b.fc2_b;
    k.gamma = m + b.gamma;
    k.scales = h->fp8 ? reinterpret_cast<const float*>(h->extra + b.p_scales) : nullptr;
  }
  return a;
}
