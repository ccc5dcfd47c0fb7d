// Internal: parameter / operand tables of the MaxViT image branch (maxvit.hip builds them; the training engine,
// maxvit_train.hip, reads them).
#pragma once
#include <stdint.h>
#include <stddef.h>

#include <utility>
#include <vector>

struct BnPk {
  int64_t w, b, rm, rv;      // master offsets
  size_t p_scale, p_shift;   // folded scale / shift (fp32) in `extra`
};
struct AttnPk {
  int64_t n1w, n1b, qkv_w, qkv_b, rel, proj_w, proj_b, n2w, n2b, fc1_w, fc1_b, fc2_w, fc2_b;
  size_t p_qkv, p_proj, p_fc1, p_fc2, p_bias, p_bias64, p_fused;
  size_t p_w1p = 0, p_w2p = 0;   // C = 256, 16-bit modes: fc1 / fc2 as stage2p.hip's MFMA A fragments (the streamed MLP)
  bool fused;
  bool smlp = false;             // the MLP runs stage2p_kernel's row-tile form (launch_stage2p_rows)
  size_t p_qkvp = 0, p_projp = 0, p_biasl = 0;   // C = 128 / 256, 16-bit modes: attn.qkv / attn.proj as MFMA A fragments, the bias in lane order (maxvit_part.hip)
  bool part = false;             // the partition block (attention half + MLP half) runs as one launch
};
struct MvBlock {
  int cin, c, mid, rd, stride, hin, hout;
  int64_t sc_w = -1;
  BnPk pre, n1, n2;
  int64_t c1_w, c1_b, c2_w, c2_b, se1_w, se1_b, se2_w, se2_b, c3_w;
  size_t p_sc, p_c1, p_c1b, p_dw, p_dwb, p_c3, p_se2t;
  AttnPk attn[2];   // [0] windows ("attn_block"), [1] grid ("attn_grid")
};

struct MaxVit {
  int64_t stem1_w, stem2_w, norm_w, norm_b;
  BnPk stem_bn;
  size_t p_stem1, p_stem2, p_zero, p_one;
  // f16x2 handles: every GEMM of the forward runs on split operands (gemm_x2.hip); its filter images hold the f16 head plane
  // followed by the remainder plane (the same 4 bytes per element as the fp32 images), p_x2_tmp stages the fp32 stem filters
  bool x2 = false;
  size_t p_x2_tmp = 0;
  std::vector<MvBlock> blocks;
  // workspace offsets (bytes) for the current reservation
  size_t o_x, o_x2, o_a, o_b, o_c, o_d, o_e, o_gate, o_feat, o_part, o_sescr, o_wg;
  // training, 16-bit modes: (fp32 GEMM input of the forward, its kept 16-bit copy) in call order; it outlives the forward
  // for the backward, and only MvtOperands (maxvit_train.hip) touches it
  std::vector<std::pair<const float*, void*>> xkept;
};

