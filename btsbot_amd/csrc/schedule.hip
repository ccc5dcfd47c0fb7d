// The switch table's readers and resolve_schedule(): from a handle's configuration, what the kernels support and the
// BTSBOT_AMD_* switches to the one Schedule every launcher of the handle follows (schedule.h).  Host only.
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "ctx.h"
#include "head16.h"
#include "stage3.h"

namespace {

enum { ON, INT };
enum { HANDLE, PROCESS };
struct SwitchDecl {
  const char* name;
  int kind, scope;
  const char* meaning;
};
const SwitchDecl SWITCHES[SW_COUNT] = {
#define X(id, kind, scope, meaning) {"BTSBOT_AMD_" #id, kind, scope, meaning},
    BTSBOT_SWITCHES(X)
#undef X
};

constexpr int UNSET = INT_MIN;

// UNSET, or the value: 0 / 1 of an ON switch, atoi() of an INT one
int read_env(Switch s) {
  const char* e = getenv(SWITCHES[s].name);
  if (e == nullptr) return UNSET;
  return SWITCHES[s].kind == ON ? (e[0] == '1' ? 1 : 0) : atoi(e);
}

// PROCESS scope: the first read stays (racing first readers store the same value)
int value(Switch s) {
  if (SWITCHES[s].scope == HANDLE) return read_env(s);
  static int cache[SW_COUNT];
  static bool cached[SW_COUNT];
  if (!cached[s]) {
    cache[s] = read_env(s);
    cached[s] = true;
  }
  return cache[s];
}

}  // namespace

bool switch_on(Switch s) { return value(s) == 1; }
int switch_int(Switch s, int dflt) {
  const int v = value(s);
  return v == UNSET ? dflt : v;
}
bool switch_set(Switch s) { return value(s) != UNSET; }

void read_handle_switches(btsbot_ctx* h) {
  for (int s = 0; s < SW_COUNT; ++s) h->sw[s] = SWITCHES[s].scope == HANDLE ? read_env((Switch)s) : UNSET;
  h->opt_deterministic = h->sw[SW_DETERMINISTIC] == 1;
}

void resolve_schedule(btsbot_ctx* h) {
  const btsbot_config& c = h->cfg;
  const int prec = c.precision;
  auto on = [&](Switch s) { return h->sw[s] == 1; };
  auto num = [&](Switch s, int dflt) { return h->sw[s] == UNSET ? dflt : h->sw[s]; };
  Schedule s;
  const bool convnext = h->has_image && !h->is_maxvit;
  const bool plain16 = !h->x2 && !h->fp8 && (prec == BTSBOT_BF16 || prec == BTSBOT_F16);
  s.head16 = !on(SW_NO_HEAD16) && head16_supported(h->prec_head(), h->has_image ? c.dims[3] : 0, h->has_meta ? c.n_meta : 0,
                                                   c.meta_fc1, c.meta_fc2, h->n_comb, h->comb_dims);
  s.head_diag = num(SW_HEAD_DIAG, 0);
  s.dwln = !on(SW_NO_DWLN);
  s.s2mlp = !on(SW_NO_S2MLP);
  s.wgrad_batch = !on(SW_NO_WGRAD_BATCH);
  s.fork_per_block = on(SW_FORK_PER_BLOCK);
  s.side_stream = !on(SW_NO_SIDE_STREAM);
  s.meta_side = !switch_on(SW_NO_META_SIDE);
  // (the deterministic reductions cover the ConvNeXt training step only: btsbot_set_option refuses it elsewhere)
  s.deterministic = h->opt_deterministic && !h->is_maxvit;
  s.train_split = h->opt_train_split;
  s.train_packs = h->opt_train_packs;
  if (convnext) {
    s.stage0 = !on(SW_NO_STAGE0) && stage0_supported(h->prec_s01(), c.dims[0]) && c.depths[0] == 2;
    s.stage1 = !on(SW_NO_STAGE1) && stage1_supported(h->prec_s01(), c.dims[1], c.dims[2]) && c.depths[1] == 2;
    s.stage2p = !on(SW_NO_STAGE2) && stage2p_supported(h->prec_tail(), c.dims[2], c.dims[3], c.depths[2]);
    s.stage3 = !on(SW_NO_S3) && stage3_supported(h->prec_tail(), c.dims[3], c.depths[3]);
    // stage 1 on five alerts per workgroup while other forwards are in flight: its launch is 3 us longer than the
    // two-alert form's and holds 205 CUs instead of 256 at 1024 alerts (the split mode's two planar images hold two alerts)
    s.s1_g5 = s.stage1 && h->opt_forwards_in_flight && (h->prec_s01() == BTSBOT_BF16 || h->prec_s01() == BTSBOT_F16);
    // stage 2's alerts per workgroup: the caller's number wins, then the overlap hint (7: 147 workgroups at 1024 alerts,
    // the other streams' kernels take the remaining CUs), else the kernel's own choice by rounds
    s.s2p_alerts = h->s2p_alerts_hint != 0 ? h->s2p_alerts_hint : h->opt_forwards_in_flight ? 7 : 0;
    s.s2p_g7 = s.stage2p && s.s2p_alerts == 7 && h->prec_tail() != BTSBOT_F16X2;   // (split planes of 7 do not fit the LDS: 5)
    // stage 3's tiles.  Wide (64 alerts / 64 channels, half the workgroups, twice the rows per filter fragment): at 640
    // channels always -- 160 workgroups are one round of the chip, 320 two --, at 512 only while other forwards are in
    // flight: a lone forward gains nothing from the CUs given back (2.255 against 2.265 ms per 8192 alerts).  The split
    // mode's fragments are 8 registers each: narrow tiles only; fp8 at 640 channels stays narrow unless forced
    {
      const int tail = h->prec_tail(), forced = switch_int(SW_S3_TILES, 0);
      const bool can = tail == BTSBOT_BF16 || tail == BTSBOT_F16 || tail == BTSBOT_FP8;
      const bool pick = (c.dims[3] == 640 && tail != BTSBOT_FP8) || (c.dims[3] == 512 && h->opt_forwards_in_flight);
      s.s3_wide = s.stage3 && can && (forced == 2 || (forced != 1 && pick));
    }
    s.stem16 = !on(SW_NO_STEM16) && stem16_supported(prec, c.dims[0]);
    s.s0_diag = num(SW_S0_DIAG, 0);
    s.s2p_diag = num(SW_S2P_DIAG, 0);
    // widths whose block MLP runs fused in the training step: 64 and 128.  The 128-channel form hands dxn over as four
    // addend planes which only dwln_bwd_kernel reads, so it is tied to that kernel
    const int only = on(SW_NO_MLP_BWD) ? -1 : num(SW_MLP_BWD_C, 0);
    for (int i = 0; i < 4; ++i) {
      const int ch = c.dims[i];
      s.fused_mlp[i] = !on(SW_NO_FUSED_MLP) && fused_mlp_supported(prec, ch);
      s.mlp_bwd[i] = s.fused_mlp[i] && only >= 0 && (only == 0 || only == ch) && (ch == 64 || s.dwln) && mlp_bwd_supported(prec, ch);
    }
    // the keeping forms of the training forward (bf16 / f16).  Stages 0 and 1: their backward is mlp_bwd_kernel +
    // dwln_bwd_kernel, which read exactly what the form keeps.  Stage 1 by default in the f16 mode only (S1_TRAIN above)
    s.s0_keep = s.stage0 && plain16 && !on(SW_NO_S0_TRAIN) && s.mlp_bwd[0] && s.dwln;
    s.s1_keep = s.stage1 && plain16 && (prec == BTSBOT_F16 || on(SW_S1_TRAIN)) && !on(SW_NO_S1_TRAIN) && s.mlp_bwd[1] && s.dwln;
    // stage 2: wherever its backward runs the 3x3 kernel that recomputes the depthwise output the form does not keep
    // (dw3ln_bwd_kernel: dwln and not BTSBOT_AMD_DW3_OLD)
    s.s2_keep = s.stage2p && c.dims[2] == 256 && plain16 && s.dwln && dw3_bwd_active(3, 256) && !on(SW_NO_S2P_TRAIN);
    s.s2_keep_max_batch = 2560;
  }
  if (h->has_image && h->is_maxvit) {
    s.maxvit_split = h->x2;
    s.mv_attn_valu = on(SW_MV_ATTN_VALU);
    s.mv_dw_plain = on(SW_MV_DW_PLAIN);
    s.mv_stem_im2col = on(SW_MV_STEM_IM2COL);
    s.mv_gated_gemm = on(SW_MV_GATED_GEMM);
    s.mv_no_front = on(SW_MV_NO_FRONT);
    s.mv_no_ln_fuse = on(SW_MV_NO_LN_FUSE);
    s.mv_no_attn_block = on(SW_MV_NO_ATTN_BLOCK);
    s.mv_mlp_unfused = on(SW_MV_MLP_UNFUSED);
    s.mv_no_part = on(SW_MV_NO_PART);
    s.mv_no_smlp = on(SW_MV_NO_SMLP);
  }
  h->sched = s;
}

int query_schedule(const btsbot_ctx* h, const char* field) {
  const Schedule& s = h->sched;
  const bool* flag = nullptr;
#define X(f) \
  if (strcmp(field, #f) == 0) flag = &s.f;
  BTSBOT_SCHEDULE_FLAGS(X)
#undef X
  const size_t n = strlen(field);
  if (flag == nullptr && n > 1 && field[n - 1] >= '0' && field[n - 1] <= '3') {
#define X(f) \
  if (strlen(#f) == n - 1 && strncmp(field, #f, n - 1) == 0) flag = &s.f[field[n - 1] - '0'];
    BTSBOT_SCHEDULE_STAGE_FLAGS(X)
#undef X
  }
  if (flag == nullptr) {
    btsbot_set_error("query_schedule: no schedule field '%s'", field);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!*flag) {
    btsbot_set_error("query_schedule: %s is off on this handle", field);
    return BTSBOT_ERR_STATE;
  }
  return BTSBOT_OK;
}
