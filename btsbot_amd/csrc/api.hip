// C ABI of libbtsbot_hip.so, the handle itself: error string and ABI version, the parameter table (build_tables), create /
// destroy, the pack entry points, btsbot_set_option, the debug / profile / stamps setters and the forward workspace
// (reserve / use_workspace).  The schedules live next door: forward.hip (inference), train_step.hip (training step and
// gradient buckets), streams.hip (side-stream placement, fork / join), exchange.hip (RCCL), infer_ops.hip (btsbot_op_*).
// See include/btsbot_hip.h for the contract and the reference code each entry point replaces.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ctx.h"
#include "maxvit.h"
#include "stage3.h"

// ---------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void btsbot_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* btsbot_last_error(void) { return g_err; }
extern "C" int btsbot_abi_version(void) { return BTSBOT_ABI_VERSION; }

namespace {

int64_t add_param(btsbot_ctx* h, const std::string& name, std::initializer_list<int> shape,
                  int is_buffer = 0) {
  ParamRec r;
  r.name = name;
  r.off = h->total_floats;
  r.ndim = (int)shape.size();
  r.numel = 1;
  int i = 0;
  for (int s : shape) {
    r.shape[i++] = s;
    r.numel *= s;
  }
  for (; i < 4; ++i) r.shape[i] = 1;
  r.is_buffer = is_buffer;
  // keep every tensor 16-byte aligned inside the arena so kernels can use vector loads
  h->total_floats += (r.numel + 3) / 4 * 4;
  h->params.push_back(r);
  return r.off;
}

int build_tables(btsbot_ctx* h) {
  const btsbot_config& c = h->cfg;
  char buf[96];
  if (h->has_image && h->is_maxvit) {
    maxvit_build_tables(h, &h->extra_fixed);   // (its operand images too; every other handle's: pack.hip)
  } else if (h->has_image) {
    const int c0 = c.dims[0];
    h->stem_w = add_param(h, "stem.0.weight", {c0, 3, 4, 4});
    h->stem_b = add_param(h, "stem.0.bias", {c0});
    h->stem_lnw = add_param(h, "stem.1.weight", {c0});
    h->stem_lnb = add_param(h, "stem.1.bias", {c0});
    h->blocks.resize(4);
    for (int i = 0; i < 4; ++i) {
      const int ch = c.dims[i];
      if (i > 0) {
        const int cin = c.dims[i - 1];
        snprintf(buf, sizeof buf, "stages.%d.downsample.", i);
        std::string p(buf);
        h->down[i].ln_w = add_param(h, p + "0.weight", {cin});
        h->down[i].ln_b = add_param(h, p + "0.bias", {cin});
        h->down[i].w = add_param(h, p + "1.weight", {ch, cin, 2, 2});
        h->down[i].b = add_param(h, p + "1.bias", {ch});
      }
      for (int j = 0; j < c.depths[i]; ++j) {
        snprintf(buf, sizeof buf, "stages.%d.blocks.%d.", i, j);
        std::string p(buf);
        BlockPk b;
        b.gamma = add_param(h, p + "gamma", {ch});
        b.dw_w = add_param(h, p + "conv_dw.weight", {ch, 1, 7, 7});
        b.dw_b = add_param(h, p + "conv_dw.bias", {ch});
        b.ln_w = add_param(h, p + "norm.weight", {ch});
        b.ln_b = add_param(h, p + "norm.bias", {ch});
        b.fc1_w = add_param(h, p + "mlp.fc1.weight", {4 * ch, ch, 1, 1});
        b.fc1_b = add_param(h, p + "mlp.fc1.bias", {4 * ch});
        b.fc2_w = add_param(h, p + "mlp.fc2.weight", {ch, 4 * ch, 1, 1});
        b.fc2_b = add_param(h, p + "mlp.fc2.bias", {ch});
        h->blocks[i].push_back(b);
      }
    }
    if (c.head_norm) {
      h->hn_w = add_param(h, "head_norm.weight", {c.dims[3]});
      h->hn_b = add_param(h, "head_norm.bias", {c.dims[3]});
    }
  }
  h->img_floats = h->total_floats;
  if (h->has_meta) {
    h->bn_w = add_param(h, "meta.0.weight", {c.n_meta});
    h->bn_b = add_param(h, "meta.0.bias", {c.n_meta});
    h->bn_rm = add_param(h, "meta.0.running_mean", {c.n_meta}, 1);
    h->bn_rv = add_param(h, "meta.0.running_var", {c.n_meta}, 1);
    h->m1_w = add_param(h, "meta.1.weight", {c.meta_fc1, c.n_meta});
    h->m1_b = add_param(h, "meta.1.bias", {c.meta_fc1});
    h->m2_w = add_param(h, "meta.4.weight", {c.meta_fc2, c.meta_fc1});
    h->m2_b = add_param(h, "meta.4.bias", {c.meta_fc2});
  }
  for (int i = 0; i < h->n_comb; ++i) {
    snprintf(buf, sizeof buf, "comb.%d.", i);
    std::string p(buf);
    h->comb_w[i] = add_param(h, p + "weight", {h->comb_dims[i + 1], h->comb_dims[i]});
    h->comb_b[i] = add_param(h, p + "bias", {h->comb_dims[i + 1]});
  }
  // gradient buckets, in the order the backward pass completes them
  if (h->has_image && !h->is_maxvit) {
    const int64_t s3 = h->down[3].ln_w, s2 = h->down[2].ln_w;
    h->n_buckets = 3;
    h->bucket_lo[0] = s3; h->bucket_hi[0] = h->total_floats;
    h->bucket_lo[1] = s2; h->bucket_hi[1] = s3;
    h->bucket_lo[2] = 0;  h->bucket_hi[2] = s2;
  } else {
    h->n_buckets = 1;
    h->bucket_lo[0] = 0;
    h->bucket_hi[0] = h->total_floats;
  }
  return BTSBOT_OK;
}

void ws_layout(const btsbot_ctx* h, int chunk, size_t* ox, size_t* ox2, size_t* oxn, size_t* oh,
               size_t* total) {
  const btsbot_config& c = h->cfg;
  size_t cur = 0;
  *ox = *ox2 = *oxn = *oh = 0;
  if (h->has_image && h->is_maxvit) {
    cur = maxvit_ws_bytes(h, chunk);
  } else if (h->has_image) {
    size_t x_el = 0, xn_el = 0, h_el = 0;
    for (int i = 0; i < 4; ++i) {
      const size_t pc = (size_t)STAGE_HW[i] * STAGE_HW[i] * c.dims[i];
      x_el = pc > x_el ? pc : x_el;
      xn_el = pc > xn_el ? pc : xn_el;
      h_el = 4 * pc > h_el ? 4 * pc : h_el;
      if (i > 0) {  // patch matrix feeding the downsample GEMM
        const size_t pe = (size_t)STAGE_HW[i] * STAGE_HW[i] * 4 * c.dims[i - 1];
        xn_el = pe > xn_el ? pe : xn_el;
      }
    }
    *ox = bump(cur, x_el * chunk * 4);
    *ox2 = bump(cur, x_el * chunk * 4);
    *oxn = bump(cur, xn_el * chunk * h->esz());
    size_t h_bytes = h_el * chunk * h->esz();
    if (h->sched.stage3) {   // stage3.hip keeps GELU(fc1) in fragment order, alerts rounded up to its 64-row tiles
      const size_t s3 = stage3_hfrag_bytes(h->prec_tail(), c.dims[3], chunk);
      h_bytes = s3 > h_bytes ? s3 : h_bytes;
    }
    *oh = bump(cur, h_bytes);
  }
  *total = cur > 256 ? cur : 256;
}

}  // namespace

extern "C" int btsbot_create(const btsbot_config* cfg, btsbot_handle* out) {
  if (cfg == nullptr || out == nullptr) {
    btsbot_set_error("create: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (cfg->abi_version != BTSBOT_ABI_VERSION) {
    btsbot_set_error("create: ABI version %d, library is %d", cfg->abi_version,
                     BTSBOT_ABI_VERSION);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (cfg->precision < BTSBOT_F32 || cfg->precision > BTSBOT_F16X2 ||
      cfg->wiring < BTSBOT_MM_CONVNEXT || cfg->wiring > BTSBOT_FROZEN_FUSION_MAXVIT) {
    btsbot_set_error("create: bad precision %d or wiring %d", cfg->precision, cfg->wiring);
    return BTSBOT_ERR_INVALID_ARG;
  }
  btsbot_ctx* h = new btsbot_ctx();
  h->cfg = *cfg;
  read_handle_switches(h);
  if (cfg->precision == BTSBOT_FP8) {   // everything but the fragment-streaming stages reads the bf16 schedule
    h->fp8 = true;
    h->cfg.precision = BTSBOT_BF16;
  }
  if (cfg->precision == BTSBOT_F16X2) {   // kernels without a split-operand form run the fp32 schedule
    h->x2 = true;
    h->cfg.precision = BTSBOT_F32;
    h->x2_tail_plain = h->sw[SW_X2_TAIL_F16] == 1;
  }
  const int w = cfg->wiring;
  h->has_image = (w != BTSBOT_UM_NN);
  h->has_meta = (w != BTSBOT_CONVNEXT && w != BTSBOT_MAXVIT);
  h->is_maxvit = (w == BTSBOT_MM_MAXVIT || w == BTSBOT_MAXVIT || w == BTSBOT_FROZEN_FUSION_MAXVIT);
  h->act = (w == BTSBOT_FROZEN_FUSION || w == BTSBOT_UM_NN || w == BTSBOT_FROZEN_FUSION_MAXVIT) ? ACT_RELU
                                                                                               : ACT_GELU;
  h->meta_trailing_act = (w == BTSBOT_MM_CONVNEXT || w == BTSBOT_UM_NN || w == BTSBOT_MM_MAXVIT) ? 1 : 0;
  if (h->is_maxvit) {
    const bool tiny = cfg->dims[0] == 64 && cfg->dims[1] == 128 && cfg->dims[2] == 256 &&
                      cfg->dims[3] == 512 && cfg->depths[0] == 2 && cfg->depths[1] == 2 &&
                      cfg->depths[2] == 5 && cfg->depths[3] == 2;
    if (cfg->image_size != 63 || !tiny || cfg->head_norm != 0) {
      btsbot_set_error("create: the MaxViT image branch is maxvit_tiny_rw_224 (dims 64,128,256,512, depths "
                       "2,2,5,2) on 63x63 cutouts resized to 224, without a head LayerNorm");
      delete h;
      return BTSBOT_ERR_INVALID_ARG;
    }
  } else if (h->has_image) {
    if (cfg->image_size != 63) {
      btsbot_set_error("create: kernels are specialised for 63x63 cutouts, got %d",
                       cfg->image_size);
      delete h;
      return BTSBOT_ERR_INVALID_ARG;
    }
    const bool pico = cfg->dims[0] == 64 && cfg->dims[1] == 128 && cfg->dims[2] == 256 &&
                      cfg->dims[3] == 512;
    const bool nano = cfg->dims[0] == 80 && cfg->dims[1] == 160 && cfg->dims[2] == 320 &&
                      cfg->dims[3] == 640;
    if (!pico && !nano) {
      btsbot_set_error("create: dims (%d,%d,%d,%d) are neither convnext_pico nor convnext_nano",
                       cfg->dims[0], cfg->dims[1], cfg->dims[2], cfg->dims[3]);
      delete h;
      return BTSBOT_ERR_INVALID_ARG;
    }
    for (int i = 0; i < 4; ++i)
      if (cfg->depths[i] < 1 || cfg->depths[i] > 64) {
        btsbot_set_error("create: bad depth %d for stage %d", cfg->depths[i], i);
        delete h;
        return BTSBOT_ERR_INVALID_ARG;
      }
  }
  if (h->has_meta && (cfg->n_meta < 1 || cfg->meta_fc1 < 1 || cfg->meta_fc2 < 1)) {
    btsbot_set_error("create: metadata branch needs n_meta, meta_fc1, meta_fc2 > 0");
    delete h;
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int feat = h->has_image ? cfg->dims[3] : 0;
  if (w == BTSBOT_UM_NN) {
    h->n_comb = 1;
    h->comb_dims[0] = cfg->meta_fc2;
    h->comb_dims[1] = 1;
  } else {
    if (cfg->comb_fc1 < 1 || cfg->comb_fc2 < 1) {
      btsbot_set_error("create: fusion head needs comb_fc1, comb_fc2 > 0");
      delete h;
      return BTSBOT_ERR_INVALID_ARG;
    }
    h->n_comb = 3;
    h->comb_dims[0] = feat + (h->has_meta ? cfg->meta_fc2 : 0);
    h->comb_dims[1] = cfg->comb_fc1;
    h->comb_dims[2] = cfg->comb_fc2;
    h->comb_dims[3] = 1;
  }
  build_tables(h);
  resolve_schedule(h);
  if (pack_layout(h) != BTSBOT_OK) {
    delete h;
    return BTSBOT_ERR_STATE;
  }
  *out = h;
  return BTSBOT_OK;
}

extern "C" int btsbot_destroy(btsbot_handle h) {
  if (h == nullptr) return BTSBOT_OK;
  if (h->mirror) (void)hipFree(h->mirror);
  if (h->extra) (void)hipFree(h->extra);
  pack_release(h);
  if (h->ws && h->ws_owned) (void)hipFree(h->ws);
  if (h->tcache) (void)hipFree(h->tcache);
  if (h->bbcache) (void)hipFree(h->bbcache);
  if (h->det_scratch) (void)hipFree(h->det_scratch);
  if (h->mv) maxvit_free(h);
  for (float* t : h->taps)
    if (t) (void)hipFree(t);
  for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
  if (h->xchg != nullptr) (void)hipStreamDestroy(h->xchg);
  if (h->xchg_done != nullptr) (void)hipEventDestroy(h->xchg_done);
  for (hipEvent_t e : h->bucket_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->side_ev) (void)hipEventDestroy(e);
  bool side_cached = false;
  for (const SidePick& p : h->side_cache) {
    side_cached = side_cached || p.side == h->side;
    (void)hipStreamDestroy(p.side);
  }
  if (h->side && !side_cached) (void)hipStreamDestroy(h->side);
  if (h->bwd_done) (void)hipEventDestroy(h->bwd_done);
  delete h;
  return BTSBOT_OK;
}

extern "C" int btsbot_param_count(btsbot_handle h) { return h ? (int)h->params.size() : -1; }
extern "C" int64_t btsbot_param_floats(btsbot_handle h) { return h ? h->total_floats : -1; }

extern "C" int btsbot_param_info_at(btsbot_handle h, int index, btsbot_param_info* out) {
  if (h == nullptr || out == nullptr || index < 0 || index >= (int)h->params.size()) {
    btsbot_set_error("param_info_at: bad handle or index %d", index);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const ParamRec& r = h->params[index];
  memset(out, 0, sizeof(*out));
  strncpy(out->name, r.name.c_str(), sizeof(out->name) - 1);
  out->offset = r.off;
  out->numel = r.numel;
  out->ndim = r.ndim;
  for (int i = 0; i < 4; ++i) out->shape[i] = r.shape[i];
  out->is_buffer = r.is_buffer;
  return BTSBOT_OK;
}

extern "C" int btsbot_pack_params(btsbot_handle h, const float* master, void* stream) {
  return pack_params(h, master, (hipStream_t)stream, false);
}

extern "C" int btsbot_pack_params_train(btsbot_handle h, const float* master, void* stream) {
  return pack_params(h, master, (hipStream_t)stream, true);
}

extern "C" int64_t btsbot_workspace_bytes(btsbot_handle h, int max_chunk) {
  if (h == nullptr || max_chunk < 1) return -1;
  size_t a, b, c, d, total;
  ws_layout(h, max_chunk, &a, &b, &c, &d, &total);
  return (int64_t)total;
}

extern "C" int btsbot_debug_stamps(btsbot_handle h, unsigned long long* device_buffer32) {
  if (h == nullptr) return BTSBOT_ERR_INVALID_ARG;
  h->stamps = device_buffer32;
  return BTSBOT_OK;
}

extern "C" int btsbot_set_option(btsbot_handle h, const char* key, int value) {
  if (h == nullptr || key == nullptr) {
    btsbot_set_error("set_option: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (strcmp(key, "stage2p_alerts") == 0) {
    if (value != 0 && value != 4 && value != 5 && value != 7) {
      btsbot_set_error("set_option: stage2p_alerts is 0 (automatic), 4, 5 or 7, got %d", value);
      return BTSBOT_ERR_INVALID_ARG;
    }
    h->s2p_alerts_hint = value;
    resolve_schedule(h);
    return BTSBOT_OK;
  }
  if (strcmp(key, "forwards_in_flight") == 0) {
    // every handle takes it; what it changes is the schedule's business (s2p_g7, s3_wide: 16-bit ConvNeXt tails)
    if (value != 0 && value != 1) {
      btsbot_set_error("set_option: forwards_in_flight is 0 or 1, got %d", value);
      return BTSBOT_ERR_INVALID_ARG;
    }
    h->opt_forwards_in_flight = value == 1;
    resolve_schedule(h);
    return BTSBOT_OK;
  }
  if (strcmp(key, "deterministic") == 0) {
    if (value != 0 && value != 1) {
      btsbot_set_error("set_option: deterministic is 0 or 1, got %d", value);
      return BTSBOT_ERR_INVALID_ARG;
    }
    if (value == 1 && h->det_scratch == nullptr && h->tcache != nullptr) {
      btsbot_set_error("set_option: deterministic = 1 must be set before btsbot_reserve_train() (it sizes a scratch there)");
      return BTSBOT_ERR_STATE;
    }
    if (value == 1 && h->is_maxvit) {
      btsbot_set_error("set_option: the deterministic reductions cover the ConvNeXt training step; a MaxViT branch's "
                       "backward still meets through atomics");
      return BTSBOT_ERR_STATE;
    }
    h->opt_deterministic = value == 1;
    resolve_schedule(h);
    return BTSBOT_OK;
  }
  if (strcmp(key, "train_split") == 0) {
    if (value != 0 && value != 1) {
      btsbot_set_error("set_option: train_split is 0 or 1, got %d", value);
      return BTSBOT_ERR_INVALID_ARG;
    }
    if (!h->x2 || !h->has_image || h->is_maxvit) {
      btsbot_set_error("set_option: train_split needs a BTSBOT_F16X2 handle with a ConvNeXt image branch (this one: %s)",
                       !h->x2 ? "another precision" : !h->has_image ? "no image branch" : "a MaxViT image branch");
      return BTSBOT_ERR_INVALID_ARG;
    }
    if (h->mirror != nullptr || h->tcache != nullptr) {
      btsbot_set_error("set_option: train_split changes the packed-operand layout: set it before the first "
                       "btsbot_pack_params* / btsbot_reserve_train()");
      return BTSBOT_ERR_STATE;
    }
    h->opt_train_split = value == 1;
    resolve_schedule(h);
    return pack_layout(h);   // (the split planes are images of their own)
  }
  if (strcmp(key, "query_train_split") == 0) {
    // a query: BTSBOT_OK when the training step's matrix products run on split operands
    if (!h->sched.train_split) {
      btsbot_set_error("query_train_split: this handle's training products run on %s",
                       h->x2 ? "the fp32 MFMA (train_split is off)" : "the operand type of its precision");
      return BTSBOT_ERR_STATE;
    }
    return BTSBOT_OK;
  }
  if (strcmp(key, "query_side_apart") == 0) {
    // a query, not a setting: BTSBOT_OK when the training step's second stream (and, once btsbot_allreduce_grads() has run,
    // its exchange stream) was measured on a hardware pipe of its own, BTSBOT_ERR_STATE when none of the candidates was
    if (h->side != nullptr && !h->side_apart) {
      btsbot_set_error("the backward's side stream shares a hardware pipe with the caller's stream");
      return BTSBOT_ERR_STATE;
    }
    if (h->xchg != nullptr && !h->xchg_apart) {
      btsbot_set_error("the exchange stream shares a hardware pipe with the caller's or the side stream");
      return BTSBOT_ERR_STATE;
    }
    return BTSBOT_OK;
  }
  if (strcmp(key, "query_maxvit_split") == 0) {
    // a query: BTSBOT_OK when the MaxViT inference forward runs its matrix products on split operands (gemm_x2.hip)
    if (!h->sched.maxvit_split) {
      btsbot_set_error("query_maxvit_split: this handle's %s", h->has_image && h->is_maxvit
                                                                  ? "MaxViT GEMMs run on the operand type of its precision"
                                                                  : "image branch is not MaxViT");
      return BTSBOT_ERR_STATE;
    }
    return BTSBOT_OK;
  }
  if (strncmp(key, "query_schedule:", 15) == 0) return query_schedule(h, key + 15);
  if (strcmp(key, "exchange") == 0) {
    if (value != 0 && value != 1) {
      btsbot_set_error("set_option: exchange is 0 (one all-reduce per span) or 1 (reduce-scatter + all-gather), got %d", value);
      return BTSBOT_ERR_INVALID_ARG;
    }
    h->exchange_mode = value;
    return BTSBOT_OK;
  }
  btsbot_set_error("set_option: unknown option '%s'", key);
  return BTSBOT_ERR_INVALID_ARG;
}

extern "C" int btsbot_set_debug(btsbot_handle h, int on) {
  if (h == nullptr) return BTSBOT_ERR_INVALID_ARG;
  h->debug = on != 0;
  return BTSBOT_OK;
}

extern "C" int btsbot_set_profile(btsbot_handle h, int on) {
  if (h == nullptr) return BTSBOT_ERR_INVALID_ARG;
  if (on && h->prof_ev.empty()) {
    h->prof_ev.resize(2 * PROF_MAX_LAUNCHES);
    h->prof_cat.resize(PROF_MAX_LAUNCHES);
    for (hipEvent_t& e : h->prof_ev) HIP_TRY(hipEventCreate(&e));
  }
  h->prof_on = on != 0;
  h->prof_used = 0;
  return BTSBOT_OK;
}

extern "C" int btsbot_profile_categories(void) { return NCAT; }

extern "C" const char* btsbot_profile_category_name(int cat) {
  return cat >= 0 && cat < NCAT ? CAT_NAMES[cat] : "";
}

extern "C" int btsbot_profile_collect(btsbot_handle h, int n_cat, double* ms_sum,
                                      int64_t* launches) {
  if (h == nullptr || ms_sum == nullptr || launches == nullptr || n_cat < NCAT) {
    btsbot_set_error("profile_collect: bad argument (need room for %d categories)", NCAT);
    return BTSBOT_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_cat; ++i) {
    ms_sum[i] = 0.0;
    launches[i] = 0;
  }
  for (size_t i = 0; i < h->prof_used; ++i) {
    HIP_TRY(hipEventSynchronize(h->prof_ev[2 * i + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->prof_ev[2 * i], h->prof_ev[2 * i + 1]));
    ms_sum[h->prof_cat[i]] += ms;
    launches[h->prof_cat[i]] += 1;
  }
  h->prof_used = 0;
  return BTSBOT_OK;
}

// workspace of the forward path: allocated here (btsbot_reserve) or handed in by the caller (btsbot_use_workspace,
// the caller-sized form of SURVEY.md section 8b: no allocation inside the library on that path)
static int install_workspace(btsbot_handle h, int max_chunk, unsigned char* caller_ws, int64_t caller_bytes) {
  size_t total;
  size_t ox, ox2, oxn, oh;
  ws_layout(h, max_chunk, &ox, &ox2, &oxn, &oh, &total);
  if (caller_ws == nullptr && h->ws != nullptr && h->ws_owned && max_chunk <= h->max_chunk &&
      (!h->debug || h->taps[0] != nullptr))
    return BTSBOT_OK;
  if (caller_ws != nullptr && (size_t)caller_bytes < total) {
    btsbot_set_error("use_workspace: %lld bytes for chunks of %d alerts, btsbot_workspace_bytes() says %zu",
                     (long long)caller_bytes, max_chunk, total);
    return BTSBOT_ERR_INVALID_ARG;
  }
  HIP_TRY(hipDeviceSynchronize());
  if (h->ws && h->ws_owned) (void)hipFree(h->ws);
  h->ws = nullptr;
  if (caller_ws != nullptr) {
    h->ws = caller_ws;
    h->ws_owned = false;
  } else {
    HIP_TRY(hipMalloc(&h->ws, total));
    h->ws_owned = true;
  }
  h->ws_bytes = total;
  h->max_chunk = max_chunk;
  h->o_x = ox;
  h->o_x2 = ox2;
  h->o_xn = oxn;
  h->o_h = oh;
  for (float*& t : h->taps) {
    if (t) (void)hipFree(t);
    t = nullptr;
  }
  if (h->debug && h->is_maxvit) {   // stem 112x112x64, stages 56 / 28 / 14 / 7
    HIP_TRY(hipMalloc(&h->taps[0], (size_t)max_chunk * 12544 * 64 * 4));
    for (int i = 0; i < 4; ++i)
      HIP_TRY(hipMalloc(&h->taps[i + 1], (size_t)max_chunk * (56 >> i) * (56 >> i) * h->cfg.dims[i] * 4));
  } else if (h->debug && h->has_image) {
    HIP_TRY(hipMalloc(&h->taps[0], (size_t)max_chunk * 225 * h->cfg.dims[0] * 4));
    for (int i = 0; i < 4; ++i)
      HIP_TRY(hipMalloc(&h->taps[i + 1],
                        (size_t)max_chunk * STAGE_HW[i] * STAGE_HW[i] * h->cfg.dims[i] * 4));
  }
  return BTSBOT_OK;
}

extern "C" int btsbot_reserve(btsbot_handle h, int max_chunk) {
  if (h == nullptr || max_chunk < 1) {
    btsbot_set_error("reserve: bad argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return install_workspace(h, max_chunk, nullptr, 0);
}

extern "C" int btsbot_use_workspace(btsbot_handle h, int max_chunk, void* workspace, int64_t bytes) {
  if (h == nullptr || max_chunk < 1 || workspace == nullptr || ((uintptr_t)workspace & 255) != 0) {
    btsbot_set_error("use_workspace: bad argument (the workspace must be 256-byte aligned device memory)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return install_workspace(h, max_chunk, reinterpret_cast<unsigned char*>(workspace), bytes);
}
