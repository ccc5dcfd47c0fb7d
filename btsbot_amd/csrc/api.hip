// C ABI of libbtsbot_hip.so: handle, parameter table, weight packing and the forward schedule.
// See include/btsbot_hip.h for the contract and the reference code each entry point replaces.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <algorithm>

#include <string>
#include <vector>

#include "common.h"
#include <dlfcn.h>

#include "ctx.h"
#include "maxvit.h"
#include "stage0.h"
#include "stage2p.h"
#include "stage3.h"
#include "head16.h"

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

#define TRY(call)                   \
  do {                              \
    int _s = (call);                \
    if (_s != BTSBOT_OK) return _s; \
  } while (0)

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

// run one launch, bracketed by HIP events on `st` when profiling is on
template <typename F> static int timed(btsbot_ctx* h, int cat, hipStream_t st, F&& fn) {
  const bool rec = h->prof_on && h->prof_used < PROF_MAX_LAUNCHES;
  if (rec) HIP_TRY(hipEventRecord(h->prof_ev[2 * h->prof_used], st));
  const int s = fn();
  if (s != BTSBOT_OK) return s;
  if (rec) {
    HIP_TRY(hipEventRecord(h->prof_ev[2 * h->prof_used + 1], st));
    h->prof_cat[h->prof_used++] = cat;
  }
  return BTSBOT_OK;
}

// a stage kernel's per-workgroup wall-clock region: nullptr without a stamp buffer or when `grid` workgroups do not fit
static unsigned long long* stamp_wgt(const btsbot_ctx* h, size_t off, int max_wg, int grid) {
  return h->stamps != nullptr && grid <= max_wg ? h->stamps + off : nullptr;
}

// image branch of one chunk; *feat_out = [nb][dims[3]] fp32 features inside the workspace
static int backbone_chunk(btsbot_ctx* h, const float* img, int nb, hipStream_t st,
                          float** feat_out) {
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
          return launch_stage1b(h->prec_s01(), a, st);
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

// ---------------------------------------------------------------------------------------
// training: forward with batch statistics + dropout, backward of the heads
// ---------------------------------------------------------------------------------------
size_t train_cache_floats(const btsbot_ctx* h, int M);
size_t bb_cache_bytes(const btsbot_ctx* h, int B);
int backbone_train_forward(btsbot_ctx* h, const float* img, int B, hipStream_t st, float** feat_out);
int backbone_train_backward(btsbot_ctx* h, const float* img, const float* dfeat, float* grads,
                            int B, hipStream_t st);
float* train_cache_feat(btsbot_ctx* h, float* cache, int M);
int head_train_forward(btsbot_ctx* h, float* cache, const float* meta, float* logits,
                       float* scores, int M, const uint8_t* meta_mask, const uint8_t* comb_mask,
                       float* master, hipStream_t st, bool meta_done = false);
int head_train_meta_forward(btsbot_ctx* h, float* cache, const float* meta, int M, const uint8_t* meta_mask, float* master,
                            hipStream_t st);
int head_train_backward(btsbot_ctx* h, float* cache, const float* dlogits, float* grads, int M,
                        int need_meta, int need_image, float** dfeat_out,
                        const uint8_t* meta_mask, const uint8_t* comb_mask, hipStream_t st);

extern "C" int btsbot_reserve_train(btsbot_handle h, int max_batch, int with_image_grads) {
  if (h == nullptr || max_batch < 1) {
    btsbot_set_error("reserve_train: bad argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  // (MaxViT: with_image_grads = 1 trains the branch -- BatchNorm2d batch statistics, maxvit_train.hip; = 0 serves heads
  //  over a frozen, eval-mode branch with the inference kernels)
  const bool want_bb = with_image_grads && h->has_image;
  if (h->sched.deterministic) {   // partial rows of the batch reductions (common.h: det_add), sized by the batch: 256 KB per alert,
    const size_t want = std::max((size_t)16 << 20, (size_t)max_batch << 16);   // at least 64 MB (what a step of <= 256 alerts takes)
    if (h->det_scratch == nullptr || h->det_floats < want) {
      HIP_TRY(hipDeviceSynchronize());
      if (h->det_scratch != nullptr) (void)hipFree(h->det_scratch);
      h->det_scratch = nullptr;
      h->det_floats = want;
      HIP_TRY(hipMalloc(&h->det_scratch, h->det_floats * sizeof(float)));
    }
  }
  if (h->tcache != nullptr && max_batch <= h->tcache_batch &&
      (!want_bb || (h->bbcache != nullptr && max_batch <= h->bbcache_batch)))
    return BTSBOT_OK;
  HIP_TRY(hipDeviceSynchronize());
  if (h->tcache == nullptr || max_batch > h->tcache_batch) {
    if (h->tcache) (void)hipFree(h->tcache);
    h->tcache = nullptr;
    HIP_TRY(hipMalloc(&h->tcache, train_cache_floats(h, max_batch) * sizeof(float)));
    h->tcache_batch = max_batch;
  }
  if (want_bb && (h->bbcache == nullptr || max_batch > h->bbcache_batch)) {
    if (h->bbcache) (void)hipFree(h->bbcache);
    h->bbcache = nullptr;
    HIP_TRY(hipMalloc(&h->bbcache, h->is_maxvit ? maxvit_train_cache_bytes(h, max_batch) : bb_cache_bytes(h, max_batch)));
    h->bbcache_batch = max_batch;
    if (!h->opt_train_packs && !h->is_maxvit) {      // the dgrad transposes must be packed too from now on
      h->opt_train_packs = true;
      resolve_schedule(h);
      TRY(pack_invalidate(h));   // (the job tables were built without the transposes)
    }
  }
  h->train_batch = 0;
  return BTSBOT_OK;
}

extern "C" int btsbot_forward_train(btsbot_handle h, const float* triplets, const float* meta,
                                    float* logits, float* scores, int batch,
                                    const uint8_t* meta_mask, const uint8_t* comb_mask,
                                    float* master_arena, int keep_image_activations,
                                    void* stream) {
  if (h == nullptr || logits == nullptr || batch < 1) {
    btsbot_set_error("forward_train: NULL handle/logits or empty batch");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!h->packed || h->ws == nullptr || h->tcache == nullptr || batch > h->tcache_batch) {
    btsbot_set_error("forward_train: pack_params / reserve / reserve_train(%d) first", batch);
    return BTSBOT_ERR_STATE;
  }
  if ((h->has_image && triplets == nullptr) || (h->has_meta && meta == nullptr)) {
    btsbot_set_error("forward_train: missing input for this wiring");
    return BTSBOT_ERR_INVALID_ARG;
  }
  const btsbot_config& c = h->cfg;
  if (h->has_meta && ((c.meta_dropout > 0.f && meta_mask == nullptr) || c.meta_dropout >= 1.f)) {
    btsbot_set_error("forward_train: metadata dropout %.3f needs a keep-mask", c.meta_dropout);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (h->n_comb > 1 && ((c.comb_dropout > 0.f && comb_mask == nullptr) || c.comb_dropout >= 1.f)) {
    btsbot_set_error("forward_train: head dropout %.3f needs a keep-mask", c.comb_dropout);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (h->has_meta && (c.n_meta > 768 || c.meta_fc1 > 768 || c.meta_fc2 > 768)) {
    btsbot_set_error("forward_train: metadata widths above 768 are not supported");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  bool meta_done = false, meta_on_side = false;
  h->bb_saved = false;
  // the pool's events of the previous forward / backward are all recorded and their waits enqueued: start over (a loop of
  // training-mode forwards without a backward -- BatchNorm recalibration -- would otherwise grow the pool without bound)
  h->side_used = 0;
  h->t_img = triplets;
  // (the ConvNeXt training forward waits for the packing launches behind its stem, backbone_train.hip)
  if (!(h->has_image && keep_image_activations && !h->is_maxvit)) TRY(pack_sync(h, st));
  if (h->has_image && keep_image_activations) {
    if (h->bbcache == nullptr || batch > h->bbcache_batch) {
      btsbot_set_error("forward_train: reserve_train(%d, with_image_grads=1) first", batch);
      return BTSBOT_ERR_STATE;
    }
    float* feat = nullptr;
    if (h->is_maxvit) {
      TRY(maxvit_train_forward(h, triplets, batch, master_arena, st, &feat));
      h->bb_saved = true;
    } else {
      // the metadata branch reads nothing of the image branch: its three launches go to the side stream (behind the
      // re-pack queued there) and run beside the backbone instead of in the chain behind it
      hipStream_t sd = st;
      if (h->has_meta && h->side != nullptr && h->sched.meta_side) {
        TRY(side_fork(h, st, &sd));
        TRY(head_train_meta_forward(h, h->tcache, meta, batch, meta_mask, master_arena, sd));
        meta_on_side = sd != st;
        h->meta_join_pending = meta_on_side;   // (cleared by the next side_join(): the forward's wait for the re-pack, as a rule)
        meta_done = true;
      }
      TRY(backbone_train_forward(h, triplets, batch, st, &feat));
      if (meta_on_side && h->meta_join_pending) TRY(side_join(h, st));
    }
    TRY(launch_copy_f32(train_cache_feat(h, h->tcache, batch), feat, (size_t)batch * c.dims[3], st));
  } else if (h->has_image) {
    // The image branch has no train/eval difference (no BatchNorm, no dropout, drop-path 0):
    // same kernels as inference, chunk by chunk; features are collected in the training cache.
    float* feat = train_cache_feat(h, h->tcache, batch);
    const int F = c.dims[3];
    for (int b0 = 0; b0 < batch; b0 += h->max_chunk) {
      const int nb = batch - b0 < h->max_chunk ? batch - b0 : h->max_chunk;
      float* x = nullptr;
      TRY(backbone_chunk(h, triplets + (size_t)b0 * 3 * 63 * 63, nb, st, &x));
      HIP_TRY(hipMemcpyAsync(feat + (size_t)b0 * F, x, (size_t)nb * F * sizeof(float),
                             hipMemcpyDeviceToDevice, st));
    }
  }
  TRY(head_train_forward(h, h->tcache, meta, logits, scores, batch, meta_mask, comb_mask,
                         master_arena, st, meta_done));
  h->train_batch = batch;
  h->t_meta_mask = meta_mask;
  h->t_comb_mask = comb_mask;
  return BTSBOT_OK;
}

extern "C" int btsbot_backward(btsbot_handle h, const float* dlogits, float* grad_arena,
                               int need_meta_grads, int need_image_grads, void* stream) {
  if (h == nullptr || dlogits == nullptr || grad_arena == nullptr) {
    btsbot_set_error("backward: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (h->train_batch < 1) {
    btsbot_set_error("backward: no training-mode forward has been run on this handle");
    return BTSBOT_ERR_STATE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int need_img = need_image_grads && h->has_image;
  if (need_img && !h->bb_saved) {
    btsbot_set_error("backward: image-branch gradients need forward_train(keep_image_activations=1)");
    return BTSBOT_ERR_STATE;
  }
  if (h->sched.deterministic && need_img) {
    // checked BEFORE anything is launched or any handle state moves: the scratch of the fixed-order reductions is sized
    // by the batch at btsbot_reserve_train() (256 KB per alert, at least 64 MB)
    const size_t want = std::max((size_t)16 << 20, (size_t)h->train_batch << 16);
    if (h->det_scratch == nullptr || h->det_floats < want) {
      btsbot_set_error("backward: the deterministic mode's scratch (%zu floats) is too small for a batch of %d (%zu): set the "
                       "option before btsbot_reserve_train(%d, 1)", h->det_floats, h->train_batch, want, h->train_batch);
      return BTSBOT_ERR_STATE;
    }
  }
  if (need_img)   // image-branch gradients are accumulated with atomics
    TRY(launch_fill0(grad_arena, (size_t)h->img_floats, st));
  for (int i = 0; i < h->n_buckets; ++i)
    if (h->bucket_ev[i] == nullptr) HIP_TRY(hipEventCreateWithFlags(&h->bucket_ev[i], hipEventDisableTiming));
  if (h->sched.side_stream && (h->side == nullptr || h->side_for != st)) {
    // the caller changed streams: the side stream chosen against the old one may share the new one's pipe.  Whatever the
    // old pair still holds is ordered in front of this call by the join below (the new caller stream waits for it)
    hipStream_t old = h->side;
    TRY(create_side_stream(h, st));
    if (old != nullptr && old != h->side) {
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      hipError_t r1 = hipEventRecord(e, old), r2 = r1 == hipSuccess ? hipStreamWaitEvent(st, e, 0) : r1;
      (void)hipEventDestroy(e);   // (released once the record has completed)
      HIP_TRY(r2);
    }
  }
  h->side_used = 0;
  // deterministic mode: the launchers below take their partial rows from this scratch (fixed-order reductions)
  struct DetScope {
    explicit DetScope(btsbot_ctx* c) { det_begin(c->sched.deterministic ? c->det_scratch : nullptr, c->det_floats); }
    ~DetScope() { det_end(); }
  } det_scope(h);
  // (the paths that record every bucket at their end anyway always do; the ConvNeXt backward forks for them on demand)
  h->bucket_fine = h->bucket_waits_seen || !need_img || h->is_maxvit;
  float* dfeat = nullptr;
  TRY(head_train_backward(h, h->tcache, dlogits, grad_arena, h->train_batch, need_meta_grads,
                          need_img, &dfeat, h->t_meta_mask, h->t_comb_mask, st));
  if (need_img) {
    if (h->is_maxvit) {
      TRY(side_join(h, st));
      TRY(maxvit_train_backward(h, h->t_img, dfeat, grad_arena, h->train_batch, st));   // records the bucket event
    } else {
      TRY(backbone_train_backward(h, h->t_img, dfeat, grad_arena, h->train_batch, st));   // records the bucket events
    }
  } else {
    TRY(side_join(h, st));
    for (int i = 0; i < h->n_buckets; ++i) HIP_TRY(hipEventRecord(h->bucket_ev[i], st));
  }
  if (!h->bucket_fine) {
    // nobody has asked for a bucket yet, so the per-stage events were not recorded: ONE event for "everything is there",
    // which a late btsbot_wait_grad_bucket() / btsbot_allreduce_grads() waits on (no stream handle is kept for later)
    if (h->bwd_done == nullptr) HIP_TRY(hipEventCreateWithFlags(&h->bwd_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->bwd_done, st));
  }
  h->bucket_recorded = true;
  h->last_grad_arena = grad_arena;
  if (det_fell_short()) {
    // (cannot happen with the entry check above unless the sizing rule and the launchers disagree: the gradients are
    //  complete and correct, but some reduction fell back to atomics)
    btsbot_set_error("backward: the deterministic mode's scratch (%zu floats) ran out inside a batch of %d although the entry "
                     "check passed -- gradients are valid, not bit-reproducible", h->det_floats, h->train_batch);
    return BTSBOT_ERR_STATE;
  }
  return BTSBOT_OK;
}

// The backward's second stream must be served by a DIFFERENT hardware pipe than the caller's stream.  A compute pipe
// works on one of its hardware queues at a time and changes queue when that one runs dry or after a time quantum; which
// pipe a new stream's queue gets depends on how many queues the process already has.  When both streams of the backward
// land on one pipe their kernels are dispatched in turns of ~50 us instead of side by side: measured 4.9-7.0 ms per
// 1024-alert step against 2.75 ms, in every process that had used exactly THREE other streams before the first
// btsbot_backward() (bench.py's scoring loop; tools/host_streams_probe2.py: two or four are fine; stream priorities and
// GPU_MAX_HW_QUEUES do not move it).  The placement cannot be asked, so it is measured, RELATIVE to a baseline taken in
// the same call: the host times an empty kernel on the candidate (launch -> event synchronise) first with the busy
// streams idle, then while a train of short spinning kernels keeps each of them busy; the minimum over the trials of
// each (host noise and a profiler's per-launch cost only ever add, and they add to both) differs by a few microseconds
// when the candidate runs beside the trains and by a quantum (30-40 us) when it shares a pipe with one of them.
// Up to eight candidates.  The choice is kept per caller stream (ctx.h: side_cache); when no candidate runs apart the
// last one is kept anyway and the handle says so: once on stderr, in btsbot_last_error() and through
// btsbot_set_option(h, "query_side_apart", 0) (returns 1 / 0 as BTSBOT_OK / BTSBOT_ERR_STATE).
__global__ void spin_kernel(unsigned long long ticks) {   // s_memrealtime counts at 100 MHz
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
__global__ void empty_kernel() {}

namespace {
constexpr double SAME_PIPE_EXTRA_US = 20.0;   // beside: +0 .. 9 us over the idle baseline; same pipe: +30 .. 40
constexpr int PLACEMENT_TRIALS = 4;

struct StreamPile {   // candidates that were not taken (and the event) are released on every path out
  hipStream_t s[8];
  int n = 0;
  hipEvent_t ev = nullptr;
  ~StreamPile() {
    for (int i = 0; i < n; ++i) (void)hipStreamDestroy(s[i]);
    if (ev != nullptr) (void)hipEventDestroy(ev);
  }
};

// microseconds from the launch of an empty kernel on `cand` to the host seeing it done (minimum of the trials), with a
// train of spinning kernels on each of busy[0..nbusy) when `loaded`
int time_candidate(hipStream_t cand, hipEvent_t ev, const hipStream_t* busy, int nbusy, bool loaded, double* best_us) {
  double best = 1e30;
  for (int trial = 0; trial < PLACEMENT_TRIALS; ++trial) {
    for (int b = 0; b < nbusy; ++b) HIP_TRY(hipStreamSynchronize(busy[b]));
    if (loaded)
      for (int i = 0; i < 24; ++i)          // 24 x 25 us per busy stream, interleaved so that every train has started
        for (int b = 0; b < nbusy; ++b) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, busy[b], 2500ULL);
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, cand);
    HIP_TRY(hipEventRecord(ev, cand));
    HIP_TRY(hipEventSynchronize(ev));
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    best = us < best ? us : best;
  }
  for (int b = 0; b < nbusy; ++b) HIP_TRY(hipStreamSynchronize(busy[b]));
  *best_us = best;
  return BTSBOT_OK;
}
}  // namespace

// a new non-blocking stream whose hardware queue is served by another pipe than every stream in busy[]
int pick_apart_stream(btsbot_ctx* h, const hipStream_t* busy, int nbusy, const char* role, hipStream_t* out, bool* apart_out) {
  StreamPile pile;
  HIP_TRY(hipEventCreateWithFlags(&pile.ev, hipEventDisableTiming));
  const bool debug = switch_set(SW_DEBUG_SIDE);
  hipStream_t chosen = nullptr;
  bool apart = false;
  for (int attempt = 0; attempt < 8 && chosen == nullptr; ++attempt) {
    hipStream_t cand = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&cand, hipStreamNonBlocking));
    pile.s[pile.n++] = cand;
    hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, cand);   // (first use of the stream: its queue exists now)
    HIP_TRY(hipStreamSynchronize(cand));
    double idle = 0.0, loaded = 0.0;
    TRY(time_candidate(cand, pile.ev, busy, nbusy, false, &idle));
    TRY(time_candidate(cand, pile.ev, busy, nbusy, true, &loaded));
    apart = loaded - idle < SAME_PIPE_EXTRA_US;
    if (debug)
      fprintf(stderr, "btsbot: %s-stream candidate %d: its kernel returns in %.1f us with the %d busy stream(s) idle, %.1f us "
                      "beside their spinning kernels -> %s\n", role, attempt, idle, nbusy, loaded,
              apart ? "taken" : "shares a pipe, rejected");
    if (apart) {
      chosen = cand;
      --pile.n;   // (the newest entry: leaves the pile)
    }
  }
  if (chosen == nullptr) {   // no candidate ran beside the busy streams: keep the last one, and say so
    chosen = pile.s[--pile.n];
    btsbot_set_error("warning: no %s stream on a hardware pipe of its own was found in 8 candidates; its kernels will take turns "
                     "with the caller's (expect slower training steps)", role);
    static bool told = false;
    if (!told) {
      told = true;
      fprintf(stderr, "btsbot_amd: %s\n", btsbot_last_error());
    }
  }
  *out = chosen;
  *apart_out = apart;
  (void)h;
  return BTSBOT_OK;
}

int create_side_stream(btsbot_ctx* h, hipStream_t caller) {
  // one choice per caller stream: a caller that alternates streams gets the stream picked for each back, no new probe
  for (const SidePick& p : h->side_cache)
    if (p.caller == caller) {
      h->side = p.side;
      h->side_for = caller;
      h->side_apart = p.apart;
      return BTSBOT_OK;
    }
  hipStream_t chosen = nullptr;
  bool apart = false;
  TRY(pick_apart_stream(h, &caller, 1, "side", &chosen, &apart));
  h->side_cache.push_back(SidePick{caller, chosen, apart});
  h->side = chosen;
  h->side_for = caller;
  h->side_apart = apart;
  return BTSBOT_OK;
}

static int side_event(btsbot_ctx* h, hipEvent_t* e) {
  if (h->side_used == h->side_ev.size()) {
    hipEvent_t fresh;
    HIP_TRY(hipEventCreateWithFlags(&fresh, hipEventDisableTiming));
    h->side_ev.push_back(fresh);
  }
  *e = h->side_ev[h->side_used++];
  return BTSBOT_OK;
}

int side_fork(btsbot_ctx* h, hipStream_t st, hipStream_t* sd) {
  *sd = st;
  if (!h->sched.side_stream || h->side == nullptr) return BTSBOT_OK;
  hipEvent_t e;
  TRY(side_event(h, &e));
  HIP_TRY(hipEventRecord(e, st));
  HIP_TRY(hipStreamWaitEvent(h->side, e, 0));
  *sd = h->side;
  return BTSBOT_OK;
}

int side_join(btsbot_ctx* h, hipStream_t st) {
  if (!h->sched.side_stream || h->side == nullptr) return BTSBOT_OK;
  hipEvent_t e;
  TRY(side_event(h, &e));
  HIP_TRY(hipEventRecord(e, h->side));
  HIP_TRY(hipStreamWaitEvent(st, e, 0));
  h->meta_join_pending = false;
  return BTSBOT_OK;
}

extern "C" int btsbot_grad_buckets(btsbot_handle h, int capacity, int64_t* lo, int64_t* hi) {
  if (h == nullptr || lo == nullptr || hi == nullptr || capacity < h->n_buckets) {
    btsbot_set_error("grad_buckets: NULL argument or room for fewer than %d buckets", h ? h->n_buckets : 0);
    return BTSBOT_ERR_INVALID_ARG;
  }
  for (int i = 0; i < h->n_buckets; ++i) {
    lo[i] = h->bucket_lo[i];
    hi[i] = h->bucket_hi[i];
  }
  return h->n_buckets;
}

extern "C" int btsbot_wait_grad_bucket(btsbot_handle h, int bucket, void* stream) {
  if (h == nullptr || bucket < 0 || bucket >= h->n_buckets) {
    btsbot_set_error("wait_grad_bucket: bad handle or bucket %d", bucket);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!h->bucket_recorded) {
    btsbot_set_error("wait_grad_bucket: btsbot_backward() has not run on this handle");
    return BTSBOT_ERR_STATE;
  }
  h->bucket_waits_seen = true;   // (the next backward records the per-stage events)
  HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, h->bucket_fine ? h->bucket_ev[bucket] : h->bwd_done, 0));
  return BTSBOT_OK;
}

// ---- the exchange step inside the C ABI (btsbot_allreduce_grads) ------------------------
// RCCL is resolved at the first call with dlopen / dlsym, not linked: a process that never trains across GPUs does
// not load it, and a host that already has an RCCL (PyTorch ships its own copy) keeps using that one -- the
// communicator the caller passes in must come from the library this resolves to (by soname: the copy already loaded
// wins).
namespace {
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_reduce_scatter_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*nccl_comm_int_fn)(void*, int*);
struct RcclApi {
  nccl_allreduce_fn all_reduce = nullptr;
  nccl_reduce_scatter_fn reduce_scatter = nullptr;
  nccl_allgather_fn all_gather = nullptr;
  nccl_comm_int_fn count = nullptr, user_rank = nullptr;
  std::string error;   // why the library or a symbol could not be resolved (dlerror() is consumed by its first reader)
};
const RcclApi& rccl_api() {
  static const RcclApi api = [] {
    RcclApi a;
    void* lib = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib != nullptr) break;
    }
    if (lib == nullptr) {
      const char* e = dlerror();
      a.error = std::string("dlopen(librccl.so.1): ") + (e != nullptr ? e : "not found");
      return a;
    }
    auto sym = [&](const char* name) -> void* {
      void* p = dlsym(lib, name);
      if (p == nullptr && a.error.empty()) {
        const char* e = dlerror();
        a.error = std::string("dlsym(") + name + "): " + (e != nullptr ? e : "missing");
      }
      return p;
    };
    a.all_reduce = reinterpret_cast<nccl_allreduce_fn>(sym("ncclAllReduce"));
    a.reduce_scatter = reinterpret_cast<nccl_reduce_scatter_fn>(sym("ncclReduceScatter"));
    a.all_gather = reinterpret_cast<nccl_allgather_fn>(sym("ncclAllGather"));
    a.count = reinterpret_cast<nccl_comm_int_fn>(sym("ncclCommCount"));
    a.user_rank = reinterpret_cast<nccl_comm_int_fn>(sym("ncclCommUserRank"));
    return a;
  }();
  return api;
}
}  // namespace

// Two forms of the exchange (btsbot_set_option(h, "exchange", 0 | 1)):
//   0  one ncclAllReduce per span (RCCL picks ring / tree);
//   1  the direct form SURVEY.md section 5.8 recommends for xGMI's point-to-point links: ncclReduceScatter of the span
//      (every rank ends up owning the sum of its 1 / N slice) followed by ncclAllGather, both in place; what is left of
//      a span after N equal slices (< N floats) goes through a small ncclAllReduce.
extern "C" int btsbot_allreduce_grads(btsbot_handle h, void* nccl_comm, float* grads, int nspans, const int* bucket,
                                      const int64_t* lo, const int64_t* hi, void* stream) {
  if (h == nullptr || nccl_comm == nullptr || grads == nullptr || nspans < 0 || (nspans > 0 && (bucket == nullptr || lo == nullptr || hi == nullptr))) {
    btsbot_set_error("allreduce_grads: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!h->bucket_recorded) {
    btsbot_set_error("allreduce_grads: btsbot_backward() has not run on this handle");
    return BTSBOT_ERR_STATE;
  }
  if (h->last_grad_arena != nullptr && grads != h->last_grad_arena) {
    // the bucket events belong to the arena the last btsbot_backward() wrote: any other pointer would be reduced behind
    // events that say nothing about it
    btsbot_set_error("allreduce_grads: `grads` (%p) is not the arena the last btsbot_backward() wrote (%p)", (void*)grads,
                     (void*)h->last_grad_arena);
    return BTSBOT_ERR_INVALID_ARG;
  }
  h->bucket_waits_seen = true;
  const RcclApi& api = rccl_api();
  if (api.all_reduce == nullptr || (h->exchange_mode == 1 && (api.reduce_scatter == nullptr || api.all_gather == nullptr ||
                                                              api.count == nullptr || api.user_rank == nullptr))) {
    btsbot_set_error("allreduce_grads: cannot load RCCL (%s)", api.error.empty() ? "symbol missing" : api.error.c_str());
    return BTSBOT_ERR_STATE;
  }
  int nranks = 1, rank = 0;
  if (h->exchange_mode == 1) {
    if (api.count(nccl_comm, &nranks) != 0 || api.user_rank(nccl_comm, &rank) != 0 || nranks < 1 || rank < 0 || rank >= nranks) {
      btsbot_set_error("allreduce_grads: ncclCommCount / ncclCommUserRank failed on this communicator");
      return BTSBOT_ERR_HIP;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  if (h->xchg == nullptr || h->xchg_for[0] != st || h->xchg_for[1] != h->side) {
    // The collectives run long kernels: on the caller's pipe (or the side stream's) they would take turns with the
    // backward exactly as a badly placed side stream does (create_side_stream).  Same measurement, against both.
    if (h->xchg != nullptr) {
      HIP_TRY(hipStreamSynchronize(h->xchg));
      (void)hipStreamDestroy(h->xchg);
      h->xchg = nullptr;
    }
    hipStream_t busy[2] = {st, h->side};
    TRY(pick_apart_stream(h, busy, h->side != nullptr ? 2 : 1, "exchange", &h->xchg, &h->xchg_apart));
    h->xchg_for[0] = st;
    h->xchg_for[1] = h->side;
    if (h->xchg_done == nullptr) HIP_TRY(hipEventCreateWithFlags(&h->xchg_done, hipEventDisableTiming));
  }
  for (int i = 0; i < nspans; ++i) {
    if (bucket[i] < 0 || bucket[i] >= h->n_buckets || lo[i] < 0 || hi[i] > h->total_floats || lo[i] >= hi[i]) {
      btsbot_set_error("allreduce_grads: span %d (bucket %d, [%lld, %lld)) is outside the arena", i, bucket[i],
                       (long long)lo[i], (long long)hi[i]);
      return BTSBOT_ERR_INVALID_ARG;
    }
    // the collective of a span starts as soon as the backward pass has written its bucket, on the library's exchange
    // stream: the rest of the backward keeps the caller's stream
    HIP_TRY(hipStreamWaitEvent(h->xchg, h->bucket_fine ? h->bucket_ev[bucket[i]] : h->bwd_done, 0));   // (ctx.h: bucket_fine)
    float* base = grads + lo[i];
    const size_t n = (size_t)(hi[i] - lo[i]);
    int rc = 0;
    const char* what = "ncclAllReduce";
    if (h->exchange_mode == 1 && nranks > 1) {
      const size_t slice = n / (size_t)nranks, body = slice * (size_t)nranks;
      if (slice > 0) {
        what = "ncclReduceScatter";
        rc = api.reduce_scatter(base, base + (size_t)rank * slice, slice, /* ncclFloat32 */ 7, /* ncclSum */ 0, nccl_comm, h->xchg);
        if (rc == 0) {
          what = "ncclAllGather";
          rc = api.all_gather(base + (size_t)rank * slice, base, slice, 7, nccl_comm, h->xchg);
        }
      }
      if (rc == 0 && body < n) {
        what = "ncclAllReduce (remainder)";
        rc = api.all_reduce(base + body, base + body, n - body, 7, 0, nccl_comm, h->xchg);
      }
    } else {
      rc = api.all_reduce(base, base, n, /* ncclFloat32 */ 7, /* ncclSum */ 0, nccl_comm, h->xchg);
    }
    if (rc != 0) {
      btsbot_set_error("allreduce_grads: %s of span %d returned %d", what, i, rc);
      return BTSBOT_ERR_HIP;
    }
  }
  HIP_TRY(hipEventRecord(h->xchg_done, h->xchg));
  HIP_TRY(hipStreamWaitEvent(st, h->xchg_done, 0));   // the optimiser step on `stream` sees the reduced gradients
  return BTSBOT_OK;
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

// ---------------------------------------------------------------------------------------
// op-level entry points
// ---------------------------------------------------------------------------------------
extern "C" int btsbot_op_gemm(int prec, int epi, const void* X, const void* W, const float* bias,
                              const float* gamma, const float* resid, void* out, int M, int N,
                              int K, void* stream) {
  if (X == nullptr || W == nullptr || bias == nullptr || out == nullptr || M < 0 || N < 1 ||
      K < 1 || (epi == EPI_RESID && (gamma == nullptr || resid == nullptr))) {
    btsbot_set_error("op_gemm: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((epi == EPI_GELU_SAVE || epi == EPI_DGELU) && resid == nullptr) {   // (every precision: the pre-activation's buffer)
    btsbot_set_error("op_gemm: this epilogue needs resid (the pre-activation)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (prec == BTSBOT_F16X2) {   // fp32 X and W: W split into its f16 head and remainder planes here, stream-ordered
    hipStream_t st = (hipStream_t)stream;
    if (M == 0) return BTSBOT_OK;
    // (the training epilogues whose X is a gradient: X's largest magnitude sets its power-of-two scale, as in the step)
    const bool grad_x = epi == EPI_DGELU || epi == EPI_PLAIN;
    void* wsplit = nullptr;
    HIP_TRY(hipMallocAsync(&wsplit, (size_t)N * K * 4 + AMAX_WORDS * 4, st));
    unsigned* xamax = grad_x ? reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(wsplit) + (size_t)N * K * 4) : nullptr;
    const float* w = reinterpret_cast<const float*>(W);
    int s = launch_cast(BTSBOT_F16, w, wsplit, (int64_t)N * K, st);
    if (s == BTSBOT_OK)
      s = launch_rowscale_cast_lo(w, nullptr, reinterpret_cast<f16_t*>(wsplit) + (size_t)N * K, N, K, st);
    if (s == BTSBOT_OK && grad_x) {
      if (hipMemsetAsync(xamax, 0, AMAX_WORDS * 4, st) != hipSuccess) s = BTSBOT_ERR_HIP;
      if (s == BTSBOT_OK) s = launch_copy_amax(reinterpret_cast<const float*>(X), nullptr, (long)M * K, xamax, st);
    }
    if (s == BTSBOT_OK)
      s = launch_gemm_x2_train(epi, reinterpret_cast<const float*>(X), wsplit, bias, gamma, resid,
                               reinterpret_cast<float*>(out), M, N, K, xamax, nullptr, st);
    HIP_TRY(hipFreeAsync(wsplit, st));
    return s;
  }
  return launch_gemm(prec, epi, X, W, bias, gamma, resid, out, M, N, K, (hipStream_t)stream);
}

extern "C" int btsbot_op_wgrad(int prec, const void* Dv, const void* Av, float* out, float* colsum, int M, int N, int K,
                               void* stream) {
  if (Dv == nullptr || Av == nullptr || out == nullptr || M < 0 || N < 1 || K < 1) {
    btsbot_set_error("op_wgrad: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return BTSBOT_OK;
  if (prec == BTSBOT_BF16 || prec == BTSBOT_F16) {
    // 16-bit D and A, the training step's form: slice partials in a stream-ordered scratch + the two-pass reduction
    if ((N & 7) || (K & 7) || ((uintptr_t)Dv & 15) || ((uintptr_t)Av & 15)) {
      btsbot_set_error("op_wgrad: N=%d K=%d must be multiples of 8 and D, A 16-byte aligned", N, K);
      return BTSBOT_ERR_INVALID_ARG;
    }
    const size_t part_floats = (size_t)16 << 20;
    void* part = nullptr;
    HIP_TRY(hipMallocAsync(&part, part_floats * 4, st));
    const int s = launch_wgrad16(prec, Dv, Av, out, colsum, M, N, K, K, st, reinterpret_cast<float*>(part), part_floats);
    HIP_TRY(hipFreeAsync(part, st));
    return s;
  }
  const float* D = reinterpret_cast<const float*>(Dv);
  const float* A = reinterpret_cast<const float*>(Av);
  if (prec == BTSBOT_F32) return launch_wgrad_cs_f32(D, A, out, colsum, M, N, K, K, st);
  if (prec != BTSBOT_F16X2) {
    btsbot_set_error("op_wgrad: precision %d (BTSBOT_F32, BTSBOT_BF16, BTSBOT_F16 or BTSBOT_F16X2)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  // split operands as in the split training step's stem: the largest magnitudes of D and of A set their power-of-two
  // scales (for an O(1) A, as the other products of the step have, the scale changes nothing but the exponents); slice
  // partials + fixed-order sum
  if ((N & 15) || (K & 15)) {
    btsbot_set_error("op_wgrad: N=%d K=%d must be multiples of 16", N, K);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const size_t part_floats = (size_t)16 << 20;
  void* scratch = nullptr;
  HIP_TRY(hipMallocAsync(&scratch, part_floats * 4 + 2 * AMAX_WORDS * 4, st));
  float* part = reinterpret_cast<float*>(scratch);
  unsigned* damax = reinterpret_cast<unsigned*>(part + part_floats);
  unsigned* aamax = damax + AMAX_WORDS;
  int s = hipMemsetAsync(damax, 0, 2 * AMAX_WORDS * 4, st) == hipSuccess ? BTSBOT_OK : BTSBOT_ERR_HIP;
  if (s == BTSBOT_OK) s = launch_copy_amax(D, nullptr, (long)M * N, damax, st);
  if (s == BTSBOT_OK) s = launch_copy_amax(A, nullptr, (long)M * K, aamax, st);
  if (s == BTSBOT_OK) s = launch_wgrad_x2(D, A, out, colsum, M, N, K, K, damax, aamax, st, part, part_floats, nullptr);
  HIP_TRY(hipFreeAsync(scratch, st));
  return s;
}

extern "C" int btsbot_op_gemm_gated(int prec, const void* X, const float* gate, int rows_per_alert, const void* W,
                                    const float* resid, float* out, int M, int N, int K, void* stream) {
  if (X == nullptr || gate == nullptr || W == nullptr || resid == nullptr || out == nullptr || M < 0 || N < 1 ||
      K < 1 || rows_per_alert < 1) {
    btsbot_set_error("op_gemm_gated: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) return BTSBOT_OK;
  if (prec != BTSBOT_F16X2)
    return launch_gemm_gated(prec, X, gate, rows_per_alert, W, resid, out, M, N, K, st);
  // fp32 X and W: W split into its f16 head and remainder planes here, stream-ordered (as btsbot_op_gemm does)
  void* wsplit = nullptr;
  HIP_TRY(hipMallocAsync(&wsplit, (size_t)N * K * 4, st));
  const float* w = reinterpret_cast<const float*>(W);
  int s = launch_cast(BTSBOT_F16, w, wsplit, (int64_t)N * K, st);
  if (s == BTSBOT_OK) s = launch_rowscale_cast_lo(w, nullptr, reinterpret_cast<f16_t*>(wsplit) + (size_t)N * K, N, K, st);
  if (s == BTSBOT_OK)
    s = launch_gemm_x2_gated(reinterpret_cast<const float*>(X), gate, rows_per_alert, wsplit, resid, out, M, N, K, st);
  HIP_TRY(hipFreeAsync(wsplit, st));
  return s;
}

extern "C" int btsbot_op_gemm_resid_ln(int prec, const void* X, const void* W, const float* resid, float* out, int batch,
                                       int M, int N, int K, const float* ln_w, const float* ln_b, void* ln_out,
                                       void* stream) {
  if (X == nullptr || W == nullptr || resid == nullptr || out == nullptr || batch < 1 || M < 1 || N < 1 || K < 1 ||
      (ln_out != nullptr && (ln_w == nullptr || ln_b == nullptr))) {
    btsbot_set_error("op_gemm_resid_ln: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  // the kernel reads a bias and a layer scale; this form has neither: zeros and ones, stream-ordered
  void* ones = nullptr;
  HIP_TRY(hipMallocAsync(&ones, (size_t)N * 8, st));
  float* zero_bias = reinterpret_cast<float*>(ones);
  float* one_gamma = zero_bias + N;
  int s = BTSBOT_OK;
  if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(zero_bias), 0, N, st) != hipSuccess ||
      hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(one_gamma), 0x3f800000, N, st) != hipSuccess)   // 1.0f
    s = BTSBOT_ERR_HIP;
  if (s == BTSBOT_OK)
    s = launch_gemm2_batched_resid(prec, X, W, zero_bias, one_gamma, resid, out, batch, M, N, K, st, ln_w, ln_b, ln_out);
  HIP_TRY(hipFreeAsync(ones, st));
  return s;
}

extern "C" int btsbot_op_dwconv_ln(int prec, const float* x, const float* w, const float* bias,
                                   const float* ln_w, const float* ln_b, void* xn, int B, int HW,
                                   int C, void* stream) {
  if (x == nullptr || w == nullptr || bias == nullptr || ln_w == nullptr || ln_b == nullptr ||
      xn == nullptr || B < 0) {
    btsbot_set_error("op_dwconv_ln: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_dwconv_ln(prec, x, w, bias, ln_w, ln_b, xn, B, HW, C, (hipStream_t)stream);
}

extern "C" int btsbot_op_stem(const float* img, const float* w, const float* bias,
                              const float* ln_w, const float* ln_b, float* out, int B, int C0,
                              void* stream) {
  if (img == nullptr || w == nullptr || bias == nullptr || ln_w == nullptr || ln_b == nullptr ||
      out == nullptr || B < 0) {
    btsbot_set_error("op_stem: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_stem(img, w, bias, ln_w, ln_b, out, B, C0, (hipStream_t)stream);
}

extern "C" int btsbot_op_ln_patch(int prec, const float* x, const float* ln_w, const float* ln_b,
                                  void* patches, int B, int HW, int Cin, void* stream) {
  if (x == nullptr || ln_w == nullptr || ln_b == nullptr || patches == nullptr || B < 0 ||
      HW < 2) {
    btsbot_set_error("op_ln_patch: invalid argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_ln_patch(prec, x, ln_w, ln_b, patches, B, HW, Cin, (hipStream_t)stream);
}

// ---- MaxViT kernels one at a time.  Parameters come in the state-dict layout (fp32); the operand images are built in a
// stream-ordered scratch by the pack launchers the handle uses (maxvit_pack), so those are exercised as well.
namespace {

// one stream-ordered allocation, carved into 256-byte aligned pieces; released on the same stream when it goes out of scope
struct OpScratch {
  hipStream_t st;
  unsigned char* base = nullptr;
  size_t cur = 0, total = 0;
  explicit OpScratch(hipStream_t s) : st(s) {}
  ~OpScratch() {
    if (base != nullptr) (void)hipFreeAsync(base, st);
  }
  size_t reserve(size_t bytes) {
    const size_t o = total;
    total += (bytes + 255) / 256 * 256;
    return o;
  }
  int alloc() { return hipMallocAsync(reinterpret_cast<void**>(&base), total ? total : 256, st) == hipSuccess ? BTSBOT_OK : BTSBOT_ERR_HIP; }
  template <typename P = void> P* at(size_t off) const { return reinterpret_cast<P*>(base + off); }
};

bool mv_prec16(int prec) { return prec == BTSBOT_BF16 || prec == BTSBOT_F16; }
bool mv_prec_any(int prec) { return prec == BTSBOT_F32 || mv_prec16(prec); }

int mv_op_bad(const char* who, const char* what) {
  btsbot_set_error("%s: %s", who, what);
  return BTSBOT_ERR_INVALID_ARG;
}

#define OP_TRY(call)                \
  do {                              \
    int _s = (call);                \
    if (_s != BTSBOT_OK) return _s; \
  } while (0)

}  // namespace

extern "C" int btsbot_op_mv_attn(int prec, int impl, const void* qkv, const float* table, void* out, int B, int H, int C,
                                 int grid_mode, void* stream) {
  if (qkv == nullptr || table == nullptr || out == nullptr) return mv_op_bad("op_mv_attn", "null pointer");
  if (B < 0 || H < 7 || H % 7 != 0 || C < 32 || C % 32 != 0 || (grid_mode != 0 && grid_mode != 1) || (impl != 0 && impl != 1)) {
    btsbot_set_error("op_mv_attn: bad shape B=%d H=%d C=%d grid_mode=%d impl=%d (H a multiple of 7, C of 32)", B, H, C,
                     grid_mode, impl);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (impl == 0 ? !mv_prec_any(prec) : !mv_prec16(prec)) {
    btsbot_set_error("op_mv_attn: precision %d (impl 0: BTSBOT_F32 / BF16 / F16; impl 1: BF16 / F16)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int heads = C / 32;
  if ((long)B * (H / 7) * (H / 7) * heads > 0x7fffffffL) return mv_op_bad("op_mv_attn", "too many (alert, partition, head) units");
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  OpScratch sc(st);
  const size_t o_bias = sc.reserve((size_t)heads * (impl == 0 ? 2401 : 4096) * 4);
  OP_TRY(sc.alloc());
  float* bias = sc.at<float>(o_bias);
  if (impl == 0) {
    OP_TRY(launch_mv_pack_relbias(table, bias, heads, st));
    return launch_mv_attn(prec, qkv, bias, out, B, H, C, grid_mode, st);
  }
  OP_TRY(launch_mv_pack_relbias64(table, bias, heads, st));
  return launch_mv_attn_mfma(prec, qkv, bias, out, B, H, C, grid_mode, st);
}

extern "C" int btsbot_op_mv_attn_block(int prec, const void* xn, float* x, void* xn2, const float* qkv_w, const float* qkv_b,
                                       const float* proj_w, const float* proj_b, const float* table, const float* ln2_w,
                                       const float* ln2_b, int B, int H, int grid_mode, void* stream) {
  if (xn == nullptr || x == nullptr || xn2 == nullptr || qkv_w == nullptr || qkv_b == nullptr || proj_w == nullptr ||
      proj_b == nullptr || table == nullptr || ln2_w == nullptr || ln2_b == nullptr)
    return mv_op_bad("op_mv_attn_block", "null pointer");
  if (B < 0 || H < 7 || H % 7 != 0 || (grid_mode != 0 && grid_mode != 1)) {
    btsbot_set_error("op_mv_attn_block: bad shape B=%d H=%d grid_mode=%d (H a multiple of 7)", B, H, grid_mode);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int c = 64, heads = 2;
  if (!mv_attn_block_supported(prec, c)) {
    btsbot_set_error("op_mv_attn_block: precision %d (BTSBOT_BF16 or BTSBOT_F16)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((long)B * (H / 7) * (H / 7) > 0x7fffffffL) return mv_op_bad("op_mv_attn_block", "too many partitions");
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  OpScratch sc(st);
  const size_t o_qkv = sc.reserve((size_t)3 * c * c * 2), o_proj = sc.reserve((size_t)c * c * 2);
  const size_t o_bias = sc.reserve((size_t)heads * 4096 * 4);
  OP_TRY(sc.alloc());
  // (as maxvit_pack builds p_qkv / p_proj / p_bias64)
  OP_TRY(launch_cast(prec, qkv_w, sc.at(o_qkv), (int64_t)3 * c * c, st));
  OP_TRY(launch_cast(prec, proj_w, sc.at(o_proj), (int64_t)c * c, st));
  OP_TRY(launch_mv_pack_relbias64(table, sc.at<float>(o_bias), heads, st));
  return launch_mv_attn_block(prec, xn, x, xn2, sc.at(o_qkv), qkv_b, sc.at(o_proj), proj_b, sc.at<float>(o_bias), ln2_w,
                              ln2_b, B, H, c, grid_mode, st);
}

extern "C" int btsbot_op_mv_part(int prec, float* x, const float* ln1_w, const float* ln1_b, const float* qkv_w,
                                 const float* qkv_b, const float* proj_w, const float* proj_b, const float* table,
                                 const float* ln2_w, const float* ln2_b, const float* fc1_w, const float* fc1_b,
                                 const float* fc2_w, const float* fc2_b, const float* post_s, const float* post_b,
                                 void* post_out, int B, int H, int C, int grid_mode, void* stream) {
  if (x == nullptr || ln1_w == nullptr || ln1_b == nullptr || qkv_w == nullptr || qkv_b == nullptr || proj_w == nullptr ||
      proj_b == nullptr || table == nullptr)
    return mv_op_bad("op_mv_part", "null pointer");
  const bool mlp = fc1_w != nullptr;
  if (mlp ? (ln2_w == nullptr || ln2_b == nullptr || fc1_b == nullptr || fc2_w == nullptr || fc2_b == nullptr)
          : (ln2_w != nullptr || ln2_b != nullptr || fc1_b != nullptr || fc2_w != nullptr || fc2_b != nullptr))
    return mv_op_bad("op_mv_part", "norm2 / fc1 / fc2: all six pointers (both halves) or none (the attention half)");
  if (post_out != nullptr && (post_s == nullptr || post_b == nullptr)) return mv_op_bad("op_mv_part", "post_out needs post_s and post_b");
  if (B < 0 || H < 7 || H % 7 != 0 || (grid_mode != 0 && grid_mode != 1)) {
    btsbot_set_error("op_mv_part: bad shape B=%d H=%d grid_mode=%d (H a multiple of 7)", B, H, grid_mode);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!mv_part_supported(prec, C)) {
    btsbot_set_error("op_mv_part: unsupported (prec %d, C %d): BTSBOT_BF16 / BTSBOT_F16, C 64 / 128 / 256", prec, C);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  const int c = C, heads = C / 32;
  OpScratch sc(st);
  const size_t o_qkv = sc.reserve((size_t)3 * c * c * 2), o_proj = sc.reserve((size_t)c * c * 2);
  const size_t o_biasl = sc.reserve((size_t)heads * 4096 * 4);
  const size_t o_w1 = sc.reserve(mlp ? (size_t)4 * c * c * 2 : 0), o_w2 = sc.reserve(mlp ? (size_t)4 * c * c * 2 : 0);
  OP_TRY(sc.alloc());
  // (maxvit_pack's calls for a block that runs as mv_part_kernel)
  OP_TRY(launch_pack_s2p(prec, qkv_w, nullptr, sc.at(o_qkv), 3 * c, c, 0, 0, nullptr, st));
  OP_TRY(launch_pack_s2p(prec, proj_w, nullptr, sc.at(o_proj), c, c, 0, 0, nullptr, st));
  OP_TRY(launch_mv_pack_relbias_lanes(table, sc.at<float>(o_biasl), heads, st));
  if (mlp) {
    OP_TRY(launch_pack_s2p(prec, fc1_w, nullptr, sc.at(o_w1), 4 * c, c, 0, 0, nullptr, st));
    OP_TRY(launch_pack_s2p(prec, fc2_w, nullptr, sc.at(o_w2), c, 4 * c, 0, 0, nullptr, st));
  }
  MvPartW pw;
  memset(&pw, 0, sizeof(pw));
  pw.ln1w = ln1_w;
  pw.ln1b = ln1_b;
  pw.wqkvp = sc.at(o_qkv);
  pw.bqkv = qkv_b;
  pw.wprojp = sc.at(o_proj);
  pw.bproj = proj_b;
  pw.biasl = sc.at<float>(o_biasl);
  if (mlp) {
    pw.ln2w = ln2_w;
    pw.ln2b = ln2_b;
    pw.w1p = sc.at(o_w1);
    pw.b1 = fc1_b;
    pw.w2p = sc.at(o_w2);
    pw.b2 = fc2_b;
  }
  if (post_out != nullptr) {
    pw.post_s = post_s;
    pw.post_b = post_b;
    pw.post_out = post_out;
  }
  pw.stamps = nullptr;
  return launch_mv_part(prec, x, pw, B, H, C, grid_mode, st);
}

extern "C" int btsbot_op_mv_dw3_groups(int H, int C, int stride) {
  if (H < 1 || C < 8 || C % 8 != 0 || (stride != 1 && stride != 2) || (H / stride) % 7 != 0 || H / stride < 7) {
    btsbot_set_error("op_mv_dw3_groups: bad shape H=%d C=%d stride=%d", H, C, stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return mv_dw3s_groups(H, C, stride);
}

extern "C" int btsbot_op_mv_dw3(int prec, int impl, const void* in, const float* w, const float* scale, const float* bias,
                                void* out, float* part, int B, int H, int C, int stride, void* stream) {
  if (in == nullptr || w == nullptr || scale == nullptr || bias == nullptr || out == nullptr || (impl == 1 && part == nullptr))
    return mv_op_bad("op_mv_dw3", "null pointer");
  if (B < 0 || H < 1 || C < 4 || (stride != 1 && stride != 2) || H % stride != 0 || (impl != 0 && impl != 1)) {
    btsbot_set_error("op_mv_dw3: bad shape B=%d H=%d C=%d stride=%d impl=%d", B, H, C, stride, impl);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (impl == 0 ? !mv_prec_any(prec) : !mv_prec16(prec)) {
    btsbot_set_error("op_mv_dw3: precision %d (impl 0: BTSBOT_F32 / BF16 / F16; impl 1: BF16 / F16)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (impl == 0 ? C % 4 != 0 : (C % 8 != 0 || (H / stride) % 7 != 0 || H / stride < 7)) {
    btsbot_set_error("op_mv_dw3: impl %d cannot run H=%d C=%d stride=%d", impl, H, C, stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  OpScratch sc(st);
  const size_t o_w9 = sc.reserve((size_t)9 * C * 4);
  OP_TRY(sc.alloc());
  OP_TRY(launch_mv_pack_dw(w, scale, sc.at<float>(o_w9), C, st));
  if (impl == 0) return launch_mv_dw3(prec, in, sc.at<float>(o_w9), bias, out, B, H, C, stride, st);
  return launch_mv_dw3s(prec, in, sc.at<float>(o_w9), bias, out, part, B, H, C, stride, st);
}

extern "C" int btsbot_op_mv_mbconv_front_tiles(int H, int stride) {
  if (H < 1 || (stride != 1 && stride != 2) || H % stride != 0 || (H / stride) % (stride == 2 ? 7 : 14) != 0) {
    btsbot_set_error("op_mv_mbconv_front_tiles: bad shape H=%d stride=%d", H, stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return mv_mbconv_front_tiles(H, stride);
}

extern "C" int btsbot_op_mv_mbconv_front(int prec, const void* xn, const float* conv1_w, const float* b1, const float* dw_w,
                                         const float* dw_scale, const float* b2, void* m2, float* part, int B, int H,
                                         int CIN, int MID, int stride, void* stream) {
  if (xn == nullptr || conv1_w == nullptr || b1 == nullptr || dw_w == nullptr || dw_scale == nullptr || b2 == nullptr ||
      m2 == nullptr || part == nullptr)
    return mv_op_bad("op_mv_mbconv_front", "null pointer");
  if (B < 0 || H < 1 || CIN < 1 || MID < 1) {
    btsbot_set_error("op_mv_mbconv_front: bad shape B=%d H=%d CIN=%d MID=%d", B, H, CIN, MID);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!mv_mbconv_front_supported(prec, H, CIN, MID, stride)) {
    btsbot_set_error("op_mv_mbconv_front: unsupported (prec %d, H %d, CIN %d, MID %d, stride %d): 16-bit modes, CIN 64, "
                     "MID a multiple of 64, output maps of 28x28 and up in whole tiles", prec, H, CIN, MID, stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  OpScratch sc(st);
  const size_t o_w1 = sc.reserve((size_t)MID * CIN * 2), o_w9 = sc.reserve((size_t)9 * MID * 4);
  OP_TRY(sc.alloc());
  OP_TRY(launch_cast(prec, conv1_w, sc.at(o_w1), (int64_t)MID * CIN, st));
  OP_TRY(launch_mv_pack_dw(dw_w, dw_scale, sc.at<float>(o_w9), MID, st));
  return launch_mv_mbconv_front(prec, xn, sc.at(o_w1), b1, sc.at<float>(o_w9), b2, m2, part, B, H, CIN, MID, stride, st);
}

extern "C" int btsbot_op_mv_se(int prec, const void* y, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                               const float* fc2_b, float* gate, int B, int HW, int C, int RD, float inv_count, void* stream) {
  if (y == nullptr || fc1_w == nullptr || fc1_b == nullptr || fc2_w == nullptr || fc2_b == nullptr || gate == nullptr)
    return mv_op_bad("op_mv_se", "null pointer");
  if (B < 0 || HW < 1 || C < 4 || C % 4 != 0 || RD < 1 || RD > 512) {
    btsbot_set_error("op_mv_se: bad shape B=%d HW=%d C=%d RD=%d (C a multiple of 4, RD 1..512)", B, HW, C, RD);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!mv_prec_any(prec)) {
    btsbot_set_error("op_mv_se: precision %d (BTSBOT_F32 rows of partials, or a BTSBOT_BF16 / BTSBOT_F16 map)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  OpScratch sc(st);
  const size_t o_w2t = sc.reserve((size_t)C * RD * 4), o_scr = sc.reserve((size_t)B * (C + RD) * 4);
  OP_TRY(sc.alloc());
  OP_TRY(launch_transpose_f32(fc2_w, sc.at<float>(o_w2t), C, RD, st));   // (as maxvit_pack builds p_se2t)
  return launch_mv_se(prec, y, fc1_w, fc1_b, sc.at<float>(o_w2t), fc2_b, gate, sc.at<float>(o_scr), B, HW, C, RD, inv_count,
                      st);
}

extern "C" int btsbot_op_mv_stem(int prec, const float* img, const float* conv1_w, const float* bn_scale,
                                 const float* bn_shift, const float* conv2_w, float* out, int pooled, void* xn,
                                 const float* pre_scale, const float* pre_shift, int B, void* stream) {
  if (img == nullptr || conv1_w == nullptr || bn_scale == nullptr || bn_shift == nullptr || conv2_w == nullptr ||
      out == nullptr || (xn != nullptr && (pre_scale == nullptr || pre_shift == nullptr)))
    return mv_op_bad("op_mv_stem", "null pointer");
  if (B < 0 || (pooled != 0 && pooled != 1)) {
    btsbot_set_error("op_mv_stem: bad argument B=%d pooled=%d", B, pooled);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!mv_prec16(prec)) {
    btsbot_set_error("op_mv_stem: precision %d (BTSBOT_BF16 or BTSBOT_F16)", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (B == 0) return BTSBOT_OK;
  hipStream_t st = (hipStream_t)stream;
  OpScratch sc(st);
  const size_t o_w1 = sc.reserve((size_t)32 * 32 * 2), o_w2 = sc.reserve((size_t)64 * 288 * 2);
  const size_t o_mid = sc.reserve((size_t)B * 12544 * 32 * 2);
  OP_TRY(sc.alloc());
  OP_TRY(launch_mv_pack_stem1(prec, conv1_w, bn_scale, sc.at(o_w1), st));
  OP_TRY(launch_mv_stem1(prec, img, sc.at(o_w1), bn_shift, sc.at(o_mid), B, st));
  OP_TRY(launch_mv_pack_conv3(prec, conv2_w, sc.at(o_w2), 64, 32, st));
  return launch_mv_stem2(prec, sc.at(o_mid), sc.at(o_w2), out, pooled, xn, pre_scale, pre_shift, B, st);
}
#undef OP_TRY
