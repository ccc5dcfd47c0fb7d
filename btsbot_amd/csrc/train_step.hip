// The training step of the C ABI: btsbot_reserve_train, the training-mode forward (batch statistics + dropout; the image
// branch in backbone_train.hip / maxvit_train.hip, the heads in head_train.hip), btsbot_backward, and the gradient
// buckets it completes.
#include <algorithm>

#include "ctx.h"
#include "maxvit.h"

extern "C" int btsbot_reserve_train(btsbot_handle h, int max_batch, int with_image_grads) {
  if (h == nullptr || max_batch < 1) {
    btsbot_set_error("reserve_train: bad argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  // (MaxViT: with_image_grads = 1 trains the branch -- BatchNorm2d batch statistics, maxvit_train.hip; = 0 serves heads
  //  over a frozen, eval-mode branch with the inference kernels)
  const bool want_bb = with_image_grads && h->has_image;
  if (h->sched.deterministic) {   // partial rows of the batch reductions (device_math.h: det_add), sized by the batch: 256 KB per alert,
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

// The keeping forward in its two forms.  eval: BatchNorm1d on running statistics, dropout the identity, no arena
// (btsbot_forward_keep_eval); otherwise btsbot_forward_train as it always was.
static int forward_keep(btsbot_handle h, const float* triplets, const float* meta, float* logits, float* scores, int batch,
                        const uint8_t* meta_mask, const uint8_t* comb_mask, float* master_arena, int keep_image_activations,
                        void* stream, bool eval) {
  if (h == nullptr || logits == nullptr || batch < 1) {
    btsbot_set_error("forward_train: NULL handle/logits or empty batch");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (eval && h->is_maxvit) {
    btsbot_set_error("forward_keep_eval: the MaxViT wirings have no eval-form keeping forward");
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
  if (!eval && h->has_meta && ((c.meta_dropout > 0.f && meta_mask == nullptr) || c.meta_dropout >= 1.f)) {
    btsbot_set_error("forward_train: metadata dropout %.3f needs a keep-mask", c.meta_dropout);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (!eval && h->n_comb > 1 && ((c.comb_dropout > 0.f && comb_mask == nullptr) || c.comb_dropout >= 1.f)) {
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
        TRY(head_train_meta_forward(h, h->tcache, meta, batch, meta_mask, master_arena, sd, eval));
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
                         master_arena, st, meta_done, eval));
  h->train_batch = batch;
  h->t_meta_mask = eval ? nullptr : meta_mask;
  h->t_comb_mask = eval ? nullptr : comb_mask;
  h->t_eval = eval;
  return BTSBOT_OK;
}

extern "C" int btsbot_forward_train(btsbot_handle h, const float* triplets, const float* meta,
                                    float* logits, float* scores, int batch,
                                    const uint8_t* meta_mask, const uint8_t* comb_mask,
                                    float* master_arena, int keep_image_activations,
                                    void* stream) {
  return forward_keep(h, triplets, meta, logits, scores, batch, meta_mask, comb_mask, master_arena, keep_image_activations,
                      stream, false);
}

extern "C" int btsbot_forward_keep_eval(btsbot_handle h, const float* triplets, const float* meta, float* logits,
                                        float* scores, int batch, int keep_image_activations, void* stream) {
  return forward_keep(h, triplets, meta, logits, scores, batch, nullptr, nullptr, nullptr, keep_image_activations, stream, true);
}

extern "C" int btsbot_backward(btsbot_handle h, const float* dlogits, float* grad_arena,
                               int need_meta_grads, int need_image_grads, void* stream) {
  return btsbot_backward_inputs(h, dlogits, grad_arena, need_meta_grads, need_image_grads, nullptr, nullptr, stream);
}

extern "C" int btsbot_backward_inputs(btsbot_handle h, const float* dlogits, float* grad_arena, int need_meta_grads,
                                      int need_image_grads, float* d_triplets, float* d_meta, void* stream) {
  if (h == nullptr || dlogits == nullptr || grad_arena == nullptr) {
    btsbot_set_error("backward: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((d_triplets != nullptr || d_meta != nullptr) && h->is_maxvit) {
    btsbot_set_error("backward_inputs: input gradients of the MaxViT wirings are not built");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((d_triplets != nullptr && !h->has_image) || (d_meta != nullptr && !h->has_meta)) {
    btsbot_set_error("backward_inputs: this wiring has no %s input", d_triplets != nullptr && !h->has_image ? "image" : "metadata");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (d_triplets != nullptr) need_image_grads = 1;   // the triplets' gradient is the end of the image branch's backward
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
                          need_img, &dfeat, h->t_meta_mask, h->t_comb_mask, st, d_meta, h->t_eval));
  if (need_img) {
    if (h->is_maxvit) {
      TRY(side_join(h, st));
      TRY(maxvit_train_backward(h, h->t_img, dfeat, grad_arena, h->train_batch, st));   // records the bucket event
    } else {
      TRY(backbone_train_backward(h, h->t_img, dfeat, grad_arena, h->train_batch, st, d_triplets));   // records the bucket events
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
