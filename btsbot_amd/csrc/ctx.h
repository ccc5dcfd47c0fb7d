// Internal: the handle behind btsbot_handle, and what the files that work on it (api.hip, forward.hip, train_step.hip,
// streams.hip, exchange.hip, the schedules and packers) call of each other.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "common.h"

struct ParamRec {
  std::string name;
  int64_t off, numel;
  int ndim;
  int shape[4];
  int is_buffer;
};

struct BlockPk {  // per ConvNeXt block: master offsets + packed offsets (bytes into `extra`; 0: no such image, pack.hip)
  int64_t gamma, dw_w, dw_b, ln_w, ln_b, fc1_w, fc1_b, fc2_w, fc2_b;
  size_t p_dw = 0, p_fc1 = 0, p_fc2 = 0, p_fused = 0;
  size_t p_s0par = 0;      // stage-0 / stage-1 blocks: parameter image for stage0b.hip / stage1b.hip
  size_t p_s0par_t = 0;    // ... for their keeping forms (training forward): the same image with f16 taps in every mode
  size_t p_fc2g = 0;       // diag(gamma) W2 in the operand type (megakernels fold the layer scale)
  size_t p_fc2g_h = 0;     // ... in f16, stage-0 blocks of a bf16 / fp8 handle: stage0b.hip's inference form hands fc2 f16 hidden activations
  size_t p_w1p = 0, p_w2p = 0;   // stage2p.hip / stage3.hip: fc1 / gamma * fc2 filters as MFMA A fragments
  size_t p_scales = 0;           // fp8 mode: {S1, 1/S1, S2, 1/S2} of those two
  size_t p_x2_w1 = 0, p_x2_w2g = 0;   // split mode, stages 0-1: fc1 / gamma * fc2 filters, f16 heads (stage0b / stage1b)
  size_t p_x2_w1lo = 0, p_x2_w2glo = 0;   // ... and their f16 remainders, same layouts
  size_t p_fc1t = 0, p_fc2t = 0;   // for the dgrad GEMMs: W1^T [C][4C], (diag(gamma) W2)^T [4C][C]
  size_t p_w1tp = 0, p_w2tp = 0;   // 256-channel blocks, training: the same two as MFMA A fragments (s2mlp_bwd.hip)
  // split training ("train_split"): p_fc1 / p_fc2 / p_fc1t / p_fc2t as f16 head + remainder planes, [n] heads then [n]
  // remainders (slots of their own: the per-op inference forward of the split mode reads the fp32 p_fc1 / p_fc2)
  size_t p_s_fc1 = 0, p_s_fc2 = 0, p_s_fc1t = 0, p_s_fc2t = 0;
};
struct DownPk {
  int64_t ln_w, ln_b, w, b;
  size_t p_w = 0, p_wt = 0;   // p_wt: [4*Cin][Cout] transpose of the packed filter (dgrad)
  size_t p_wp = 0;         // stage2p.hip / stage1b.hip: the filter as MFMA A fragments
  size_t p_x2_w = 0, p_x2_wlo = 0;   // split mode, stage0b's downsample: the filter's f16 heads / remainders, [Cout][q][Cin]
  size_t p_s_w = 0, p_s_wt = 0;      // split training: p_w / p_wt as f16 head + remainder planes (BlockPk::p_s_fc1)
};

constexpr int STAGE_HW[4] = {15, 7, 3, 1};

enum { CAT_STEM = 0, CAT_DWLN, CAT_FC1, CAT_FC2, CAT_LNPATCH, CAT_DOWN, CAT_HEAD, CAT_FUSED, CAT_STAGE0, CAT_STAGE1, CAT_STAGE2, CAT_S3FC1, CAT_S3FC2, CAT_HEAD16,
       CAT_MV_STEM, CAT_MV_G_STEM, CAT_MV_G_CONV1, CAT_MV_G_CONV3, CAT_MV_G_SC, CAT_MV_G_QKV, CAT_MV_G_PROJ, CAT_MV_G_FC1,
       CAT_MV_G_FC2, CAT_MV_FUSED, CAT_MV_FRONT, CAT_MV_ABLK, CAT_MV_ELT, CAT_MV_DW, CAT_MV_SE, CAT_MV_LN, CAT_MV_ATTN, CAT_MV_SMLP, CAT_MV_PART, NCAT };
const char* const CAT_NAMES[NCAT] = {"stem_kernel",       "dwconv_ln_kernel", "gemm_kernel<fc1,GELU>",
                                     "gemm_kernel<fc2,RESID>", "ln_patch_kernel", "gemm_kernel<down,BIAS>",
                                     "head_kernel", "fused_mlp_kernel", "stage0b_kernel", "stage1b_kernel",
                                     "stage2p_kernel", "s3_fc1_kernel", "s3_fc2_kernel", "head16_kernel",
                                     "mv_stem_im2col", "mv_gemm<stem>", "mv_gemm<conv1,SILU>", "mv_gemm<conv3,gated>",
                                     "mv_gemm<shortcut>", "mv_gemm<qkv>", "mv_gemm<proj,RESID>", "mv_gemm<fc1,GELU>",
                                     "mv_gemm<fc2,RESID>", "mv_fused_mlp", "mv_mbconv_front", "mv_attn_block", "mv_elementwise", "mv_dw3_kernel",
                                     "mv_se_kernel", "mv_ln_kernel", "mv_attn_kernel", "mv_streamed_mlp", "mv_partition"};
constexpr size_t PROF_MAX_LAUNCHES = 16384;

// Regions of the developer timestamp buffer (btsbot_debug_stamps; include/btsbot_hip.h lists them): offsets and sizes in
// uint64 entries.  Phase clocks come from one workgroup of a launch; a per-workgroup region holds [grid][2] start / end
// wall clocks and is passed only when the launch's grid fits (stamp_wgt in forward.hip).
constexpr size_t STAMP_TOTAL = 32 + 16384 + 64 + 2048;       // 18528
constexpr size_t STAMP_S0 = 0, STAMP_S0_N = 16;               // stage 0 phases (stage0b.hip)
constexpr size_t STAMP_S1 = 16, STAMP_S1_N = 16;              // stage 1 phases (stage1b.hip)
constexpr size_t STAMP_S0_WG = 32, STAMP_S0_WG_N = 8192;      // stage 0 per workgroup: 4096 workgroups of one alert
constexpr size_t STAMP_S1_WG = 8224, STAMP_S1_WG_N = 8192;    // stage 1 per workgroup in [0, 4096): 2048 workgroups of two
                                                              // alerts; its loop clocks at [4096, 4112) (stage1b.hip)
constexpr int STAMP_S0_MAX_WG = 4096, STAMP_S1_MAX_WG = 2048;
constexpr size_t STAMP_S2 = 16416, STAMP_S2_N = 64;           // stage 2 phases (stage2p.hip)
constexpr size_t STAMP_S3 = 16480, STAMP_S3_N = 16;           // stage 3 phases (stage3.hip)
constexpr size_t STAMP_HEAD16 = 17980, STAMP_HEAD16_N = 16;   // head16.hip
constexpr size_t STAMP_MV_PART = 32, STAMP_MV_PART_N = 64;    // MaxViT handles: mv_part_kernel, 32 for C = 256, then 32
                                                              // for C = 128; over stage 0's per-workgroup region, which
                                                              // only ConvNeXt handles write
constexpr bool stamp_fits(size_t off, size_t n) { return off + n <= STAMP_TOTAL; }
static_assert(stamp_fits(STAMP_S0, STAMP_S0_N) && stamp_fits(STAMP_S1, STAMP_S1_N) &&
                  stamp_fits(STAMP_S0_WG, STAMP_S0_WG_N) && stamp_fits(STAMP_S1_WG, STAMP_S1_WG_N) &&
                  stamp_fits(STAMP_S2, STAMP_S2_N) && stamp_fits(STAMP_S3, STAMP_S3_N) &&
                  stamp_fits(STAMP_HEAD16, STAMP_HEAD16_N) && stamp_fits(STAMP_MV_PART, STAMP_MV_PART_N),
              "a stamp region runs past the documented buffer");
static_assert(2 * STAMP_S0_MAX_WG <= STAMP_S0_WG_N && 2 * STAMP_S1_MAX_WG <= 4096 &&
                  STAMP_MV_PART + STAMP_MV_PART_N <= STAMP_S0_WG + STAMP_S0_WG_N,
              "a stamp region does not hold what is written into it");

// One packed operand image of a ConvNeXt / metadata / fusion handle (pack.hip: image_walk() lists them, pack_layout()
// reserves them, pack_params() writes them).
enum { IN_FULL = 1, IN_TRAIN = 2 };   // btsbot_pack_params() / the training re-pack btsbot_pack_params_train()
struct ImageEntry {
  const char* name;
  size_t* slot;           // the BlockPk / DownPk / btsbot_ctx field that holds its offset into `extra`
  size_t bytes;           // 0: another writer of a slot an entry in front reserved
  unsigned when;          // which packs write it (0: reserved only, e.g. the dgrad transposes before btsbot_reserve_train)
  bool early;             // training re-pack: stage0b_kernel's keeping form reads it -- written in front of pack_early_ev
  const size_t* reads;    // the packed image it is made from, listed in front of it (nullptr: made from the mirror)
  int op;                 // >= 0: a PackJob of the batch table (launchers.h: PACK_*), src / scale = master offsets (-1: none)
  int64_t src, scale;
  int R, Cc;
  long split_n;           // > 0: the f16 head + remainder planes of the split_n floats of *reads (SplitJob)
  // a dedicated packer; with op >= 0 the job's single-operand launch where the generic one does not fit.  None of the
  // three: written by the entry in front (a packer with two outputs)
  std::function<int(hipStream_t)> launch;
};

struct MaxVit;   // maxvit.hip
struct SidePick {
  hipStream_t caller, side;
  bool apart;
};

struct btsbot_ctx {
  btsbot_config cfg;
  bool has_image, has_meta;
  bool is_maxvit = false;   // image branch = timm maxvit_tiny_rw_224 (maxvit.hip) instead of ConvNeXt
  MaxVit* mv = nullptr;
  int n_comb;        // linear layers of the fusion MLP
  int comb_dims[4];
  int act;           // ACT_GELU / ACT_RELU of the heads
  int meta_trailing_act;
  std::vector<ParamRec> params;
  int64_t total_floats = 0;

  // master offsets
  int64_t stem_w, stem_b, stem_lnw, stem_lnb, hn_w = -1, hn_b = -1;
  std::vector<std::vector<BlockPk>> blocks;  // [stage][block]
  DownPk down[4];
  int64_t bn_w, bn_b, bn_rm, bn_rv, m1_w, m1_b, m2_w, m2_b;
  int64_t comb_w[3], comb_b[3];
  size_t p_m1 = 0, p_m2 = 0, p_comb[3] = {0, 0, 0}, p_bn_scale = 0, p_bn_shift = 0, p_stem16 = 0;
  size_t p_x2_stem = 0, p_x2_stemlo = 0;    // split mode: the stem filter's f16 heads / remainders (stage0b)
  int prec_head() const { return x2 ? BTSBOT_F16 : cfg.precision; }   // head16.hip splits its operands in every mode
  int prec_s01() const { return x2 ? BTSBOT_F16X2 : cfg.precision; }   // operand mode of stage0b.hip / stage1b.hip
  size_t p_m1h = 0, p_m2h = 0, p_combh[3] = {0, 0, 0};   // head16.hip: the Linear filters as split A fragments

  // which kernel runs what (schedule.h): sw = the HANDLE-scope switches as btsbot_create found them (INT_MIN: not set),
  // opt_* = what btsbot_set_option / btsbot_reserve_train asked for; resolve_schedule() makes `sched` of them
  int sw[SW_COUNT];
  bool opt_deterministic = false;   // btsbot_set_option("deterministic") / BTSBOT_AMD_DETERMINISTIC=1
  // btsbot_set_option("train_split"), BTSBOT_F16X2 ConvNeXt handles: the training step's 1x1 / downsample products (forward,
  // input gradients, filter gradients) run on split operands (gemm_x2.hip, wgrad_x2.hip) instead of the fp32 MFMA
  bool opt_train_split = false;
  bool opt_train_packs = false;     // also pack the dgrad transposes (set by btsbot_reserve_train)
  Schedule sched;

  // device memory
  float* mirror = nullptr;          // fp32 copy of the master arena (same offsets)
  unsigned char* extra = nullptr;   // transformed operands; offset 0 is reserved: a slot of 0 is an image that was never laid out
  unsigned char* image(size_t slot) const { return slot != 0 ? extra + slot : nullptr; }   // readers: IMG() below
  std::vector<ImageEntry> images;   // pack.hip
  size_t extra_fixed = 256;         // where they start: behind offset 0 and a MaxViT branch's images (maxvit_build_tables)
  void* pack_jobs[3] = {nullptr, nullptr, nullptr};   // (pack.hip) device tables of PackJob: [0] full pack, [1] training re-pack,
  int pack_njobs[3] = {0, 0, 0}, pack_blocks[3] = {0, 0, 0};   // [2] the part of [1] the stage-0 megakernel reads (s0_keep)
  hipEvent_t pack_early_ev = nullptr;   // recorded behind that part and the stage-0 parameter images (pack_sync_early)
  bool pack_early = false;              // the running re-pack recorded it
  size_t extra_bytes = 0;
  bool packed = false;
  bool packed_full = false;   // false after btsbot_pack_params_train(): inference-only operand images are stale

  unsigned char* ws = nullptr;
  bool ws_owned = true;             // false: the caller's memory (btsbot_use_workspace), never freed here
  size_t ws_bytes = 0;
  int max_chunk = 0;
  size_t o_x, o_x2, o_xn, o_h;      // workspace offsets
  // per-kernel-family timing with HIP events on the launch stream (btsbot_set_profile)
  bool prof_on = false;
  std::vector<hipEvent_t> prof_ev;   // pairs: [2i] before, [2i+1] after launch i
  std::vector<int> prof_cat;
  size_t prof_used = 0;

  int s2p_alerts_hint = 0; // btsbot_set_option("stage2p_alerts"): 0 = by rounds, 4 / 7 forced
  bool opt_forwards_in_flight = false;   // btsbot_set_option("forwards_in_flight"): other forwards run beside this handle's
  bool fp8 = false;        // created with BTSBOT_FP8: cfg.precision reads BTSBOT_BF16, stages 2-3 run fp8 operands
  bool x2 = false;         // created with BTSBOT_F16X2: cfg.precision reads BTSBOT_F32 (the schedule of every kernel without
                           // a split-operand form), the kernels that have one run it
  bool x2_tail_plain = false;   // BTSBOT_AMD_X2_TAIL_F16 (schedule.h)
  int prec_tail() const { return fp8 ? BTSBOT_FP8 : x2 ? (x2_tail_plain ? BTSBOT_F16 : BTSBOT_F16X2) : cfg.precision; }   // operand mode of stage2p.hip / stage3.hip
  int prec_down3() const { return x2 ? (x2_tail_plain ? BTSBOT_F16 : BTSBOT_F16X2) : cfg.precision; }   // ... of the last downsample inside stage2p.hip
  // image-branch training cache (backbone_train.hip)
  unsigned char* bbcache = nullptr;
  int bbcache_batch = 0;
  int64_t img_floats = 0;     // master-arena floats [0, img_floats) belong to the image branch
  const float* t_img = nullptr;   // triplets of the last training forward (stem backward re-reads them)
  void* split_jobs = nullptr;   // split training: the re-pack's SplitJob table (device), built on the first training pack
  int split_njobs = 0;
  bool bb_saved = false;      // the last training forward kept the image-branch activations
  // training cache (head_train.hip): activations of the last training-mode forward
  float* tcache = nullptr;
  int tcache_batch = 0, train_batch = 0;
  const uint8_t* t_meta_mask = nullptr;
  const uint8_t* t_comb_mask = nullptr;
  bool t_eval = false;        // the last keeping forward was the eval form (btsbot_forward_keep_eval)

  // gradient buckets in the order btsbot_backward() completes them (btsbot_grad_buckets / btsbot_wait_grad_bucket)
  int n_buckets = 0;
  int64_t bucket_lo[3] = {0, 0, 0}, bucket_hi[3] = {0, 0, 0};
  hipEvent_t bucket_ev[3] = {nullptr, nullptr, nullptr};
  bool bucket_recorded = false;
  // The per-stage bucket events cost the backward's chain a fork each (an event record between two kernels: ~6 us), so they
  // are recorded only once somebody has waited for a bucket (btsbot_wait_grad_bucket / btsbot_allreduce_grads: a
  // multi-GPU run, from its first step on).  bucket_fine: the LAST backward recorded bucket_ev[]; otherwise a waiter gets
  // an event recorded on that backward's stream at the time it asks (everything the backward queued is in front of it).
  bool bucket_waits_seen = false, bucket_fine = false;
  bool meta_join_pending = false;   // the metadata branch's training forward sits on the side stream and `st` has not joined it yet
  hipStream_t xchg = nullptr;        // btsbot_allreduce_grads: the stream its collectives run on
  float* det_scratch = nullptr;      // deterministic mode: the partial rows of its reductions (sized at btsbot_reserve_train)
  size_t det_floats = 0;
  int exchange_mode = 0;             // btsbot_set_option("exchange"): 0 all-reduce per span, 1 reduce-scatter + all-gather
  const float* last_grad_arena = nullptr;   // what the last btsbot_backward() wrote (the bucket events belong to it)
  hipEvent_t xchg_done = nullptr;
  // second stream of the image-branch backward (backbone_train.hip): filter-gradient GEMMs trail the dX chain on it
  hipStream_t side = nullptr;
  hipStream_t side_for = nullptr;    // the caller's stream h->side was chosen against (create_side_stream)
  bool side_apart = true;            // ... and was measured to run on another hardware pipe than it (false: none of 8 did)
  std::vector<SidePick> side_cache;  // one chosen side stream per caller stream this handle has seen (never re-probed)
  hipStream_t xchg_for[2] = {nullptr, nullptr};   // the (caller, side) pair h->xchg was placed against
  bool xchg_apart = true;
  hipEvent_t bwd_done = nullptr;     // recorded at the end of a backward that did not record the per-bucket events
  std::vector<hipEvent_t> side_ev;   // pool, side_used of them taken by the current btsbot_backward()
  size_t side_used = 0;
  // btsbot_pack_params_train() queues its packing launches on `side` behind the mirror copy: they then overlap the
  // first kernel of the training forward (the stem reads the fp32 mirror only).  Every consumer of the operand images
  // calls pack_sync() first.
  bool pack_on_side = false;

  unsigned long long* stamps = nullptr;   // btsbot_debug_stamps: STAMP_TOTAL entries, regions STAMP_* above
  bool debug = false;
  float* taps[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int last_chunk = 0;

  int esz() const { return cfg.precision == BTSBOT_F32 ? 4 : 2; }
};

// Fork / join of the backward's second stream.  side_fork: work queued on *sd afterwards sees everything queued on
// `st` so far (*sd = st when the second stream is off); side_join: `st` waits for everything queued on the side.
int create_side_stream(btsbot_ctx* h, hipStream_t caller);   // streams.hip: h->side, on another hardware queue than `caller`
// streams.hip: a new stream measured to run beside every stream of busy[] (else the last candidate, *apart = false + a warning)
int pick_apart_stream(btsbot_ctx* h, const hipStream_t* busy, int nbusy, const char* role, hipStream_t* out, bool* apart);
int side_fork(btsbot_ctx* h, hipStream_t st, hipStream_t* sd);
int side_join(btsbot_ctx* h, hipStream_t st);

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

// forward.hip: image branch of one chunk; *feat_out = [nb][dims[3]] fp32 features inside the workspace
int backbone_chunk(btsbot_ctx* h, const float* img, int nb, hipStream_t st, float** feat_out);

// the training step's halves (backbone_train.hip, head_train.hip), called by train_step.hip
size_t train_cache_floats(const btsbot_ctx* h, int M);
size_t bb_cache_bytes(const btsbot_ctx* h, int B);
int backbone_train_forward(btsbot_ctx* h, const float* img, int B, hipStream_t st, float** feat_out);
int backbone_train_backward(btsbot_ctx* h, const float* img, const float* dfeat, float* grads,
                            int B, hipStream_t st, float* d_img = nullptr);
float* train_cache_feat(btsbot_ctx* h, float* cache, int M);
int head_train_forward(btsbot_ctx* h, float* cache, const float* meta, float* logits,
                       float* scores, int M, const uint8_t* meta_mask, const uint8_t* comb_mask,
                       float* master, hipStream_t st, bool meta_done = false, bool eval = false);
int head_train_meta_forward(btsbot_ctx* h, float* cache, const float* meta, int M, const uint8_t* meta_mask, float* master,
                            hipStream_t st, bool eval = false);
int head_train_backward(btsbot_ctx* h, float* cache, const float* dlogits, float* grads, int M,
                        int need_meta, int need_image, float** dfeat_out,
                        const uint8_t* meta_mask, const uint8_t* comb_mask, hipStream_t st, float* d_meta = nullptr,
                        bool eval = false);

// h->extra + slot for a reader or a packer.  An image the layout never reserved ends the calling function (or lambda)
// with BTSBOT_ERR_STATE and its name, in front of the launch it was meant for.
#define IMG(h, slot)                                                                            \
  ({                                                                                            \
    unsigned char* img_ = (h)->image(slot);                                                     \
    if (img_ == nullptr) {                                                                      \
      btsbot_set_error("the packed operand image %s does not exist on this handle", #slot);   \
      return (int)BTSBOT_ERR_STATE;                                                              \
    }                                                                                           \
    img_;                                                                                       \
  })
#define IMG_F32(h, slot) reinterpret_cast<const float*>(IMG(h, slot))

// pack.hip
int pack_layout(btsbot_ctx* h);       // lists the images, reserves their slots behind extra_fixed, sets extra_bytes
int pack_params(btsbot_ctx* h, const float* master, hipStream_t st, bool train_only);
int pack_invalidate(btsbot_ctx* h);   // a schedule field the image list reads has changed (train_packs): new list, new job tables
void pack_release(btsbot_ctx* h);     // btsbot_destroy
int pack_sync(btsbot_ctx* h, hipStream_t st);
int pack_sync_early(btsbot_ctx* h, hipStream_t st);   // only what stage0b_kernel reads (else = pack_sync)

// stage_args.hip: the argument blocks of the ConvNeXt stage kernels with every parameter pointer the handle holds
// filled in, everything else zero.  keep: the keeping form of the training forward (bf16 / f16: stage-0 / stage-1
// parameter images with f16 taps, no split-mode remainder planes, no fp8 scales).
struct Stage0Args;
struct Stage1Args;
struct Stage2pArgs;
struct Stage3Args;
int stage0_args(const btsbot_ctx* h, bool keep, Stage0Args* out);
int stage1_args(const btsbot_ctx* h, bool keep, Stage1Args* out);
int stage2p_args(const btsbot_ctx* h, bool keep, Stage2pArgs* out);
int stage3_args(const btsbot_ctx* h, Stage3Args* out);
