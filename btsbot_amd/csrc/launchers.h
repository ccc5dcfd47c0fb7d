// The launcher prototypes of libbtsbot_hip.so and the argument structs that travel with them, grouped by the source file
// that defines them, in the Makefile's order.  All launchers return btsbot_status.  Part of common.h, which includes it
// behind the types (include common.h, not this file).
#pragma once

enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2 };
enum { EPI_GELU = 0, EPI_RESID = 1, EPI_BIAS = 2, EPI_GELU_SAVE = 3, EPI_DGELU = 4, EPI_PLAIN = 5,
       EPI_SILU = 6, EPI_BIAS_T = 7 };

// ---- pack.hip: parameter packing helpers
int launch_cast(int prec, const float* src, void* dst, int64_t n, hipStream_t st);
// One launch for a table of operand-packing jobs (the per-step re-pack of the training loop is ~75 of these,
// each a 2-5 us kernel: launch-floor bound one by one).  The table lives in device memory; job j owns blocks
// [blk0_j, blk0_{j+1}).  ops: the element maps of cast / transpose_f32 / transpose_cast / pack_down / pack_down_t.
// PACK_TFRAG: the transpose-cast's result [Cc][R] as 16x16x32 MFMA A fragments [row tile][k-step][lane][8] (s2mlp_bwd.hip)
// PACK_FRAG: src [R][Cc] (x scale[row]) as 16x16x32 MFMA A fragments [row tile][k-step][lane][8] (stage2p.hip's filters in the
// training re-pack); PACK_FRAG_DOWN: a downsample filter [R = Cout][Cc = Cin][2][2] likewise with k = (2 ky + kx) * Cin + c
enum { PACK_CAST = 0, PACK_TRANSPOSE_F32 = 1, PACK_TRANSPOSE_CAST = 2, PACK_DOWN = 3, PACK_DOWN_T = 4, PACK_TFRAG = 5, PACK_FRAG = 6,
       PACK_FRAG_DOWN = 7 };
struct PackJob {
  const float* src;
  const float* scale;   // PACK_TRANSPOSE_CAST: optional per-source-row scale
  void* dst;
  int R, Cc;            // CAST: R = element count, Cc = 1; DOWN / DOWN_T: R = Cout, Cc = Cin
  int op, blk0;
};
int pack_job_blocks(const PackJob& j);
int launch_pack_jobs(int prec, const PackJob* dev_jobs, int njobs, int total_blocks, hipStream_t st);
// src [R][Cc] fp32 -> dst [Cc][R] fp32
int launch_transpose_f32(const float* src, float* dst, int R, int Cc, hipStream_t st);
// downsample filter [Cout][Cin][2][2] fp32 -> [Cout][(ky*2+kx)*Cin + cin] prec-typed
int launch_pack_down(int prec, const float* src, void* dst, int Cout, int Cin, hipStream_t st);
// split mode (BTSBOT_F16X2): the same element order, f16 heads into `hi`, f16 remainders into `lo`
int launch_pack_down_split(const float* src, void* hi, void* lo, int Cout, int Cin, hipStream_t st);
// BatchNorm1d eval fold: scale = w / sqrt(rv + eps), shift = b - rm * scale
int launch_bn_fold(const float* w, const float* b, const float* rm, const float* rv, float* scale,
                   float* shift, int n, hipStream_t st);
// src fp32 [R][Cc] -> dst prec-typed [Cc][R]
int launch_transpose_cast(int prec, const float* src, const float* rowscale, void* dst, int R, int Cc,
                          hipStream_t st);
int launch_pack_down_t(int prec, const float* src, void* dst, int Cout, int Cin, hipStream_t st);
// Gd [Cout][4][Cin] (q-major patches order) accumulated into dst [Cout][Cin][4] (master layout)
int launch_unpack_down_grad(float* Gd, float* dst, int Cout, int Cin, hipStream_t st);   // leaves Gd zero
int launch_rowscale_cast(int prec, const float* in, const float* rowscale, void* out, int rows,
                         int cols, hipStream_t st);   // out[r][c] = in[r][c] * rowscale[r]
// f16 remainder image of launch_rowscale_cast(BTSBOT_F16, ...): out[r][c] = f16(v - f16(v)), v = in[r][c] * rowscale[r] (rowscale
// may be NULL: v = in[r][c]) -- the second half of a split operand (BTSBOT_F16X2)
int launch_rowscale_cast_lo(const float* in, const float* rowscale, void* out, int rows, int cols, hipStream_t st);
int launch_scale_cast(int prec, const float* in, const float* scale, void* out, long n, int C,
                      hipStream_t st);
int launch_stem_im2col(int prec, const float* img, void* patches, int B, hipStream_t st);

// ---- gemm.hip
// out = epi(X[M,K] . W[N,K]^T + bias[N]);  X, W are `prec`-typed, bias/gamma/resid fp32.
//   EPI_GELU : out (prec-typed) [M,N] = gelu(acc + bias)
//   EPI_RESID: out (fp32)       [M,N] = resid + gamma[n] * (acc + bias)   (in place allowed)
//   EPI_BIAS : out (fp32)       [M,N] = acc + bias
//   EPI_SILU : out (prec-typed) [M,N] = silu(acc + bias)     (MaxViT MBConv: BatchNorm folded into W / bias)
//   EPI_BIAS_T: out (prec-typed) [M,N] = acc + bias           (MaxViT qkv projection)
// training-only epilogues (register-staged kernel; `resid` carries a prec-typed aux pointer):
//   EPI_GELU_SAVE: aux [M,N] = acc + bias (pre-activation, written), out = gelu(aux)
//   EPI_DGELU    : out (prec-typed) = acc * gelu'(aux[m][n])            (aux read, no bias)
//   EPI_PLAIN    : out (fp32) = acc
int launch_gemm(int prec, int epi, const void* X, const void* W, const float* bias,
                const float* gamma, const float* resid, void* out, int M, int N, int K,
                hipStream_t st);

// out (fp32) [M,N] = resid + (X[m][k] * gate[m / rows_per_alert][k]) . W[n][k]^T: the squeeze-excite gate of a
// MaxViT MBConv block applied to the A operand on its way to LDS (register-staged kernel); in place allowed
int launch_gemm_gated(int prec, const void* X, const float* gate, int rows_per_alert, const void* W,
                      const float* resid, float* out, int M, int N, int K, hipStream_t st);

// ---- gemm2.hip
// pipelined LDS-DMA variant for the 16-bit modes (gemm2.hip); launch_gemm dispatches to it
bool gemm2_supported(int prec, int M, int N, int K);
int launch_gemm2(int prec, int epi, const void* X, const void* W, const float* bias,
                 const float* gamma, const float* resid, void* out, int M, int N, int K,
                 hipStream_t st);

int launch_gemm2_batched_resid(int prec, const void* X, const void* W, const float* zero_bias,
                               const float* one_gamma, const float* resid, float* out, int batch, int M,
                               int N, int K, hipStream_t st, const float* ln_w = nullptr,
                               const float* ln_b = nullptr, void* ln_out = nullptr);

// ---- gemm_x2.hip
// split-operand form (gemm_x2.hip, the MaxViT forward of an f16x2 handle): X fp32 [M][K], W the packed f16 head plane
// [N][K] followed by the remainder plane; out fp32 for every epilogue (EPI_GELU / RESID / BIAS / SILU / BIAS_T, resid may
// alias out); K % 8 == 0, N % 4 == 0
int launch_gemm_x2(int epi, const float* X, const void* W, const float* bias, const float* gamma, const float* resid,
                   float* out, int M, int N, int K, hipStream_t st);
// ... and launch_gemm_gated's form: out = resid + (X[m][k] * gate[m / rows_per_alert][k]) . W^T, the product split after
// the gate
int launch_gemm_x2_gated(const float* X, const float* gate, int rows_per_alert, const void* W, const float* resid,
                         float* out, int M, int N, int K, hipStream_t st);
// ---- split training products (BTSBOT_F16X2 handles with "train_split"; gemm_x2.hip / wgrad_x2.hip)
// launch_gemm_x2 with every epilogue, the training ones included (EPI_GELU_SAVE / EPI_DGELU / EPI_PLAIN: gemm.hip's fp32
// semantics).  xamax (optional): X's largest magnitude (split_exp) -- X enters scaled by 2^e, the epilogue undoes it;
// oamax (optional, EPI_DGELU): receives the largest magnitude of what the launch writes
int launch_gemm_x2_train(int epi, const float* X, const void* W, const float* bias, const float* gamma, const float* resid,
                         float* out, int M, int N, int K, const unsigned* xamax, unsigned* oamax, hipStream_t st);

// ---- fused_mlp.hip
// fused fc1 -> GELU -> fc2 -> layer-scale -> residual (fused_mlp.hip); 16-bit modes, C in {64,128} and nano's {80,160}
bool fused_mlp_supported(int prec, int C);
size_t fused_mlp_packed_bytes(int C);
int launch_pack_fused_mlp(int prec, int C, const float* w1, const float* w2, void* dst,
                          hipStream_t st);
// post_out != NULL: also post_out [M,C] (prec-typed) = LayerNorm_C(x_new) * pw + pb (post_mode 1, eps 1e-6) or
// x_new * pw + pb (post_mode 2) -- the next consumer's normalised input (MaxViT schedule)
int launch_fused_mlp(int prec, int C, const void* xn, const void* wpk, const float* b1,
                     const float* b2, const float* gamma, float* x, int M, hipStream_t st,
                     void* post_out = nullptr, const float* pw = nullptr, const float* pb = nullptr,
                     int post_mode = 0, const float* xres = nullptr);   // xres: residual source when it is not x itself

// ---- stage0b.hip
// stage-0 megakernel (stage0b.hip): stem + 2 blocks + downsample in one launch, 16-bit modes, C0 = 64
struct Stage0Args;
bool stage0_supported(int prec, int c0);
int launch_stage0b(int prec, const Stage0Args& a, hipStream_t st);   // stage0b.hip
size_t s0par_bytes();
int launch_pack_s0par(int prec, const float* taps, const float* dw_b, const float* ln_w, const float* ln_b,
                      const float* b1, const float* b2, const float* gamma, void* out,
                      hipStream_t st);

// ---- stage1b.hip
struct Stage1Args;
bool stage1_supported(int prec, int c1, int c2);   // stage1b.hip
int launch_stage1b(int prec, const Stage1Args& a, bool g5, hipStream_t st);   // stage1b.hip
size_t s1par_bytes();
int launch_pack_frag32(int prec, const float* src, void* dst, int cout, int cin, hipStream_t st);   // stage1b.hip
int launch_pack_s1par(int prec, const float* taps, const float* dw_b, const float* ln_w,
                      const float* ln_b, void* out, hipStream_t st);

// ---- stage2p.hip
// persistent stage 2 (+ stages[3].downsample) for C = 256 -> 512, 16-bit modes (stage2p.hip)
struct Stage2pArgs;
bool stage2p_supported(int prec, int c2, int c3, int depth);
int launch_stage2p(int prec, const Stage2pArgs& a, hipStream_t st);
// alerts resident per workgroup (4, 5 or 7) of a call of B alerts with Stage2pArgs::alerts_hint = hint (256 channels)
int stage2p_alerts_per_workgroup(int B, int hint);
// the kernel's row-tile form (stage2p.hip, ROWS): x [rows][256] fp32 += W2 gelu(W1 LN(x) + b1) + b2 in place -- the MLP half
// of a MaxViT partition-attention layer at 256 channels.  blk: ln_w / ln_b = norm2, b1 / b2 the Linear biases, gamma = ones,
// w1p / w2p = launch_pack_s2p fragments of fc1 [1024][256] / fc2 [256][1024]; dw_* unused
struct Stage2pBlk;
bool stage2p_rows_supported(int prec, int c);
int launch_stage2p_rows(int prec, float* x, long rows, const Stage2pBlk& blk, hipStream_t st);
// fp32 [rows][K] (reorder_down: a [Cout][Cin][2][2] downsample filter, K = 4 Cin) -> 16x16x32 A fragments
// [row tile][k-step][lane][8], optionally scaled per row
int launch_pack_s2p(int prec, const float* src, const float* rowscale, void* dst, int rows, int K, int reorder_down,
                    int cin, float* scale, hipStream_t st);   // scale: fp8 mode only ({S, 1/S}, device)

// ---- convnext.hip
// stem: conv 4x4 s4 (+bias) + LayerNorm over C0.  img [B,3,63,63] fp32 -> out [B,225,C0] fp32.
// (pre_out, optional: the convolution's output before the LayerNorm, [B,225,C0] fp32 -- what the training backward needs)
int launch_stem(const float* img, const float* w48xC, const float* bias, const float* lnw,
                const float* lnb, float* out, int B, int C0, hipStream_t st, float* pre_out = nullptr);

// depthwise 7x7 p3 (+bias) + LayerNorm over C.  x [B,HW*HW,C] fp32 -> xn [B,HW*HW,C] prec-typed.
// wdw is tap-major [49][C] fp32.
// dsave != NULL: also the pre-LayerNorm map d = dwconv(x) + bias, [B,HW*HW,C] fp32 (kept for the backward)
int launch_dwconv_ln(int prec, const float* x, const float* wdw, const float* bdw,
                     const float* lnw, const float* lnb, void* xn, int B, int HW, int C,
                     hipStream_t st, float* dsave = nullptr);

// downsample prologue: LayerNorm over Cin per pixel, then 2x2/s2 patch gather.
// x [B,HW,HW,Cin] fp32 -> patches [B*(HW/2)^2, 4*Cin] prec-typed, k = (ky*2+kx)*Cin + c.
int launch_ln_patch(int prec, const float* x, const float* lnw, const float* lnb, void* patches,
                    int B, int HW, int Cin, hipStream_t st);

// ---- stem16.hip
// the same on the matrix pipe for the 16-bit modes (stem16.hip): w is the fp32 filter [C0][48], converted in registers
bool stem16_supported(int prec, int C0);
int launch_stem16(int prec, const float* img, const float* w, const float* bias, const float* lnw, const float* lnb,
                  float* out, int B, int C0, hipStream_t st, float* pre_out = nullptr);

// ---- dw15.hip
// depthwise 7x7 + LayerNorm of a 15x15 map on the matrix pipe (dw15.hip): 16-bit modes, C in {64, 80}; the map enters
// the products rounded to the operand type (launch_dwconv_ln routes the inference forward there; BTSBOT_AMD_NO_DW15=1: A/B)
bool dw15_supported(int prec, int C);
int launch_dw15_ln(int prec, const float* x, const float* wdw, const float* bdw, const float* lnw, const float* lnb,
                   void* xn, int B, int C, hipStream_t st);

// ---- head.hip
struct HeadArgs {
  // image feature part
  const float* feat;  // [B, feat_dim] fp32 (final 1x1 map), or nullptr
  int feat_dim;
  const float* hn_w;  // head LayerNorm (nullptr -> none)
  const float* hn_b;
  // metadata part (BatchNorm folded to scale/shift; training: scale/shift of the batch stats)
  const float* meta;  // [B, n_meta] or nullptr
  int n_meta, f1, f2;
  const float* bn_scale;
  const float* bn_shift;
  const float* m1_wt;  // [n_meta][f1]  (K-major)
  const float* m1_b;
  const float* m2_wt;  // [f1][f2]
  const float* m2_b;
  int meta_act, meta_trailing_act;
  // combined MLP: up to 3 linear layers, act between them
  int n_layers;
  int dims[4];         // dims[0] = feat_dim + f2 (or f2 / feat_dim), ..., dims[n_layers] = 1
  const float* wt[3];  // K-major [dims[i]][dims[i+1]]
  const float* b[3];
  int comb_act;
  float* logits;
  float* scores;  // may be nullptr
  // embedding outputs (btsbot_forward_embed), each may be nullptr; row-contiguous fp32, rows b >= B are never written
  float* features;  // [B][dims[0]]: the concat row z, the input of the first fusion layer
  float* hidden;    // [B][dims[n_layers - 1]]: the input of the last layer (= features when n_layers == 1)
  int B;
  int diag;       // timing diagnostics (BTSBOT_AMD_HEAD_DIAG): 1 skip feature LN, 2 skip metadata
                  // branch, 4 skip fusion layer 0, 8 skip fusion layers 1.., 16 skip all K loops
};
int launch_head(const HeadArgs& a, hipStream_t st);

// ---- head_train.hip: the training heads' kernels (fp32), one launcher each; the schedules of head_train.hip and the op
// entry points of head_ops.hip go through these and nothing else
// pre [M][N] (may be nullptr) = bias + in [M][ldi] . wt [K][N];  outa [M][ldo] = dropout(act(pre)), mask [M][N] or nullptr
int launch_ht_lin_fwd(const float* in, int ldi, const float* wt, const float* bias, float* pre, float* outa, int ldo, int M,
                      int N, int K, int act, const uint8_t* mask, float keep_scale, hipStream_t st);
int launch_ht_act_fwd(const float* pre, float* outa, int ldo, int M, int N, int act, const uint8_t* mask, float keep_scale,
                      hipStream_t st);
// a fusion layer's forward: head_train_lin_is_wide(M, N, K, ldi) ? launch_gemm on w [N][K] into pre (which must exist) +
// launch_ht_act_fwd : launch_ht_lin_fwd on wt [K][N]
bool head_train_lin_is_wide(int M, int N, int K, int ldi);
int launch_ht_layer_fwd(const float* in, int ldi, const float* w, const float* wt, const float* bias, float* pre, float* outa,
                        int ldo, int M, int N, int K, int act, const uint8_t* mask, float keep_scale, hipStream_t st);
// dpre [M][N] = dout [M][ldd] * act'(pre) * mask * keep_scale   (in place allowed)
int launch_ht_act_bwd(const float* dout, int ldd, const float* pre, float* dpre, int M, int N, int act, const uint8_t* mask,
                      float keep_scale, hipStream_t st);
// din [M][ldi] (columns 0 .. K) = dpre [M][N] . w [N][K]
int launch_ht_lin_bwd_in(const float* dpre, const float* w, float* din, int ldi, int M, int N, int K, hipStream_t st);
// a fusion layer's input gradient, din [M][K]: head_train_lin_is_wide(M, K, N, N) ? launch_gemm on wt [K][N] : the above
int launch_ht_layer_bwd_in(const float* dpre, const float* w, const float* wt, float* din, int M, int N, int K,
                           hipStream_t st);
// dw [N][K] = dpre^T in, db [N] = colsum(dpre) (written); which kernel: 0 lin_bwd_w4, 1 lin_bwd_w<4, 64>, 2 lin_bwd_w<16, 16>
int head_train_lin_bwd_w_kind(const float* in, int ldi, const float* dw, int N, int K);
int launch_ht_lin_bwd_w(const float* dpre, const float* in, int ldi, float* dw, float* db, int M, int N, int K,
                        hipStream_t st);
// BatchNorm1d on batch statistics over x [M][n]; run_mean / run_var (nullptr: none) updated with momentum 0.1
int launch_ht_bn_fwd(const float* x, int M, int n, const float* w, const float* b, float* run_mean, float* run_var,
                     float* xhat, float* out, float* rstd, hipStream_t st);
int launch_ht_bn_bwd(const float* dy, int M, int n, const float* w, const float* xhat, const float* rstd, float* dw,
                     float* db, hipStream_t st);
// BatchNorm1d on running statistics: out = (x - rm) * rsqrt(rv + eps) * w + b; xhat and rstd [n] kept as by the above
int launch_ht_bn_eval_fwd(const float* x, int M, int n, const float* w, const float* b, const float* run_mean,
                          const float* run_var, float* xhat, float* out, float* rstd, hipStream_t st);
// the BatchNorm's input gradient dx [M][n].  eval != 0: dx = dy w rstd (running statistics are constants); else the
// batch-statistics form dx = (w rstd / M) (M dy - sum_dy - xhat sum_dyx) on the two column sums launch_ht_bn_bwd left
// (its db and dw); they are not read in the eval form
int launch_ht_bn_bwd_in(const float* dy, int M, int n, const float* w, const float* xhat, const float* rstd,
                        const float* sum_dy, const float* sum_dyx, float* dx, int eval, hipStream_t st);
// z [M][ldz] (columns 0 .. F) = feat [M][F], through the head LayerNorm where hw != nullptr
int launch_ht_feat_rows(const float* feat, int F, const float* hw, const float* hb, float* z, int ldz, int M,
                        hipStream_t st);
int launch_ht_logits(const float* in, float* logits, float* scores, int M, hipStream_t st);   // scores may be nullptr
int launch_ht_copy_cols(float* dst, int ldd, const float* src, int lds, int cols, int M, hipStream_t st);

// ---- wgrad.hip
// slice reduction of a filter-gradient GEMM (wgrad.hip), described so that two of them can share a launch
struct WgradReduceJob {
  const float* part;   // partial tiles [nsl][gy][gx][TN][TK]
  float* out;          // out[n][k] += sum over the slices
  int N, K, ldo, gx, gy, nsl, TN, TK;   // nsl == 0: nothing to reduce
};
int launch_wgrad16(int prec, const void* D, const void* A, float* out, float* colsum, int M, int N,
                   int K, int ldo, hipStream_t st, float* part = nullptr, size_t part_floats = 0,
                   WgradReduceJob* defer = nullptr);   // wgrad.hip: 16-bit modes, colsum optional
int launch_wgrad_reduce(const WgradReduceJob* jobs, int njobs, hipStream_t st);
// several filter-gradient GEMMs (N, K multiples of 128; out[n][k] += ..., colsum[n] += ... optional) as one launch + one
// slice reduction (wgrad.hip); out must be 16-byte aligned with ldo a multiple of 4
struct WgradBatchJob {
  const void* D;
  const void* A;
  float* out;
  float* colsum;
  int M, N, K, ldo;
};
int launch_wgrad16_batched(int prec, const WgradBatchJob* jobs, int njobs, float* part, size_t part_floats, int target_wg,
                           hipStream_t st);

// ---- wgrad_f32.hip
// fp32 mode: out[n][k] += sum_m D[m][n] A[m][k] and (cs != nullptr) cs[n] += sum_m D[m][n] (wgrad_f32.hip)
int launch_wgrad_cs_f32(const float* D, const float* A, float* out, float* cs, int M, int N, int K, int ldo, hipStream_t st);

// ---- wgrad_x2.hip
// out[n][k] += sum_m D[m][n] A[m][k] and (colsum != nullptr) colsum[n] += sum_m D[m][n] (fp32 sums of the unscaled D,
// fixed-order in deterministic mode) on split operands (D, A fp32 pixel-major; D scaled by 2^split_exp(damax) before the
// split, undone on the slice partials; aamax, optional: A likewise -- the stem's patches are raw pixel values).  N, K
// multiples of 16.  part / part_floats / defer as for launch_wgrad16; with part the slices never meet through atomics
// (a single slice still goes through the partial tiles).
int launch_wgrad_x2(const float* D, const float* A, float* out, float* colsum, int M, int N, int K, int ldo, const unsigned* damax,
                    const unsigned* aamax, hipStream_t st, float* part, size_t part_floats, WgradReduceJob* defer);
// out = in (fp32 copy; out may be nullptr) and amax's record (AMAX_WORDS words) takes in's largest magnitude (n a multiple
// of 4, 16-byte aligned)
int launch_copy_amax(const float* in, float* out, long n, unsigned* amax, hipStream_t st);
// f16 head / remainder planes of fp32 images: for each job, dst[0, n) = f16(src), dst[n, 2n) = f16(src - f16(src))
struct SplitJob { const float* src; void* dst; long n; };
int launch_split_jobs(const SplitJob* jobs_dev, int njobs, hipStream_t st);

// ---- det_reduce.hip: the deterministic mode's scratch and reductions (device_math.h: det_add)
struct DetOut { float* ptr; int stride; };   // column c of output o goes to ptr[c * stride]
void det_begin(float* base, size_t floats);  // the scratch of this thread's btsbot_backward() call (base == nullptr: mode off)
void det_end();
bool det_fell_short();                       // (and clears the flag) a det_alloc() since the last call found the scratch full
float* det_alloc(size_t floats);             // nullptr when the mode is off (or the scratch is exhausted: atomics then)
// outs[o].ptr[c * stride] += sum over rows r (in order) of part[r * nout * C + o * C + c]
int launch_det_reduce(const float* part, int nrows, int C, int nout, const DetOut* outs, hipStream_t st);
int launch_colsum(int prec, const void* in, float* out, int M, int N, hipStream_t st);  // out[n] += ...

// ---- ln_dw_bwd.hip
int launch_fc2_grads(float* G, float* S, const float* w2, const float* b2,
                     const float* gamma, float* dW2, float* db2, float* dgamma, int C, int H,
                     hipStream_t st);
int launch_ln_bwd(const float* d, const float* dxn, const float* g, float* dd, float* dg,
                  float* dbeta, long rows, int C, hipStream_t st, void* out16 = nullptr, int prec16 = 0,
                  int patch_hw = 0);
// (out16: also dd in the 16-bit operand type prec16 -- the operand of the GEMM that consumes it;
//  patch_hw != 0: dxn holds the gradient of a 2x2 / stride-2 downsample's patch matrix [B (hw/2)^2][4 C] for input
//  maps of side patch_hw, gathered per input pixel -- the rows count input pixels)
int launch_dw_plain(const float* x, const float* w, int flip, const float* bias,
                    const float* addend, float* out, int B, int HW, int C, hipStream_t st,
                    void* out16 = nullptr, int prec16 = 0);
// (out16: also the result in the 16-bit operand type prec16 -- the next block's GEMM operand)
int launch_dw_wgrad(const float* x, const float* dd, float* dw, float* dbias, float* partials,
                    int B, int HW, int C, hipStream_t st);   // partials: >= 256 * 50 * C floats
// 1x1 maps: the same three steps (plus the filter gradient's column sum) as one per-(alert, channel) kernel, ln_dw_bwd.hip
int launch_ln_dw1_bwd(const float* d, const float* dxn, const float* g, const float* xin, const float* w, float* dy,
                      void* out16, int prec16, float* dg, float* dbeta, float* dw, float* dbias, long rows, int C,
                      hipStream_t st);

// ---- dwln_bwd.hip
// dwln_bwd.hip: the three launches above (LayerNorm backward, depthwise filter gradient, depthwise input gradient)
// as one kernel, dd never leaving LDS; dy is updated in place (dy += conv(dd, flipped taps))
bool dwln_bwd_supported(int HW, int C);
int dwln_bwd_rows(int HW, int C, int B);   // partial rows (52 * C floats each) to keep room for
int dwln_bwd_grid(int HW, int C, int B);   // ... and those launch_dwln_bwd writes: the rows of the column sum behind it
// (d == nullptr: the depthwise output is recomputed from x_in, the taps and the depthwise bias dwb)
int launch_dwln_bwd(const float* d, const float* dxn, const float* g, const float* xin, const float* w, float* dy,
                    void* out16, int prec16, float* partials, int B, int HW, int C, hipStream_t st, int nplanes = 1,
                    size_t pstride = 0);
// 3x3 maps of 256 channels: their own kernel (d recomputed from x_in, compact partial rows) and its row reduction
bool dw3_bwd_active(int HW, int C);
int dw3_rows(int B);
int launch_dw3ln_bwd(const float* dwb, const float* dxn, const float* g, const float* xin, const float* w, float* dy,
                     void* out16, int prec16, float* partials, int B, hipStream_t st, int nplanes = 1, size_t pstride = 0);
int launch_dw3_rows(const float* partials, float* out, int nrows, hipStream_t st);

// ---- stem_dgrad.hip
// dimg [B][3][63][63] = the input gradient of the patch stem from dxn [B*225][C0] (fp32, behind the stem convolution) and
// the filter w [C0][48] (fp32, state-dict layout); every element written once, rows / columns 60..62 as +0.0f.  C0 64 or 80
int stem_dgrad_grid(int B);
int launch_stem_dgrad(const float* dxn, const float* w, float* dimg, int B, int C0, hipStream_t st);

// ---- mlp_bwd.hip
// backward of a block's MLP as one kernel (mlp_bwd.hip): 16-bit modes, C in {64, 128}
bool mlp_bwd_supported(int prec, int C);
int mlp_bwd_slices(int C, int R);
size_t mlp_bwd_part_floats(int C, int R);   // scratch for the partial filter-gradient tiles of one block
// dxn leaves as mlp_bwd_planes(C) addend planes, R * C floats apart (C = 128: one per hidden slice; the reader adds them:
// launch_dwln_bwd's nplanes)
int mlp_bwd_planes(int C);
int launch_mlp_bwd(int prec, int C, const void* xn, const void* dy, const void* w1, const void* w2g, const float* b1,
                   float* dxn, float* part, float* Gacc, float* Ssum, float* dW1, float* db1, int R, hipStream_t st,
                   WgradReduceJob* jobs);

// ---- s2mlp_bwd.hip
// the input-gradient half of a 256-channel block's MLP backward as one launch (s2mlp_bwd.hip): da = ((gamma W2)^T dy) *
// gelu'(a) [R][1024] (operand type) and dxn = W1^T da [R][256] (fp32); w2tp / w1tp = launch_pack_frag16 of the 16-bit
// dgrad transposes (diag(gamma) W2)^T [1024][256] and W1^T [256][1024]
bool s2mlp_bwd_supported(int prec, int C);
int s2mlp_bwd_rows();   // pixel rows per workgroup (<= 48): da is stored in whole workgroups of them
int launch_pack_frag16(const void* src, void* dst, int rows, int K, hipStream_t st);
int launch_s2mlp_bwd(int prec, const void* dy, const void* a, const void* w2tp, const void* w1tp, void* da, float* dxn, int R,
                     hipStream_t st);

// ---- train.hip
// fills / copies of the training step as plain kernels (train.hip says why not hipMemsetAsync / hipMemcpyAsync)
int launch_fill0(float* p, size_t n, hipStream_t st);
int launch_copy_f32(float* dst, const float* src, size_t n, hipStream_t st);
