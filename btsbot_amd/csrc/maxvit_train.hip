// Training of the MaxViT image branch (timm maxvit_tiny_rw_224 as /root/reference/btsbot/architectures.py:25-101
// builds it; the reference fine-tunes it end to end: train.py:218-236, 510-527): the training-mode forward --
// BatchNorm2d on BATCH statistics, running statistics updated in the master arena -- and the backward of every
// layer: stem convolutions, MBConv (pre-norm, 1x1 expand, depthwise 3x3, squeeze-excite, 1x1 project, pooled /
// projected shortcut), window and grid attention with the relative-position bias, the MLPs, the final LayerNorm2d
// and the global pool.  The algorithm is restated (with autograd) in oracle/maxvit_oracle.py, branch_training=True.
//
// An fp32 engine of its own, whatever the handle's operand mode: activations are fp32 NHWC rows [B*H*H][C]; every
// 1x1 convolution / Linear runs on the exact-fp32 MFMA GEMM (gemm.hip), its input gradient on the same GEMM against
// the transposed filter, its filter gradient on wgrad_f32.hip's split-K GEMM; what has no GEMM shape (BatchNorm
// statistics, depthwise 3x3, squeeze-excite, attention inside a 49-token partition) is a small kernel of
// maxvit_train_kernels.hip.  It is correctness-first -- one launch per layer, every intermediate through HBM (~110 MB
// of cache per alert) -- and says so in DESIGN.md: configs[2], the training benchmark, is ConvNeXt.
//
// This file is the engine alone: the cache (MvtCache / carve), the state both passes share (MvtPass), the 16-bit
// operands of the GEMMs (MvtOperands), maxvit_train_forward and maxvit_train_backward.  The op-level entry points of
// the kernels (btsbot_op_mvt_*) are in maxvit_train_ops.hip.
#include <string.h>

#include <vector>

#include "ctx.h"
#include "maxvit.h"
#include "maxvit_tables.h"

namespace {

// ---- the engine's cache: every activation the backward needs, carved from one allocation -------------------------
constexpr size_t MVT_WPART_FLOATS = (size_t)16 << 20;
constexpr int MVT_SUM_SLOTS = 96;   // BatchNorm reduction slots per pass: 2 per layer forward (34 layers), 1 backward

struct AttnAct {
  float *n1, *qkv, *o, *y1, *n2, *f1, *gl, *y2;
};
struct BlkAct {
  float *xin, *pool_in, *a0, *c1, *a1, *d2, *a2, *sepool, *rpre, *r, *g, *y;
  float *st_pre, *st1, *st2;   // BatchNorm batch statistics: mean [C] | rstd [C]
  AttnAct at[2];
};
struct MvtCache {
  float *col1, *y1, *a1s, *st_stem, *x0, *w1p, *w2p;
  std::vector<BlkAct> blk;
  float *xfin;                     // final LayerNorm input = last block's output
  // backward scratch
  float *dA, *dB, *dC, *wt, *sums, *dsmall, *dbias, *g9, *gconv, *xn_final;
  // 16-bit operand modes: the GEMMs' operands are cast per call into these (fp32 everywhere else)
  void *x16, *d16, *w16;
  // ... except the filters, cast once per forward as one pass over the whole parameter mirror (filter W at wall16 + (W - mirror)),
  // and the GEMM inputs of the forward, whose 16-bit copies stay (xkeep, handed out in call order) for the filter
  // gradients of the backward: 230 of the step's 612 cast launches gone
  void *wall16, *xkeep;
  size_t xkeep_floats;
  float* wpart;                    // partial tiles of the 16-bit filter-gradient GEMM (two-pass reduction)
  size_t total;
};

MvtCache carve(const MaxVit* mv, unsigned char* base, int B, int64_t nparams = 0) {
  MvtCache k;
  size_t cur = 0;
  auto take = [&](size_t floats) {
    float* p = base ? reinterpret_cast<float*>(base + cur) : nullptr;
    cur += align256(floats * 4);
    return p;
  };
  const size_t n = (size_t)B, M0 = n * 12544;
  k.col1 = take(M0 * 32);
  k.y1 = take(M0 * 32);
  k.a1s = take(M0 * 32);
  k.st_stem = take(64);
  k.x0 = take(M0 * 64);
  k.w1p = take(32 * 32);
  k.w2p = take(64 * 288);
  float* x = k.x0;
  for (const MvBlock& b : mv->blocks) {
    BlkAct a;
    const size_t Min = n * b.hin * b.hin, Mo = n * b.hout * b.hout;
    a.xin = x;
    a.pool_in = b.stride == 2 ? take(Mo * b.cin) : nullptr;
    a.a0 = take(Min * b.cin);
    a.c1 = take(Min * b.mid);
    a.a1 = take(Min * b.mid);
    a.d2 = take(Mo * b.mid);
    a.a2 = take(Mo * b.mid);
    a.sepool = take(n * b.mid);
    a.rpre = take(n * b.rd);
    a.r = take(n * b.rd);
    a.g = take(n * b.mid);
    a.y = take(Mo * b.c);
    a.st_pre = take(2 * b.cin);
    a.st1 = take(2 * b.mid);
    a.st2 = take(2 * b.mid);
    float* yin = a.y;
    for (int g = 0; g < 2; ++g) {
      AttnAct& t = a.at[g];
      t.n1 = take(Mo * b.c);
      t.qkv = take(Mo * 3 * b.c);
      t.o = take(Mo * b.c);
      t.y1 = take(Mo * b.c);
      t.n2 = take(Mo * b.c);
      t.f1 = take(Mo * 4 * b.c);
      t.gl = take(Mo * 4 * b.c);
      t.y2 = take(Mo * b.c);
      yin = t.y2;
    }
    x = yin;
    k.blk.push_back(a);
  }
  k.xfin = x;
  k.dA = take(M0 * 256);       // the largest gradient maps: [12544][256] per alert (block 0's expanded map)
  k.dB = take(M0 * 256);
  k.dC = take(M0 * 288);       // stem: gradient of the im2col matrix [12544][288]; also forward's im2col scratch
  k.wt = take(2048 * 512);
  k.sums = take((size_t)MVT_SUM_SLOTS * 4096);   // per-BatchNorm slots of a zeroed arena (sum | sum of squares, <= 2048 channels)
  k.dsmall = take(n * 2048 * 4);
  k.dbias = take(32 * 2401);   // gradient of the bias [heads <= 16][49][49] | its forward image
  k.g9 = take(10 * 2048);
  k.gconv = take(64 * 288);
  k.xn_final = take(n * 49 * 512);
  k.x16 = take(M0 * 288 / 2);
  k.d16 = take(M0 * 288 / 2);
  k.w16 = take(2048 * 512 / 2);
  k.wall16 = take((size_t)nparams / 2 + 64);
  {
    // 16-bit copies of every forward GEMM input, in call order (two per float)
    size_t e = M0 * 32 + M0 * 288;
    for (const MvBlock& b : mv->blocks) {
      const size_t Min = n * b.hin * b.hin, Mo = n * b.hout * b.hout;
      e += (b.stride == 2 && b.sc_w >= 0 ? Mo * b.cin + 128 : 0) + Min * b.cin + Mo * b.mid + 2 * (3 * Mo * b.c + Mo * 4 * b.c) + 12 * 128;
    }
    k.xkeep_floats = e / 2 + 256;
    k.xkeep = take(k.xkeep_floats);
  }
  k.wpart = take(MVT_WPART_FLOATS);
  k.total = cur;
  return k;
}

// ---- the 16-bit operands of the GEMMs (16-bit operand modes): every cast the engine makes is one of these methods
struct MvtOperands {
  int prec;
  hipStream_t st;
  const float* mirror;   // the fp32 parameters [nmirror]; wall16 holds them in the operand type at the same offsets
  int64_t nmirror;
  void *wall16, *w16, *x16, *d16, *xkeep;
  size_t xkeep_bytes, xcur = 0;                             // xkeep's size, and what the forward has handed out of it
  const float *dA, *dB, *dC;                                // scratch maps, rewritten before the backward: never kept
  std::vector<std::pair<const float*, void*>>& kept_list;   // MaxVit::xkept: it outlives the forward
  const float* d16_src = nullptr;                           // the map [d16_n] d16 holds since the last filter gradient
  int64_t d16_n = 0;

  MvtOperands(const btsbot_ctx* h, const MvtCache& k, hipStream_t st)
      : prec(h->cfg.precision), st(st), mirror(h->mirror), nmirror(h->total_floats), wall16(k.wall16), w16(k.w16), x16(k.x16),
        d16(k.d16), xkeep(k.xkeep), xkeep_bytes(k.xkeep_floats * 4), dA(k.dA), dB(k.dB), dC(k.dC), kept_list(h->mv->xkept) {}

  int cast(const float* src, void* dst, int64_t n, const void** out) {
    *out = dst;
    return launch_cast(prec, src, dst, n, st);
  }
  // the forward starts: no input is kept yet; every filter of the parameter mirror in the operand type, one launch
  int start_forward(bool lowp) {
    kept_list.clear();
    xcur = 0;
    return lowp ? launch_cast(prec, mirror, wall16, nmirror, st) : BTSBOT_OK;
  }
  // a filter [n]: inside the mirror it is wall16 + 2 (W - mirror), no launch; outside (the stem's packed filters) it is
  // cast into w16  (filter alignment behind wall16: the fix belongs here)
  int filter(const float* W, int64_t n, const void** out) {
    if (!(W >= mirror && W + n <= mirror + nmirror)) return cast(W, w16, n, out);
    *out = reinterpret_cast<const unsigned char*>(wall16) + (size_t)(W - mirror) * 2;
    return BTSBOT_OK;
  }
  // the transposed filter of an input gradient: W [R][Cc] -> w16 [Cc][R]
  int filter_t(const float* W, int R, int Cc, const void** out) {
    *out = w16;
    return launch_transpose_cast(prec, W, nullptr, w16, R, Cc, st);
  }
  // a GEMM input [n] of the forward: a scratch map is cast into x16 per call; every other one into the next
  // 256-byte-aligned slot of xkeep, where it stays for the filter gradient of the backward
  int input(const float* X, int64_t n, const void** out) {
    if (X == dA || X == dB || X == dC) return cast(X, x16, n, out);
    const size_t bytes = align256((size_t)n * 2);
    if (xcur + bytes > xkeep_bytes) {
      btsbot_set_error("maxvit_train_forward: the kept-operand arena is too small");
      return BTSBOT_ERR_STATE;
    }
    void* dst = reinterpret_cast<unsigned char*>(xkeep) + xcur;
    xcur += bytes;
    TRY(cast(X, dst, n, out));
    kept_list.push_back({X, dst});
    return BTSBOT_OK;
  }
  // the forward's copy of X, or nullptr.  A buffer is cast where it is written last: a map the forward reused appears
  // once per use, and the LAST entry is the one the backward reads
  const void* kept(const float* X) const {
    const void* x = nullptr;
    for (const auto& e : kept_list)
      if (e.first == X) x = e.second;
    return x;
  }
  // a gradient map dY [n] in d16.  A filter gradient casts it and remembers that; the input gradient of the same layer,
  // directly behind it on the same map and size, finds it there.  Every other call casts, and forgets.
  int grad(const float* dY, int64_t n, bool filter_grad, const void** out) {
    const bool there = !filter_grad && d16_src == dY && d16_n == n;
    d16_src = filter_grad ? dY : nullptr;
    d16_n = n;
    *out = d16;
    return there ? BTSBOT_OK : launch_cast(prec, dY, d16, n, st);
  }
  void forget_grad() { d16_src = nullptr; }   // (a filter gradient that ran in fp32 left d16 alone)
};

// ---- what both passes start from: the carved cache, the constants, the precision, the BatchNorm reduction slots
struct MvtPass {
  btsbot_ctx* h;
  MaxVit* mv;
  const float* m;   // the parameter mirror
  MvtCache k;
  hipStream_t st;
  const float *zero, *one;
  // 16-bit operand modes: the 1x1 convolutions / Linear layers run the LDS-DMA GEMMs on operands cast per call (fp32
  // accumulation, fp32 results; the split mode keeps cfg.precision = fp32 and with it the exact GEMMs)
  int prec;
  bool lowp;
  MvtOperands ops;
  int next_slot = 0;     // of k.sums

  MvtPass(btsbot_ctx* h, int B, hipStream_t st)
      : h(h), mv(h->mv), m(h->mirror), k(carve(h->mv, h->bbcache, B, h->total_floats)), st(st),
        zero(reinterpret_cast<float*>(h->extra + h->mv->p_zero)), one(reinterpret_cast<float*>(h->extra + h->mv->p_one)),
        prec(h->cfg.precision), lowp(prec == BTSBOT_BF16 || prec == BTSBOT_F16), ops(h, k, st) {}

  // (the BatchNorm reductions add into slots of an arena zeroed ONCE per pass instead of behind a memset of their own:
  //  141 fills per step were 0.66 ms)
  int start() {
    HIP_TRY(hipMemsetAsync(k.sums, 0, (size_t)MVT_SUM_SLOTS * 4096 * 4, st));
    return BTSBOT_OK;
  }
  int take_sums(int slots, float** out) {
    if (next_slot + slots > MVT_SUM_SLOTS) {
      btsbot_set_error("maxvit_train: out of BatchNorm reduction slots");
      return BTSBOT_ERR_STATE;
    }
    *out = k.sums + (size_t)next_slot * 4096;
    next_slot += slots;
    return BTSBOT_OK;
  }
  // BatchNorm2d, training mode: batch statistics of x [M][C] into stat (mean | rstd), running statistics updated in the
  // master arena, y = act(...)
  int bn_train(const float* x, const BnPk& bn, float* stat, float* y, long M, int C, int act, float* master) {
    float* sums;
    TRY(take_sums(2, &sums));
    return launch_bn_train(x, m + bn.w, m + bn.b, stat, sums, sums + 4096, master ? master + bn.rm : nullptr,
                           master ? master + bn.rv : nullptr, y, M, C, act, st);
  }
  // ... and its backward: dy = gradient w.r.t. the layer's output (behind the activation), dx (+)= gradient w.r.t. x
  int bn_train_bwd(const float* x, const float* dy, const BnPk& bn, const float* stat, float* dx, float* grads, long M, int C,
                   int act, int accumulate) {
    float* sums;
    TRY(take_sums(1, &sums));
    return launch_bn_train_bwd(x, dy, stat, m + bn.w, m + bn.b, sums, dx, grads + bn.w, grads + bn.b, M, C, act, accumulate, st);
  }
  // out [M][N] = X [M][K] . W [N][K]^T + bias (EPI_BIAS), or resid + that (EPI_RESID)
  // (16-bit modes: the input is cast before the filter)
  int gemm(int epi, const float* X, const float* W, const float* bias, const float* resid, float* out, long M, int N, int K) {
    const void *x = X, *w = W;
    if (lowp) {
      TRY(ops.input(X, (int64_t)M * K, &x));
      TRY(ops.filter(W, (int64_t)N * K, &w));
    }
    return launch_gemm(lowp ? prec : BTSBOT_F32, epi, x, w, bias ? bias : zero, epi == EPI_RESID ? one : nullptr, resid, out, (int)M,
                       N, K, st);
  }
  // dX [M][K] = dY [M][N] . W [N][K]  (the GEMM against the transposed filter)
  int dgrad(const float* dY, const float* W, float* dX, long M, int N, int K) {
    const void *d = dY, *w = k.wt;
    if (lowp) {
      TRY(ops.grad(dY, (int64_t)M * N, false, &d));
      TRY(ops.filter_t(W, N, K, &w));
    } else {
      TRY(launch_transpose_f32(W, k.wt, N, K, st));
    }
    return launch_gemm(lowp ? prec : BTSBOT_F32, EPI_BIAS, d, w, zero, nullptr, nullptr, dX, (int)M, K, N, st);
  }
  // dW [N][K] += dY^T X, db [N] += column sums of dY
  int wgrad(const float* dY, const float* X, float* dW, float* db, long M, int N, int K) {
    if (!(lowp && N % 8 == 0 && K % 8 == 0)) {
      ops.forget_grad();
      return launch_wgrad_cs_f32(dY, X, dW, db, (int)M, N, K, K, st);
    }
    const void* d;
    TRY(ops.grad(dY, (int64_t)M * N, true, &d));
    const void* x = ops.kept(X);
    if (x == nullptr) TRY(ops.cast(X, ops.x16, (int64_t)M * K, &x));
    return launch_wgrad16(prec, d, x, dW, db, (int)M, N, K, K, st, k.wpart, MVT_WPART_FLOATS);
  }
};

}  // namespace

size_t maxvit_train_cache_bytes(const btsbot_ctx* h, int B) { return carve(h->mv, nullptr, B, h->total_floats).total; }

int maxvit_train_forward(btsbot_ctx* h, const float* img, int B, float* master, hipStream_t st, float** feat_out) {
  MvtPass p(h, B, st);
  TRY(p.start());
  TRY(p.ops.start_forward(p.lowp));
  const MaxVit* mv = p.mv;
  const float* m = p.m;
  const MvtCache& k = p.k;
  const long M0 = (long)B * 12544;
  // ---- stem: resize + conv 3x3 s2 (im2col GEMM) -> BN + SiLU -> conv 3x3 s1
  TRY(launch_mv_pack_stem1(BTSBOT_F32, m + mv->stem1_w, p.one, k.w1p, st));
  TRY(launch_mv_pack_conv3(BTSBOT_F32, m + mv->stem2_w, k.w2p, 64, 32, st));
  TRY(launch_mv_resize_im2col(BTSBOT_F32, img, k.col1, B, st));
  TRY(p.gemm(EPI_BIAS, k.col1, k.w1p, nullptr, nullptr, k.y1, M0, 32, 32));
  TRY(p.bn_train(k.y1, mv->stem_bn, k.st_stem, k.a1s, M0, 32, 1, master));
  TRY(launch_mv_im2col3(BTSBOT_F32, k.a1s, k.dC, B, 112, 32, st));
  TRY(p.gemm(EPI_BIAS, k.dC, k.w2p, nullptr, nullptr, k.x0, M0, 64, 288));
  if (h->debug && h->taps[0]) HIP_TRY(hipMemcpyAsync(h->taps[0], k.x0, (size_t)M0 * 64 * 4, hipMemcpyDeviceToDevice, st));
  int stage = 0, jblk = 0;
  constexpr int DEPTHS[4] = {2, 2, 5, 2};
  for (size_t bi = 0; bi < mv->blocks.size(); ++bi) {
    const MvBlock& b = mv->blocks[bi];
    const BlkAct& a = k.blk[bi];
    const long Min = (long)B * b.hin * b.hin, Mo = (long)B * b.hout * b.hout;
    const int hw2 = b.hout * b.hout;
    // shortcut: x | avgpool2(x) | avgpool2(x) Wsc^T -- goes straight into y, the projection adds to it
    const float* sc = a.xin;
    if (b.stride == 2) {
      TRY(launch_mv_avgpool2(BTSBOT_F32, a.xin, a.pool_in, 0, B, b.hin, b.cin, st));
      sc = a.pool_in;
      if (b.sc_w >= 0) {
        TRY(p.gemm(EPI_BIAS, a.pool_in, m + b.sc_w, nullptr, nullptr, a.y, Mo, b.c, b.cin));
        sc = a.y;
      }
    }
    TRY(p.bn_train(a.xin, b.pre, a.st_pre, a.a0, Min, b.cin, 0, master));
    TRY(p.gemm(EPI_BIAS, a.a0, m + b.c1_w, m + b.c1_b, nullptr, a.c1, Min, b.mid, b.cin));
    TRY(p.bn_train(a.c1, b.n1, a.st1, a.a1, Min, b.mid, 1, master));
    TRY(launch_mv_pack_dw(m + b.c2_w, p.one, k.g9, b.mid, st));
    TRY(launch_dw3_fwd(a.a1, k.g9, m + b.c2_b, a.d2, B, b.hin, b.mid, b.stride, st));
    TRY(p.bn_train(a.d2, b.n2, a.st2, a.a2, Mo, b.mid, 1, master));
    // squeeze-excite
    TRY(launch_se_fwd(a.a2, m + b.se1_w, m + b.se1_b, m + b.se2_w, m + b.se2_b, a.sepool, a.rpre, a.r, a.g, k.dA, B, hw2, b.mid,
                       b.rd, st));
    TRY(p.gemm(EPI_RESID, k.dA, m + b.c3_w, nullptr, sc, a.y, Mo, b.c, b.mid));
    const float* yin = a.y;
    for (int g = 0; g < 2; ++g) {
      const AttnPk& q = b.attn[g];
      const AttnAct& t = a.at[g];
      const int c = b.c;
      TRY(launch_mv_ln(BTSBOT_F32, yin, m + q.n1w, m + q.n1b, t.n1, Mo, c, st));
      TRY(p.gemm(EPI_BIAS, t.n1, m + q.qkv_w, m + q.qkv_b, nullptr, t.qkv, Mo, 3 * c, c));
      TRY(launch_mv_pack_relbias(m + q.rel, k.dbias, c / 32, st));
      TRY(launch_mv_attn(BTSBOT_F32, t.qkv, k.dbias, t.o, B, b.hout, c, g, st));
      TRY(p.gemm(EPI_RESID, t.o, m + q.proj_w, m + q.proj_b, yin, t.y1, Mo, c, c));
      TRY(launch_mv_ln(BTSBOT_F32, t.y1, m + q.n2w, m + q.n2b, t.n2, Mo, c, st));
      TRY(p.gemm(EPI_BIAS, t.n2, m + q.fc1_w, m + q.fc1_b, nullptr, t.f1, Mo, 4 * c, c));
      TRY(launch_gelu_fwd(t.f1, t.gl, Mo * c, st));
      TRY(p.gemm(EPI_RESID, t.gl, m + q.fc2_w, m + q.fc2_b, t.y1, t.y2, Mo, c, 4 * c));
      yin = t.y2;
    }
    ++jblk;
    if (jblk == DEPTHS[stage]) {
      if (h->debug && h->taps[stage + 1])
        HIP_TRY(hipMemcpyAsync(h->taps[stage + 1], yin, (size_t)Mo * b.c * 4, hipMemcpyDeviceToDevice, st));
      ++stage;
      jblk = 0;
    }
  }
  float* feat = k.dsmall;   // [B][512] (copied out by the caller before the backward reuses the scratch)
  TRY(launch_mv_final(k.xfin, m + mv->norm_w, m + mv->norm_b, feat, B, 49, 512, st));
  *feat_out = feat;
  return BTSBOT_OK;
}

int maxvit_train_backward(btsbot_ctx* h, const float* img, const float* dfeat, float* grads, int B, hipStream_t st) {
  MvtPass p(h, B, st);
  TRY(p.start());
  const MaxVit* mv = p.mv;
  const float* m = p.m;
  const MvtCache& k = p.k;
  // ---- final LayerNorm2d + global average pool: d(xn)[b][p][c] = dfeat[b][c] / 49
  float* dy = k.dA;         // gradient w.r.t. the current map [rows][C]
  float* dt = k.dB;         // second map
  {
    TRY(launch_bcast_set(k.xn_final, dfeat, B, 49, 512, 1.0f / 49.0f, st));
    TRY(launch_ln_bwd(k.xfin, k.xn_final, m + mv->norm_w, dy, grads + mv->norm_w, grads + mv->norm_b, (long)B * 49, 512, st));
  }
  for (int bi = (int)mv->blocks.size() - 1; bi >= 0; --bi) {
    const MvBlock& b = mv->blocks[bi];
    const BlkAct& a = k.blk[bi];
    const long Min = (long)B * b.hin * b.hin, Mo = (long)B * b.hout * b.hout;
    const int hw2 = b.hout * b.hout, c = b.c;
    // ---- the two partition-attention layers, grid first (it ran last); dy = d(loss)/d(y2)
    for (int g = 1; g >= 0; --g) {
      const AttnPk& q = b.attn[g];
      const AttnAct& t = a.at[g];
      const float* yin = g == 0 ? a.y : a.at[0].y2;
      // y2 = y1 + gl W2^T + b2
      TRY(p.wgrad(dy, t.gl, grads + q.fc2_w, grads + q.fc2_b, Mo, c, 4 * c));
      TRY(p.dgrad(dy, m + q.fc2_w, dt, Mo, c, 4 * c));                       // d(gl) [Mo][4c]
      TRY(launch_gelu_bwd(t.f1, dt, Mo * c, st));
      TRY(p.wgrad(dt, t.n2, grads + q.fc1_w, grads + q.fc1_b, Mo, 4 * c, c));
      TRY(p.dgrad(dt, m + q.fc1_w, k.dC, Mo, 4 * c, c));                     // d(n2) [Mo][c]
      TRY(launch_ln_bwd(t.y1, k.dC, m + q.n2w, dt, grads + q.n2w, grads + q.n2b, Mo, c, st));
      TRY(launch_add(dy, dt, Mo * c / 4, st));   // dy = d(y1)
      // y1 = yin + o Wp^T + bp
      TRY(p.wgrad(dy, t.o, grads + q.proj_w, grads + q.proj_b, Mo, c, c));
      TRY(p.dgrad(dy, m + q.proj_w, dt, Mo, c, c));                          // d(o) [Mo][c]
      TRY(launch_attn_bwd(t.qkv, m + q.rel, dt, k.dC, k.dbias, grads + q.rel, B, b.hout, c, g, st));   // d(qkv) [Mo][3c]
      TRY(p.wgrad(k.dC, t.n1, grads + q.qkv_w, grads + q.qkv_b, Mo, 3 * c, c));
      TRY(p.dgrad(k.dC, m + q.qkv_w, dt, Mo, 3 * c, c));                     // d(n1) [Mo][c]
      TRY(launch_ln_bwd(yin, dt, m + q.n1w, k.dC, grads + q.n1w, grads + q.n1b, Mo, c, st));
      TRY(launch_add(dy, k.dC, Mo * c / 4, st));   // dy = d(yin)
    }
    // ---- MBConv: y = sc + (a2 * g) W3^T;  dy = d(loss)/d(y) [Mo][c]
    float* dx = dt;           // gradient w.r.t. the block's input [Min][cin], accumulated from three paths
    // a3 = a2 * g (recomputed), d(a3) = dy W3
    TRY(launch_gate_mul(a.a2, a.g, k.dC, B, hw2, b.mid, st));
    TRY(p.wgrad(dy, k.dC, grads + b.c3_w, nullptr, Mo, c, b.mid));
    TRY(p.dgrad(dy, m + b.c3_w, k.dC, Mo, c, b.mid));                        // d(a3) [Mo][mid]
    // squeeze-excite: dg[b][c] = sum_p d(a3) a2; d(a2) = d(a3) g (+ the pooled path below)
    float* dgate = k.dsmall;                    // [B][mid]
    float* dr = k.dsmall + (size_t)B * 2048;    // [B][rd] and scratch
    float* dpool = k.dsmall + (size_t)B * 2048 * 2;
    float* dgpre = k.dsmall + (size_t)B * 2048 * 3;
    TRY(launch_se_bwd(k.dC, a.a2, a.sepool, a.rpre, a.r, a.g, m + b.se1_w, m + b.se2_w, grads + b.se1_w, grads + b.se1_b,
                       grads + b.se2_w, grads + b.se2_b, dgate, dr, dpool, dgpre, B, hw2, b.mid, b.rd, st));
    // BN2 + SiLU: d(d2) in place of d(a2)
    TRY(p.bn_train_bwd(a.d2, k.dC, b.n2, a.st2, k.dC, grads, Mo, b.mid, 1, 0));
    // depthwise 3x3: filter / bias gradients (tap-major, then into the master layout), input gradient d(a1) [Min][mid]
    TRY(launch_dw3_bwd_w(a.a1, k.dC, k.g9, grads + b.c2_w, grads + b.c2_b, B, b.hin, b.mid, b.stride, st));
    TRY(launch_mv_pack_dw(m + b.c2_w, p.one, k.g9, b.mid, st));
    TRY(launch_dw3_bwd_in(k.dC, k.g9, dx, B, b.hin, b.mid, b.stride, st));
    // BN1 + SiLU: d(c1) in place; conv1 1x1
    TRY(p.bn_train_bwd(a.c1, dx, b.n1, a.st1, dx, grads, Min, b.mid, 1, 0));
    TRY(p.wgrad(dx, a.a0, grads + b.c1_w, grads + b.c1_b, Min, b.mid, b.cin));
    TRY(p.dgrad(dx, m + b.c1_w, k.dC, Min, b.mid, b.cin));                   // d(a0) [Min][cin]
    // pre-norm BatchNorm (no activation): d(xin) = its input gradient ...
    TRY(p.bn_train_bwd(a.xin, k.dC, b.pre, a.st_pre, dx, grads, Min, b.cin, 0, 0));
    // ... plus the shortcut's: dy through identity | avgpool2 | avgpool2 . Wsc
    if (b.stride == 1) {
      TRY(launch_add(dx, dy, Min * b.cin / 4, st));
    } else if (b.sc_w >= 0) {
      TRY(p.wgrad(dy, a.pool_in, grads + b.sc_w, nullptr, Mo, c, b.cin));
      TRY(p.dgrad(dy, m + b.sc_w, k.dC, Mo, c, b.cin));
      TRY(launch_avgpool2_bwd(k.dC, dx, B, b.hin, b.cin, 1, st));
    } else {
      TRY(launch_avgpool2_bwd(dy, dx, B, b.hin, b.cin, 1, st));
    }
    float* tswap = dy;       // dx becomes the next (earlier) block's dy
    dy = dx;
    dt = tswap;
  }
  // ---- stem: x0 = im2col3(a1s) W2^T;  a1s = silu(BN(y1));  y1 = col1 W1^T
  {
    const long M0 = (long)B * 12544;
    TRY(launch_mv_im2col3(BTSBOT_F32, k.a1s, k.dC, B, 112, 32, st));
    HIP_TRY(hipMemsetAsync(k.gconv, 0, (size_t)64 * 288 * 4, st));
    TRY(p.wgrad(dy, k.dC, k.gconv, nullptr, M0, 64, 288));
    TRY(launch_unpack_conv3_grad(k.gconv, grads + mv->stem2_w, 64, 32, 288, st));
    TRY(p.dgrad(dy, k.w2p, k.dC, M0, 64, 288));                              // d(col2) [M0][288]
    TRY(launch_col2im3(k.dC, dt, B, 112, 32, st));
    TRY(p.bn_train_bwd(k.y1, dt, mv->stem_bn, k.st_stem, dt, grads, M0, 32, 1, 0));
    HIP_TRY(hipMemsetAsync(k.gconv, 0, (size_t)32 * 32 * 4, st));
    TRY(p.wgrad(dt, k.col1, k.gconv, nullptr, M0, 32, 32));
    TRY(launch_unpack_conv3_grad(k.gconv, grads + mv->stem1_w, 32, 3, 32, st));
  }
  for (int i = 0; i < h->n_buckets; ++i) HIP_TRY(hipEventRecord(h->bucket_ev[i], st));
  return BTSBOT_OK;
}
