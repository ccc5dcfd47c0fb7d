// Stage-0 megakernel (gfx950), one launch for
//
//   stem (conv 4x4 s4 + LN)  ->  2 x [ dwconv 7x7 + LN -> fc1 -> GELU -> fc2 -> layer-scale -> +x ]
//                            ->  downsample (LN + conv 2x2 s2)  ->  [49][128] f32
//
// (timm ConvNeXt stem / stages[0] / stages[1].downsample) -- cut so that TWO workgroups share a CU:
// a single 512-thread workgroup per CU (the first layout of this kernel, rounds 1-2, no longer in the tree) runs its
// phases in lockstep (depthwise = VALU + LDS, MLP = MFMA + VALU, parameter fetches = latency) and nothing overlaps; two independent
// 256-thread workgroups drift apart and fill each other's stalls, at the same 2 waves per SIMD
// that the f32 VALU needs for its full rate (tools/unit/valu_rate.hip).
//
// What had to shrink to fit 80 KB of LDS and 4 waves per workgroup:
//   * ONE image region.  The depthwise phase reads it as the planar 16-bit map (lane = channel) and leaves its
//     outputs in registers; once every wave has finished reading, they go back as an fp32 [225 px][64 ch] image
//     (272-byte rows) -- the one transpose between the depthwise layout (lane = channel, registers = pixels) and
//     the MLP's (lane = pixel).  Each lane reads its own pixel's channels back in fc1's k order, does the LayerNorm
//     in registers (in-lane sums + one exchange with lane ^ 32, as the stem's and the downsample's) and holds the
//     MFMA B operand: no cross-wave reduction, no 16-bit LayerNorm image.  The MLP writes the new x back at its end;
//   * the pointwise filters stream through a 3-slot ring of 8 KB chunks (32 hidden units: W1 rows
//     + W2 columns) by LDS-DMA straight from the plain row-major 16-bit filters -- the per-lane
//     source address does the re-arrangement (XOR swizzles for conflict-free ds_read_b128, and the
//     W1 rows of a chunk in bit-2/bit-3-swapped order so that the fc1 accumulator of a lane IS the
//     fc2 B operand in plain k order).  Slots 0 and 1, which receive chunks 0 and 1 during the depthwise phase, lie
//     behind the image; slot 2 overlays the image's tail, which is dead before chunk 2 is requested;
//   * layer scale is folded into the fc2 filter (gamma * W2, packed once), so fc2 accumulates
//     straight into the fp32 residual registers: no second accumulator tile;
//   * a wave owns 64 pixels (2 column blocks of the 32x32 MFMA): residual = 64 registers.
#include <type_traits>

#include "stage0.h"
#include "stage_regs.h"

namespace {

constexpr int C = 64, HW = 15, P = 225, CT = 2, HID = 256;
constexpr int PITCH = 2 * C + 16;                 // [pixel][channel] image: 144 bytes per pixel row
static_assert(C == StageRegs<CT>::C && PITCH == StageRegs<CT>::PITCH, "ln_regs / regs_to_map derive both from CT");
static_assert(256 * PITCH <= C * 800, "the [pixel][channel] image overlays the planar one");
// planar image for the depthwise phase: [channel][x quad 0..3][row -3..18][4 x] in the operand type.
// 8-byte entries (4 consecutive x of one row); 22 rows of a quad are contiguous, so the four lanes j of a
// 4x4x4 MFMA block read 4 consecutive entries; the channel stride (100 entries) is 4 mod 32, which spreads
// the 8 blocks x 4 rows of a 32-lane half over all 32 eight-byte bank slots: ds_read_b64 without conflicts.
constexpr int PL_ROWS = 22, PL_XQ = PL_ROWS * 8, PL_CH = 800;
constexpr int PLB = C * PL_CH;                    // 51200 (the [pixel][channel] image overlays it)
constexpr int CHUNKB = 8192, NCH = HID / 32, NSLOT = 3;
// per-block parameter image in HBM (launch_pack_s0par):
//   Toeplitz taps, operand type: [r = ky * 3 + (rb + 1)][channel][i][k] = W[channel][ky][4 rb + k - i + 3] (0 outside
//   the 7 taps): the A operand of the 4x4x4 MFMA that maps input columns 4 (xb + rb) + k to outputs 4 xb + i;
//   then fp32: dw bias [64] | LN weight [64] | LN bias [64] | fc1 bias [256] | gamma * fc2 bias [64]
constexpr int TW_R = 21, TW_BYTES = TW_R * C * 4 * 4 * 2;   // 43008
constexpr int PF_DWB = 0, PF_LNW = C, PF_LNB = 2 * C, PF_B1 = 3 * C, PF_B2 = PF_B1 + HID, PF_FLOATS = 512;
static_assert(PF_B2 + C == PF_FLOATS, "parameter image layout");
constexpr int PARB = TW_BYTES + PF_FLOATS * 4;    // 45056
// split mode (BTSBOT_F16X2): the taps' f16 remainders follow their heads, the fp32 part comes last
constexpr int PARB_X2 = 2 * TW_BYTES + PF_FLOATS * 4;
// the fp32 [pixel][channel] image between the depthwise phase and the LayerNorm: 225 rows of 68 dwords, so the rows of
// lanes i = 0..15 start at banks 4 i (ds_read_b128 without conflicts); a transposing store (16 channels x 4 rows, 15
// pixels apart) is 2-way, which a ds_write_b32 does not pay for
constexpr int LNP = 4 * C + 16;                   // 272
constexpr int LNIMGB = P * LNP;                   // 61200
static_assert(LNIMGB % 16 == 0 && PLB + CHUNKB <= LNIMGB, "ring slot 2 inside the image's tail, behind the planar image");
// LDS layout: the image region (planar image, fp32 image, the downsample's 16-bit map: never live together), ring
// slots 0 and 1 behind it, slot 2 over the fp32 image's tail at byte 51200 (zero_planar() never touches it), then the
// block's fp32 words and the downsample's (kernel-lifetime constants, fetched once in the prologue).  Split mode (X2): a second planar image behind the first (the f16 remainders of the map the
// depthwise phase reads; the fp32 image fits inside the two) and chunks of twice the size (the filters' remainders
// behind their heads), all three slots behind the images -- 153,344 bytes, one workgroup per CU.
template <bool X2> struct S0L {
  static constexpr int PLANES = X2 ? 2 : 1;
  static constexpr int CHB = X2 ? 2 * CHUNKB : CHUNKB;     // bytes of a ring slot
  static constexpr int OFF_RING = X2 ? PLANES * PLB : LNIMGB;
  static constexpr int OFF_SLOT2 = X2 ? OFF_RING + 2 * CHB : PLB;
  static constexpr int OFF_B1 = OFF_RING + (X2 ? NSLOT : 2) * CHB;   // 256 + 3 x 64 floats: this block's fc1 bias, gamma*b2, LN weight, LN bias
  // kernel-lifetime constants, fp32: the downsample's LN weight [64] | LN bias [64] | conv bias [128], then the stem's
  // bias [64] | LN weight [64] | LN bias [64]
  static constexpr int OFF_DSC = OFF_B1 + (HID + 3 * C) * 4;
  static constexpr int LDS_BYTES = OFF_DSC + 7 * C * 4;              // 81168 (two workgroups per CU) / 155136
  static __device__ __forceinline__ int slot(int s) { return s == 2 ? OFF_SLOT2 : OFF_RING + s * CHB; }
};
static_assert(S0L<false>::LDS_BYTES <= 81920, "two workgroups per CU");
static_assert(S0L<true>::LDS_BYTES <= 160 * 1024, "one workgroup per CU");
static_assert(LNIMGB <= S0L<true>::OFF_RING && LNIMGB <= S0L<false>::OFF_RING, "the fp32 image in front of ring slots 0 and 1");

#define SB_STAMP(i)                                                                \
  do {                                                                             \
    if (a.stamps != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {             \
      a.stamps[i] = clock64();                                                     \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* keep the counted waits of the DMA ring exact */ \
    }                                                                              \
    if (a.wgt != nullptr && threadIdx.x == 0 && ((i) == 0 || (i) == 13))           \
      a.wgt[2 * blockIdx.x + ((i) == 13)] = wall_clock64();                        \
  } while (0)

struct __attribute__((packed, aligned(4))) f4u { float v[4]; };

// this lane's pixel (32 of its 64 channels: rows (r & 3) + 8 (r >> 2) + 4 h of column block ct) into the planar
// image; the zero padding around the 15x15 map is never touched
// (LOPLANE > 0: also the values' f16 remainders, LOPLANE bytes behind -- split mode)
// (SAT: the value is clamped to the f16 range first -- the keeping forms run their depthwise phase on f16 operands in
//  every mode, and a bf16 handle's residual stream may exceed 65504: saturate instead of inf -> NaN through the LayerNorm)
template <typename T, int LOPLANE = 0, bool SAT = false>
__device__ __forceinline__ void regs_to_planar(const f32x16 (&x)[CT], unsigned char* pl, int p, int h) {
  const int y = p / HW, xx = p - y * HW;
  unsigned char* dst = pl + (xx >> 2) * PL_XQ + (y + 3) * 8 + (xx & 3) * 2 + h * 4 * PL_CH;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const T hi = (T)(SAT ? __builtin_amdgcn_fmed3f(x[ct][r], -65504.0f, 65504.0f) : x[ct][r]);
      *reinterpret_cast<T*>(dst + (ct * 32 + 8 * (r >> 2) + (r & 3)) * PL_CH) = hi;
      if (LOPLANE > 0)
        *reinterpret_cast<T*>(dst + LOPLANE + (ct * 32 + 8 * (r >> 2) + (r & 3)) * PL_CH) = (T)(x[ct][r] - (float)hi);
    }
}

__device__ __forceinline__ void regs_to_tap(const f32x16 (&x)[CT], float* tap, int h) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd)
      *reinterpret_cast<float4*>(tap + ct * 32 + 8 * qd + 4 * h) =
          make_float4(x[ct][4 * qd], x[ct][4 * qd + 1], x[ct][4 * qd + 2], x[ct][4 * qd + 3]);
}

// X2 (BTSBOT_F16X2, T = f16): the LayerNorm outputs and the hidden activations go to the matrix pipe as f16 head +
// f16 remainder (two products per k-step against the f16 filters), the depthwise taps likewise (two 4x4x4 products per
// tap fragment against the f16 map), the downsample with both operands split (three products).  What stays plain f16
// -- the stem's operands, the map the depthwise phase reads, the pointwise filters -- is budgeted in DESIGN.md
// (tools/error_budget2.py): 1.4e-5 rms of the 1e-4 score tolerance for the whole network.
// WPS = waves per SIMD the register allocation leaves room for (2: two workgroups per CU, 256 registers; 1: one
// workgroup per CU with 512 registers -- the split mode's doubled fragments spill at 256)
// KEEP: the training forward (Stage0Args::keep_*): the same kernel plus the copies the backward reads
// HT: the type in which the hidden activations (and with them gamma * W2, Stage0Blk::w2g) reach the matrix pipe.  The
// bf16 inference form takes f16.  Every single-operand inference form with f16 hidden activations -- that one and the f16
// handle's -- applies the GELU as gelu_pk4() on pairs of neighbouring fc1 accumulator registers: 5.5 issue slots per value
// against 7.5 (gelu_poly<3> and the rounding to bf16) and 9 (gelu_poly<5>, f16), and for the bf16 handle 11 significant
// bits of the hidden value against 8.  The keeping forms have HT = T and gelu_for<T>, because the backward
// differentiates gelu_poly; the split form keeps gelu_poly<5>, whose remainder operand needs the fp32 value.
template <typename T, bool X2, int WPS = 2, bool KEEP = false, typename HT = T>
__global__ __launch_bounds__(256, WPS) void stage0b_kernel(Stage0Args a) {
  using frag = typename Mfma<T>::frag;
  using hfrag = typename Mfma<HT>::frag;
  constexpr bool PKG = std::is_same<HT, f16_t>::value && !X2 && !KEEP;   // the packed-f16 GELU
  static_assert(std::is_same<HT, T>::value || PKG, "a hidden type of its own: f16, inference, one operand");
  // the depthwise phase's operand type: the training forward reads map and taps as f16 in the bf16 mode too -- the
  // map is the fp32 residual stream, and its rounding to bf16 in front of 49 products moved a 50-step bf16 training
  // run ten times further from the fp32 recipe than the per-op forward's fp32 convolution (test_16bit_training_follows_
  // the_fp32_recipe: worst loss difference 4.0e-2 against 4.0e-3); f16 keeps 11 bits of it
  using DT = typename std::conditional<KEEP, f16_t, T>::type;
  using frag4 = typename Mfma<DT>::frag4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* map = smem;     // 16-bit [pixel][channel] image (downsample input)
  unsigned char* pl = smem;      // planar image (depthwise operand) and the fp32 [pixel][channel] image: same bytes, never live together
  using L = S0L<X2>;
  constexpr int PLO = X2 ? PLB : 0;                  // split mode: the planar image of the remainders
  float* b1s = reinterpret_cast<float*>(smem + L::OFF_B1);
  float* b2s = b1s + HID;
  float* lnws = b2s + C;         // this block's LayerNorm weight and bias
  float* lnbs = lnws + C;
  float* dscs = reinterpret_cast<float*>(smem + L::OFF_DSC);   // ds_lnw | ds_lnb | ds_b | stem_b | stem_lnw | stem_lnb

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, h = lane >> 5;
  const int alert = blockIdx.x;
  int pix[2];
  bool live[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    pix[t] = wave * 64 + t * 32 + lr;     // this lane's pixel slot of column block t
    live[t] = pix[t] < P;
  }
  // depthwise roles: lane = (block b = channel 16 wave + b, row offset j)
  const int dj = lane & 3, dch = wave * 16 + (lane >> 2);

  SB_STAMP(0);
  // ---- the vector-memory queue returns in order, so what the first products need is requested first: both column
  //      blocks' image rows (2 x 3 channels x 2 rows of 4 pixels, unaligned 16-byte loads), whose HBM latency then runs
  //      under the zero fill below instead of behind a block's 43 KB of taps
  f4u iq[2][3][2];
  {
    const float* src = a.img + (size_t)alert * 3 * 63 * 63;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int pc = live[t] ? pix[t] : 0;
      const int py = pc / HW, px = pc - py * HW;
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {     // k-step = input channel: k = ci*16 + ky*4 + kx
        const float* r0 = src + (ci * 63 + 4 * py + 2 * h) * 63 + 4 * px;
        iq[t][ci][0] = *reinterpret_cast<const f4u*>(r0);
        iq[t][ci][1] = *reinterpret_cast<const f4u*>(r0 + 63);
      }
    }
  }
  // the kernel-lifetime constants, the same for every workgroup: the downsample's LayerNorm weight and bias and its
  // conv bias (one float per lane), the stem's bias and LayerNorm weight and bias (waves 0-2); in LDS before the first
  // barrier.  Neither the stem nor the tail then waits for a parameter behind other requests.
  const float dscv = tid < C ? a.ds_lnw[tid] : tid < 2 * C ? a.ds_lnb[tid - C] : a.ds_b[tid - 2 * C];
  const float stcv = tid < C ? a.stem_b[tid] : tid < 2 * C ? a.stem_lnw[tid - C] : tid < 3 * C ? a.stem_lnb[tid - 2 * C] : 0.f;
  // the stem's filter fragments
  frag saf[3][CT], safl[X2 ? 3 : 1][CT];
  {
    const T* sw = reinterpret_cast<const T*>(a.stem_w);
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        saf[ci][ct] = *reinterpret_cast<const frag*>(sw + (ct * 32 + lr) * 48 + ci * 16 + h * 8);
        if (X2)
          safl[ci][ct] = *reinterpret_cast<const frag*>(reinterpret_cast<const T*>(a.stem_w_lo) + (ct * 32 + lr) * 48 + ci * 16 + h * 8);
      }
  }
  __builtin_amdgcn_sched_barrier(0);
  // a block's Toeplitz taps (16 channels x 4 rows x 21 fragments per wave, lane-linear 8-byte loads) and its
  // per-lane scalars: requested one phase ahead of the depthwise convolution that needs them
  frag4 tw[TW_R], twl[X2 ? TW_R : 1];
  float dwbias, lng, lnb2, b1v, b2v;
  auto load_block_params = [&](int j) {
    const Stage0Blk& bk = a.blk[j];
    const uint2* src = reinterpret_cast<const uint2*>(bk.par) + wave * 64 + lane;
#pragma unroll
    for (int r = 0; r < TW_R; ++r) tw[r] = __builtin_bit_cast(frag4, src[r * 256]);
    if (X2) {
#pragma unroll
      for (int r = 0; r < TW_R; ++r) twl[r] = __builtin_bit_cast(frag4, src[TW_BYTES / 8 + r * 256]);
    }
    const float* pf = reinterpret_cast<const float*>(bk.par + (X2 ? 2 : 1) * TW_BYTES);
    dwbias = pf[PF_DWB + dch];
    lng = pf[PF_LNW + (tid & 63)];
    lnb2 = pf[PF_LNB + (tid & 63)];
    b1v = pf[PF_B1 + tid];
    b2v = pf[PF_B2 + (tid & 63)];
  };
  load_block_params(0);   // lands under the stem
  auto zero_planar = [&]() {
    for (int i = tid; i < L::PLANES * PLB / 16; i += 256) reinterpret_cast<uint4*>(pl)[i] = make_uint4(0u, 0u, 0u, 0u);
  };
  zero_planar();
  dscs[tid] = dscv;
  if (tid < 3 * C) dscs[4 * C + tid] = stcv;
  __syncthreads();

  // ============================ stem: conv 4x4 s4 + LN =====================================
  // (operands requested in the prologue; bias and LayerNorm parameters are words of LDS: one counted wait per column
  //  block for its image rows, none for a parameter)
  f32x16 x[2][CT];
  {
    const float* stbs = dscs + 4 * C;   // stem bias | LN weight | LN bias
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const f32x4 bv = lds_f32x4(stbs + ct * 32 + 8 * qd + 4 * h);
          x[t][ct][4 * qd + 0] = bv[0];
          x[t][ct][4 * qd + 1] = bv[1];
          x[t][ct][4 * qd + 2] = bv[2];
          x[t][ct][4 * qd + 3] = bv[3];
        }
#pragma unroll
      for (int ci = 0; ci < 3; ++ci) {     // k-step = input channel: k = ci*16 + ky*4 + kx
        const f4u v0 = iq[t][ci][0];
        const f4u v1 = iq[t][ci][1];
        frag bf, bfl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bf[e] = (T)v0.v[e];
          bf[4 + e] = (T)v1.v[e];
          if (X2) {
            bfl[e] = (T)(v0.v[e] - (float)bf[e]);
            bfl[4 + e] = (T)(v1.v[e] - (float)bf[4 + e]);
          }
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          if (X2) {
            x[t][ct] = Mfma<T>::m32(safl[ci][ct], bf, x[t][ct]);
            x[t][ct] = Mfma<T>::m32(saf[ci][ct], bfl, x[t][ct]);
          }
          x[t][ct] = Mfma<T>::m32(saf[ci][ct], bf, x[t][ct]);
        }
      }
      if (KEEP && live[t]) regs_to_tap(x[t], a.keep_stem_pre + ((size_t)alert * P + pix[t]) * C, h);
      ln_regs<true>(x[t], stbs + C, stbs + 2 * C, h, x[t]);
      if (live[t]) regs_to_planar<DT, PLO, KEEP && !std::is_same<T, f16_t>::value>(x[t], pl, pix[t], h);
      if (a.tap_stem != nullptr && live[t])
        regs_to_tap(x[t], a.tap_stem + ((size_t)alert * P + pix[t]) * C, h);
    }
  }
  SB_STAMP(1);   // stem done

  // ============================ two ConvNeXt blocks ========================================
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const Stage0Blk& bk = a.blk[j];
    SB_STAMP(2 + 5 * j);
    __syncthreads();   // planar image complete (stem / previous MLP); ring free; the block's fp32 words idle
    b1s[tid] = b1v;
    if (tid < C) {
      b2s[tid] = b2v;
      lnws[tid] = lng;
      lnbs[tid] = lnb2;
    }

    // ---- pointwise filters: chunk = 32 hidden units = 8 pieces of 1 KiB, 2 per wave.
    //      pieces 0..3: W1 rows (LDS row m <- hidden unit 32*ch + swap23(m)), 128-byte rows,
    //                   16-byte chunk c of row r at position c ^ ((r >> 1) & 7)
    //      pieces 4..7: gamma*W2 columns 32*ch .. +31 of the 64 channel rows, 64-byte rows,
    //                   chunk c of row r at position c ^ F[(r >> 2) & 3]
    const unsigned char* wsrc[2];
    const unsigned char* wsrcl[2];   // split mode: the same pieces of the remainder images, 8 KB further into the slot
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = wave * 2 + i;
      if (pc < 4) {
        const int m = pc * 8 + (lane >> 3);
        const int hid = (m & ~12) | ((m & 4) << 1) | ((m & 8) >> 1);   // swap bits 2 and 3
        const size_t o = (size_t)hid * (C * 2) + (((lane & 7) ^ ((m >> 1) & 7)) << 4);
        wsrc[i] = bk.w1 + o;
        wsrcl[i] = X2 ? bk.w1_lo + o : nullptr;
      } else {
        const int r = (pc - 4) * 16 + (lane >> 2);
        const size_t o = (size_t)r * (HID * 2) + (((lane & 3) ^ swz4(r)) << 4);
        wsrc[i] = bk.w2g + o;
        wsrcl[i] = X2 ? bk.w2g_lo + o : nullptr;
      }
    }
    // chunk ch adds 32 W1 rows (4096 B) resp. 32 W2 columns (64 B)
    const int wstep0 = wave < 2 ? 32 * C * 2 : 64;
    auto issue = [&](int ch) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_global_load_lds((gptr_t)(wsrc[i] + (size_t)ch * wstep0),
                                         (lptr_t)(smem + L::slot(ch % NSLOT) + (wave * 2 + i) * 1024),
                                         16, 0, 0);
      if (X2) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
          __builtin_amdgcn_global_load_lds((gptr_t)(wsrcl[i] + (size_t)ch * wstep0),
                                           (lptr_t)(smem + L::slot(ch % NSLOT) + CHUNKB + (wave * 2 + i) * 1024),
                                           16, 0, 0);
      }
    };
    SB_STAMP(3 + 5 * j);

    // ---- depthwise 7x7 on the matrix pipe: per channel (= MFMA block) and output tile (4 rows yb, 4 columns xb)
    //      D[i][j] = out[4 yb + j][4 xb + i] = sum over ky, rb, k of  W[ky][4 rb + k - i + 3] * in[4 yb + j + ky - 3][4 (xb + rb) + k]
    //      A = the Toeplitz taps (registers), B = 4 consecutive x of 4 consecutive rows (one ds_read_b64 per lane);
    //      a row step s = 4 yb + ky serves every (yb, ky) pair with that sum: 76 reads, 280 MFMAs per wave.
    float v[64];
    {
      f32x4 acc[4][4];
#pragma unroll
      for (int yb = 0; yb < 4; ++yb)
#pragma unroll
        for (int xb = 0; xb < 4; ++xb) acc[yb][xb] = f32x4{dwbias, dwbias, dwbias, dwbias};
      const unsigned char* lb = pl + dch * PL_CH + dj * 8;
      // (the row step's four reads are requested a whole step -- 10 to 48 products -- ahead of their use: read and used in
      //  the same step, every step began with an exposed LDS round trip, 19 per block, about as long as the products)
      frag4 bq[2][4], bql[X2 ? 2 : 1][X2 ? 4 : 1];
      auto read_step = [&](int s, int buf) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bq[buf][q] = __builtin_bit_cast(frag4, *reinterpret_cast<const uint2*>(lb + q * PL_XQ + s * 8));
          if (X2) bql[buf][q] = __builtin_bit_cast(frag4, *reinterpret_cast<const uint2*>(lb + PLB + q * PL_XQ + s * 8));
        }
      };
      read_step(0, 0);
#ifdef S0_EXP_NODW
#pragma unroll 1
      for (int s = 0; s < 1; ++s) {
#else
#pragma unroll
      for (int s = 0; s < 19; ++s) {
#endif
        // (touching this step's fragments makes hipcc wait for them HERE, while they are the only LDS reads in flight:
        //  placed by itself the wait lands behind the next step's reads -- lgkmcnt(0), their whole latency exposed)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          asm volatile("" : "+v"(bq[s & 1][q]));
          if (X2) asm volatile("" : "+v"(bql[X2 ? s & 1 : 0][X2 ? q : 0]));
        }
        if (s + 1 < 19) read_step(s + 1, (s + 1) & 1);
        if (s == 0) {
          // the taps are in registers by now: only now queue the filter chunks (a wait for an ordinary load
          // placed behind an LDS-DMA would wait for the DMA too)
          __builtin_amdgcn_sched_barrier(0);
          issue(0);
          issue(1);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int yb = 0; yb < 4; ++yb) {
          const int ky = s - 4 * yb;
          if (ky < 0 || ky > 6) continue;
#pragma unroll
          for (int rbi = 0; rbi < 3; ++rbi)
#pragma unroll
            for (int xb = 0; xb < 4; ++xb) {
              const int q = xb + rbi - 1;
              if (q < 0 || q > 3) continue;
              if (X2) {   // remainders first (small terms into the accumulator before the large one)
                acc[yb][xb] = Mfma<DT>::m4(twl[ky * 3 + rbi], bq[s & 1][q], acc[yb][xb]);
                acc[yb][xb] = Mfma<DT>::m4(tw[ky * 3 + rbi], bql[X2 ? s & 1 : 0][X2 ? q : 0], acc[yb][xb]);
              }
              acc[yb][xb] = Mfma<DT>::m4(tw[ky * 3 + rbi], bq[s & 1][q], acc[yb][xb]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int yb = 0; yb < 4; ++yb)
#pragma unroll
        for (int xb = 0; xb < 4; ++xb)
#pragma unroll
          for (int i = 0; i < 4; ++i) v[yb * 16 + xb * 4 + i] = acc[yb][xb][i];
    }
    if (KEEP && a.keep_d[j] != nullptr) {   // the depthwise output before the LayerNorm: lane = (channel, row j of the quad), 60 live
                                             // values (nullptr: the backward recomputes it, dwln_bwd.hip)
      float* dst = a.keep_d[j] + (size_t)alert * P * C + dch;
#pragma unroll
      for (int yb = 0; yb < 4; ++yb)
#pragma unroll
        for (int xb = 0; xb < 4; ++xb)
          if (yb < 3 || dj < 3) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (xb == 3 && i == 3) continue;
              dst[((4 * yb + dj) * HW + 4 * xb + i) * C] = v[yb * 16 + xb * 4 + i];
            }
          }
    }
    SB_STAMP(4 + 5 * j);   // depthwise done
    // ---- the one transpose: the depthwise outputs (lane = channel, registers = pixels) as fp32 into the
    //      [pixel][channel] image, which overlays the planar image that other waves may still be reading
    __syncthreads();   // nobody reads the planar image any more
    {
      float* dst = reinterpret_cast<float*>(smem + dj * HW * LNP) + dch;
#pragma unroll
      for (int yb = 0; yb < 4; ++yb)
#pragma unroll
        for (int xb = 0; xb < 4; ++xb)
          if (yb < 3 || dj < 3) {   // row 15 is padding (and lies behind the image)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (xb == 3 && i == 3) continue;   // column 15 is padding
              dst[(4 * yb * HW + 4 * xb + i) * (LNP / 4)] = v[yb * 16 + xb * 4 + i];
            }
          }
    }
    if (j == 0) SB_STAMP(14);
    __syncthreads();   // fp32 image complete
    if (j == 0) SB_STAMP(15);

    // ---- LayerNorm in registers -> fc1 -> GELU -> fc2 over 8 chunks; fc2 accumulates into x (gamma is in the filter)
    {
      // this lane's pixel, 32 of its 64 channels per column block in fc1's k order (k-step ks: channels 16 ks + 8 h
      // + 0..7); the partner lane ^ 32 holds the other 32: two-pass statistics as ln_regs(); the normalised value is
      // rounded once to the operand type (split mode: its f16 remainder from the same fp32 value)
      frag xf[2][4], xfl[X2 ? 2 : 1][4];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        // (lanes of the dead pixel slots 225..255 read the last row: their values are never used)
        const unsigned char* row = smem + (live[t] ? pix[t] : P - 1) * LNP + h * 32;
        float xv[32];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const float4 r4 = *reinterpret_cast<const float4*>(row + ks * 64 + q * 16);
            xv[ks * 8 + q * 4 + 0] = r4.x;
            xv[ks * 8 + q * 4 + 1] = r4.y;
            xv[ks * 8 + q * 4 + 2] = r4.z;
            xv[ks * 8 + q * 4 + 3] = r4.w;
          }
        float s = 0.f;
#pragma unroll
        for (int n = 0; n < 32; ++n) s += xv[n];
        s += __shfl_xor(s, 32, 64);
        const float mean = s * (1.0f / C);
        float q2 = 0.f;
#pragma unroll
        for (int n = 0; n < 32; ++n) {
          xv[n] -= mean;
          q2 += xv[n] * xv[n];
        }
        q2 += __shfl_xor(q2, 32, 64);
        const float rstd = rsqrtf(q2 * (1.0f / C) + LN_EPS);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const float4 w4 = *reinterpret_cast<const float4*>(lnws + ks * 16 + h * 8 + q * 4);
            const float4 b4 = *reinterpret_cast<const float4*>(lnbs + ks * 16 + h * 8 + q * 4);
            const float ww[4] = {w4.x, w4.y, w4.z, w4.w}, bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float y = xv[ks * 8 + q * 4 + e] * rstd * ww[e] + bb[e];
              const T yh = (T)y;
              xf[t][ks][q * 4 + e] = yh;
              if (X2) xfl[t][ks][q * 4 + e] = (T)(y - (float)yh);
            }
          }
          if (KEEP && live[t])   // the LayerNorm output for the backward: this lane's 16-byte piece of the pixel's row
            *reinterpret_cast<frag*>(reinterpret_cast<unsigned char*>(a.keep_xn[j]) +
                                     ((size_t)alert * P + pix[t]) * C * 2 + ks * 32 + h * 16) = xf[t][ks];
        }
      }
      SB_STAMP(5 + 5 * j);   // LN done: every B operand of the MLP is in registers
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const float4 bv = *reinterpret_cast<const float4*>(b2s + ct * 32 + 8 * qd + 4 * h);
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            x[t][ct][4 * qd + 0] += bv.x;
            x[t][ct][4 * qd + 1] += bv.y;
            x[t][ct][4 * qd + 2] += bv.z;
            x[t][ct][4 * qd + 3] += bv.w;
          }
        }
#ifdef S0_EXP_NOLOOP
#pragma unroll 1
      for (int ch = 0; ch < 0; ++ch) {
#else
#pragma unroll 1
      for (int ch = 0; ch < NCH; ++ch) {
#endif
        // this wave's pieces of chunk ch have landed once only the younger chunk is outstanding
        if (ch + 1 < NCH) wait_vm<X2 ? 4 : 2>();
        else wait_vm<0>();
        // raw barrier: __syncthreads() would also wait vmcnt(0) while an LDS-DMA is in flight and so drain the two
        // chunks this ring keeps ahead (the chunk time then IS the DMA latency, ~2k cycles for ~1k of work)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // chunk ch has landed for everyone; chunk ch-1 is read out
        // the fp32 image is dead once every wave holds its xf (ch == 0: ring slot 2, in its tail, may be filled):
        // clear it for the next block's planar image (whose padding must read as zero) while the matrix pipe works
        if (ch == 1 && j == 0) zero_planar();
        const unsigned char* w1s = smem + L::slot(ch % NSLOT);
        const unsigned char* w2s = w1s + 4096;
        frag a1[4], a1l[X2 ? 4 : 1];
        hfrag a2[CT][2], a2l[X2 ? CT : 1][2];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          a1[ks] = *reinterpret_cast<const frag*>(w1s + lr * 128 + (((ks * 2 + h) ^ ((lr >> 1) & 7)) << 4));
          if (X2) a1l[ks] = *reinterpret_cast<const frag*>(w1s + CHUNKB + lr * 128 + (((ks * 2 + h) ^ ((lr >> 1) & 7)) << 4));
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const int r = ct * 32 + lr;
            a2[ct][s2] = *reinterpret_cast<const hfrag*>(w2s + r * 64 + (((s2 * 2 + h) ^ swz4(r)) << 4));
            if (X2) a2l[ct][s2] = *reinterpret_cast<const hfrag*>(w2s + CHUNKB + r * 64 + (((s2 * 2 + h) ^ swz4(r)) << 4));
          }
        // (inline asm: behind a compiler-visible ds_read of anything but the ring hipcc waits vmcnt(0) -- it cannot
        //  tell that the bias words are not an LDS-DMA destination -- and the ring's two chunks in flight are gone)
        f32x4 bq[4];
        {
          const unsigned baddr = (unsigned)(size_t)(lptr_t)(b1s + ch * 32 + 8 * h);
          asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:64\n\t"
                       "ds_read_b128 %3, %4 offset:80\n\ts_waitcnt lgkmcnt(0)"
                       : "=&v"(bq[0]), "=&v"(bq[1]), "=&v"(bq[2]), "=&v"(bq[3]) : "v"(baddr) : "memory");
        }
        // every fragment read is queued before the first product (see stage1b.hip)
        __builtin_amdgcn_sched_barrier(0);
        // both column blocks' fc1 first: the second one's MFMAs run under the first one's GELU
        f32x16 hacc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          // accumulator row (r&3) + 8(r>>2) + 4h holds hidden unit 32ch + (r&3) + 4((r>>2)&1) + 8h + 16(r>>3)
#pragma unroll
          for (int qd = 0; qd < 4; ++qd)
#pragma unroll
            for (int e = 0; e < 4; ++e) hacc[t][4 * qd + e] = bq[qd][e];
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            if (X2) {
              hacc[t] = Mfma<T>::m32(a1l[ks], xf[t][ks], hacc[t]);
              hacc[t] = Mfma<T>::m32(a1[ks], xfl[t][ks], hacc[t]);
            }
            hacc[t] = Mfma<T>::m32(a1[ks], xf[t][ks], hacc[t]);
          }
        }
        // (issued here, not at the barrier: an LDS-DMA holds the issuing wave ~90 cycles per
        //  instruction, which now passes while the fc1 MFMAs drain)
        if (ch + 2 < NCH) issue(ch + 2);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          // GELU in two halves, each followed by the fc2 MFMAs that consume it
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            hfrag hf, hfl;
            if constexpr (PKG) {
              // registers 8 s2 + 2 i and + 1 are neighbouring k of the fc2 B fragment: the packed result is its dword i
              float hx[8];
#pragma unroll
              for (int r = 0; r < 8; ++r) hx[r] = hacc[t][8 * s2 + r];
              f16x2v g2[4];
              gelu_pk4(hx, g2);
              hf = __builtin_shufflevector(__builtin_shufflevector(g2[0], g2[1], 0, 1, 2, 3),
                                           __builtin_shufflevector(g2[2], g2[3], 0, 1, 2, 3), 0, 1, 2, 3, 4, 5, 6, 7);
            } else {
#pragma unroll
              for (int r = 0; r < 8; ++r) {
#ifdef S0_EXP_NOGELU
                const float gv = hacc[t][8 * s2 + r];
#else
                const float gv = gelu_for<T>(hacc[t][8 * s2 + r]);
#endif
                hf[r] = (HT)gv;
                if (X2) hfl[r] = (HT)(gv - (float)hf[r]);
              }
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
              if (X2) {
                x[t][ct] = Mfma<HT>::m32(a2l[ct][s2], hf, x[t][ct]);
                x[t][ct] = Mfma<HT>::m32(a2[ct][s2], hfl, x[t][ct]);
              }
              x[t][ct] = Mfma<HT>::m32(a2[ct][s2], hf, x[t][ct]);
            }
          }
        }
      }
      // next block's depthwise operand (the region was cleared during this MLP)
      if (j == 0) {
        load_block_params(1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (live[t]) regs_to_planar<DT, PLO, KEEP && !std::is_same<T, f16_t>::value>(x[t], pl, pix[t], h);
          if (KEEP && live[t]) regs_to_tap(x[t], a.keep_xin1 + ((size_t)alert * P + pix[t]) * C, h);
        }
      }
    }
    SB_STAMP(6 + 5 * j);   // MLP done
  }
  if (a.tap_stage != nullptr) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (live[t]) regs_to_tap(x[t], a.tap_stage + ((size_t)alert * P + pix[t]) * C, h);
  }

  // ============================ downsample: LN + conv 2x2 s2 (64 -> 128) ====================
  {
    // wave -> 32 output channels (cot = wave) x the 49 output pixels (2 column blocks); K = 4 x 64
    // (filter fragments requested first: their L2 latency passes under the LayerNorm below)
    const T* dw = reinterpret_cast<const T*>(a.ds_w) + (size_t)(wave * 32 + lr) * 256 + h * 8;
    frag af[16], afl[X2 ? 16 : 1];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) af[ks] = *reinterpret_cast<const frag*>(dw + ks * 16);
    // (every wave loaded its xf from the last block's fp32 image before that MLP's first barrier; chunks 5..7, which
    //  other waves may still be reading, lie at or behind byte 51200)
    constexpr int MAPB = 256 * PITCH;   // split mode: the remainder image follows (into the second planar image's bytes)
    static_assert(MAPB <= PLB && 2 * MAPB <= S0L<true>::OFF_RING, "the 16-bit [pixel][channel] image(s) in front of every ring slot");
    // (the lane id is laundered: hipcc otherwise computes the constants' LDS addresses in the prologue and keeps them
    //  through the whole kernel, in a register the inference forms do not have)
    int lt = tid;
    asm volatile("" : "+v"(lt));
    const int ht = (lt >> 5) & 1, lrt = lt & 31;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x16 xn[CT];
      ln_regs<true>(x[t], dscs, dscs + C, ht, xn);   // (weights from LDS: no wait behind the 16 fragments above)
      regs_to_map<T, X2 ? MAPB : 0>(xn, map, pix[t], h);
    }
    if (X2) {
      const T* dwl = reinterpret_cast<const T*>(a.ds_w_lo) + (size_t)(wave * 32 + lr) * 256 + h * 8;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) afl[ks] = *reinterpret_cast<const frag*>(dwl + ks * 16);
    }
    // raw barrier: the map is complete once everybody's LDS stores are; __syncthreads() would wait for the filter too
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (KEEP) {   // the downsample's patch rows [output pixel][q = 2 ky + kx][64] = LayerNorm'd pixels (2 oy + ky, 2 ox + kx)
      unsigned char* dst = reinterpret_cast<unsigned char*>(a.keep_patches) + (size_t)alert * 49 * 4 * C * 2;
      for (int i = tid; i < 49 * 4 * 8; i += 256) {
        const int c16 = i & 7, q = (i >> 3) & 3, o = i >> 5;
        const int pin = (2 * (o / 7) + (q >> 1)) * HW + 2 * (o % 7) + (q & 1);
        *reinterpret_cast<uint4*>(dst + (size_t)(o * 4 + q) * C * 2 + 16 * c16) =
            *reinterpret_cast<const uint4*>(map + pin * PITCH + 16 * c16);
      }
    }
    SB_STAMP(12);
    // Both column blocks' 16-step chains interleaved (two independent accumulators, each in its k order); the B fragments
    // are read two steps ahead of their products into four rotating register sets (read directly in front of its
    // product, each of the 32 products waited for an LDS round trip: stage2p.hip, part 4); the bias is a word of LDS,
    // so the only waits for vector memory are hipcc's counted ones for af.
    const unsigned char* bsrc[2];
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int o = t * 32 + lrt, oc = o < 49 ? o : 0;
      const int oy = oc / 7, ox = oc - oy * 7;
      bsrc[t] = map + (2 * oy * HW + 2 * ox) * PITCH + ht * 16;
    }
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const f32x4 bv = lds_f32x4(dscs + 2 * C + wave * 32 + 8 * qd + 4 * ht);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][4 * qd + e] = bv[e];
    }
    frag bq[4][2], bql[X2 ? 4 : 1][X2 ? 2 : 1];
    auto read_b = [&](int ks, int set) {
      const int q = ks >> 2;
      const int ofs = ((q >> 1) * HW + (q & 1)) * PITCH + (ks & 3) * 32;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bq[set][t] = *reinterpret_cast<const frag*>(bsrc[t] + ofs);
        if (X2) bql[X2 ? set : 0][X2 ? t : 0] = *reinterpret_cast<const frag*>(bsrc[t] + MAPB + ofs);
      }
    };
    read_b(0, 0);
    read_b(1, 1);
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      // (touching this step's fragments makes hipcc wait for them here, in front of the next request)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        asm volatile("" : "+v"(bq[ks & 3][t]));
        if (X2) asm volatile("" : "+v"(bql[X2 ? ks & 3 : 0][X2 ? t : 0]));
      }
      if (ks + 2 < 16) read_b(ks + 2, (ks + 2) & 3);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (X2) {
          acc[t] = Mfma<T>::m32(afl[ks], bq[ks & 3][t], acc[t]);
          acc[t] = Mfma<T>::m32(af[ks], bql[X2 ? ks & 3 : 0][X2 ? t : 0], acc[t]);
        }
        acc[t] = Mfma<T>::m32(af[ks], bq[ks & 3][t], acc[t]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int o = t * 32 + lrt;
      if (o < 49) {
        float* dst = a.out + ((size_t)alert * 49 + o) * 128 + wave * 32 + 4 * ht;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
          *reinterpret_cast<float4*>(dst + 8 * qd) =
              make_float4(acc[t][4 * qd], acc[t][4 * qd + 1], acc[t][4 * qd + 2], acc[t][4 * qd + 3]);
      }
    }
    SB_STAMP(13);
  }
}

// one block's parameter image (layout at TW_R / PF_* above); taps tap-major [49][64] fp32
template <typename T, bool X2>
__global__ void pack_s0par_kernel(const float* __restrict__ taps, const float* __restrict__ dw_b,
                                  const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                  const float* __restrict__ b1, const float* __restrict__ b2,
                                  const float* __restrict__ gamma, unsigned char* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int NTW = TW_R * C * 16;
  if (idx < NTW) {
    const int k = idx & 3, i = (idx >> 2) & 3, c = (idx >> 4) & (C - 1), r = idx >> 10;
    const int ky = r / 3, rb = r % 3 - 1, kx = 4 * rb + k - i + 3;
    const float w = (kx >= 0 && kx < 7) ? taps[(ky * 7 + kx) * C + c] : 0.f;
    const T wh = (T)w;
    reinterpret_cast<T*>(out)[idx] = wh;
    if (X2) reinterpret_cast<T*>(out)[NTW + idx] = (T)(w - (float)wh);
    return;
  }
  const int f = idx - NTW;
  if (f >= PF_FLOATS) return;
  float v;
  if (f < PF_LNW) v = dw_b[f - PF_DWB];
  else if (f < PF_LNB) v = ln_w[f - PF_LNW];
  else if (f < PF_B1) v = ln_b[f - PF_LNB];
  else if (f < PF_B2) v = b1[f - PF_B1];
  else v = gamma[f - PF_B2] * b2[f - PF_B2];
  reinterpret_cast<float*>(out + (X2 ? 2 : 1) * TW_BYTES)[f] = v;
}

template <typename T, bool X2 = false, int WPS = 2, bool KEEP = false, typename HT = T>
int launch_stage0b_t(const Stage0Args& a, hipStream_t st) {
  auto kern = stage0b_kernel<T, X2, WPS, KEEP, HT>;
  static DevOnce attr_set;
  // (BTSBOT_AMD_S0_ONE_WG=1: developer probe -- the LDS request padded so that ONE workgroup fits a CU: how the kernel's
  //  time scales from one to two waves per SIMD says what two more would buy)
  static const int pad = switch_on(SW_S0_ONE_WG) && !X2 ? 90 * 1024 - S0L<X2>::LDS_BYTES : 0;
  const int LDS_BYTES = S0L<X2>::LDS_BYTES + pad;
  if (attr_set.need()) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
    attr_set.done();
  }
  hipLaunchKernelGGL(kern, dim3(a.B), dim3(256), LDS_BYTES, st, a);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

}  // namespace

#ifdef STAGE0B_X2_TU
// ---- this translation unit (stage0x.hip) holds only the split-operand instantiation: co-compiled instantiations of
//      one kernel template share the register allocator's context and move each other's spills
int launch_stage0b_x2(const Stage0Args& a, hipStream_t st) {
  // (one workgroup per CU -- the two planar images and the doubled filter ring take 153 KB of LDS -- with 512 registers)
  return launch_stage0b_t<f16_t, true, 1>(a, st);
}
int launch_pack_s0par_x2(const float* taps, const float* dw_b, const float* ln_w, const float* ln_b, const float* b1,
                         const float* b2, const float* gamma, void* out, hipStream_t st) {
  const dim3 grid((TW_R * C * 16 + PF_FLOATS + 255) / 256), blk(256);
  hipLaunchKernelGGL((pack_s0par_kernel<f16_t, true>), grid, blk, 0, st, taps, dw_b, ln_w, ln_b, b1, b2, gamma,
                     reinterpret_cast<unsigned char*>(out));
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
#else
int launch_stage0b_x2(const Stage0Args& a, hipStream_t st);
int launch_pack_s0par_x2(const float* taps, const float* dw_b, const float* ln_w, const float* ln_b, const float* b1,
                         const float* b2, const float* gamma, void* out, hipStream_t st);

size_t s0par_bytes() { return PARB_X2; }   // (the split mode's image is the larger one)

// taps: the block's depthwise filter tap-major [49][64] fp32; the others the master parameters
int launch_pack_s0par(int prec, const float* taps, const float* dw_b, const float* ln_w, const float* ln_b,
                      const float* b1, const float* b2, const float* gamma, void* out, hipStream_t st) {
  const dim3 grid((TW_R * C * 16 + PF_FLOATS + 255) / 256), blk(256);
  unsigned char* o = reinterpret_cast<unsigned char*>(out);
  if (prec == BTSBOT_BF16)
    hipLaunchKernelGGL((pack_s0par_kernel<bf16_t, false>), grid, blk, 0, st, taps, dw_b, ln_w, ln_b, b1, b2, gamma, o);
  else if (prec == BTSBOT_F16)
    hipLaunchKernelGGL((pack_s0par_kernel<f16_t, false>), grid, blk, 0, st, taps, dw_b, ln_w, ln_b, b1, b2, gamma, o);
  else if (prec == BTSBOT_F16X2)
    return launch_pack_s0par_x2(taps, dw_b, ln_w, ln_b, b1, b2, gamma, out, st);
  else {
    btsbot_set_error("pack_s0par: precision %d is not a 16-bit mode", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

bool stage0_supported(int prec, int c0) {
  return (prec == BTSBOT_BF16 || prec == BTSBOT_F16 || prec == BTSBOT_F16X2) && c0 == 64;
}

// Needs Stage0Blk::par, ::w1 (plain [256][64]) and Stage0Blk::w2g (gamma-scaled [64][256]), 16-bit.  The bf16 inference
// form (also stage 0 of an fp8 handle) reads w2g as f16 (stage_args.hip: p_fc2g_h); its keeping form as bf16.
int launch_stage0b(int prec, const Stage0Args& a, hipStream_t st) {
  if (a.B <= 0) return BTSBOT_OK;
  if (a.keep_xn[0] != nullptr) {   // the training forward
    if (a.keep_stem_pre == nullptr || a.tap_stem == nullptr || a.keep_xin1 == nullptr || a.tap_stage == nullptr ||
        (a.keep_d[0] == nullptr) != (a.keep_d[1] == nullptr) || a.keep_xn[1] == nullptr || a.keep_patches == nullptr) {
      btsbot_set_error("stage0b: the training forward needs every kept buffer");
      return BTSBOT_ERR_INVALID_ARG;
    }
    if (prec == BTSBOT_BF16) return launch_stage0b_t<bf16_t, false, 2, true>(a, st);
    if (prec == BTSBOT_F16) return launch_stage0b_t<f16_t, false, 2, true>(a, st);
    btsbot_set_error("stage0b: the training forward runs in the bf16 / f16 modes, not %d", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (prec == BTSBOT_BF16) return launch_stage0b_t<bf16_t, false, 2, false, f16_t>(a, st);
  if (prec == BTSBOT_F16) return launch_stage0b_t<f16_t>(a, st);
  if (prec == BTSBOT_F16X2) {
    if (a.ds_w_lo == nullptr || a.stem_w_lo == nullptr || a.blk[0].w1_lo == nullptr || a.blk[0].w2g_lo == nullptr ||
        a.blk[1].w1_lo == nullptr || a.blk[1].w2g_lo == nullptr) {
      btsbot_set_error("stage0b: the split mode needs the remainder images (ds_w_lo, stem_w_lo, w1_lo, w2g_lo)");
      return BTSBOT_ERR_INVALID_ARG;
    }
    return launch_stage0b_x2(a, st);
  }
  btsbot_set_error("stage0b: unsupported precision %d", prec);
  return BTSBOT_ERR_INVALID_ARG;
}
#endif
