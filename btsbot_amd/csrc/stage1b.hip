// Stage-1 megakernel (gfx950): G alerts' 7x7x128 maps per workgroup:
//
//   2 x [ dwconv 7x7 + LN -> fc1 -> GELU -> fc2 -> layer-scale -> +x ]  ->  LN + conv 2x2 s2 (128 -> 256)
//
// Two forms of one template (S1L<G, X2> holds what follows G):
//   G = 5  inference in the bf16 / f16 modes (stage 1 of an fp8 handle too) while other forwards are in flight
//          (Schedule::s1_g5): 512 threads, the 245 pixels on 245 of 8 x 32 pixel slots, one workgroup per CU (134,992 B
//          of LDS), ceil(B / 5) workgroups: 205 CUs at 1024 alerts, the others are the other streams'.  A wave
//          takes ONE group of 16 channels over all five alerts in the depthwise phase (its 21 tap fragments loaded once),
//          2 of a filter chunk's 16 pieces (waves 0-3 W1, waves 4-7 W2) and one 32-channel tile of the downsample over both
//          32-column blocks of the 45 output pixels, so a downsample filter fragment is loaded once per workgroup.
//   G = 2  a lone forward (its launch is 3 us shorter and a lone forward has no use for idle CUs), the keeping forms
//          (training forward) and the split mode: 256 threads, 98 pixels on 4 x 32 slots, two workgroups per CU (split
//          mode: one).  Two planar images of five alerts do not fit LDS, and the backward's buffers hold what the keeping
//          forms keep.  The text below describes this form; where G = 5 differs it says so.
// Every sum runs in the same order in both forms and in every workgroup (no chunk rotation by workgroup index), so an
// alert's bits depend neither on G nor on its place in the batch: hinted and plain forwards give the same logits.
//
// (timm ConvNeXt stages[1].blocks / stages[2].downsample, reached from
// /root/reference/btsbot/architectures.py:108,132).  HBM sees [49][128] f32 in and [9][256] f32
// out per alert.  At B = 1024 the 512 workgroups are all resident at once (2 per CU) and drift
// apart, so one's depthwise phase runs under the other's MLP (MFMA + GELU).
//   * residual stream fp32 in registers, 32x32 MFMA accumulator layout: wave = 32 pixel slots of
//     the 98, lane half h and 64 registers = the 128 channels;
//   * depthwise 7x7 on the matrix pipe, as in stage0b.hip: the 16-block 4x4x4 MFMA, one block per channel,
//     A = Toeplitz taps in registers (21 fragments per group of 16 channels), B = 4 consecutive x of 4
//     consecutive rows read with one ds_read_b64 from a planar image [alert][x quad][row][channel][4 x]: the
//     channel-minor order with a 136-entry row pitch makes the 8 blocks x 4 rows of a half wave hit 32 different
//     8-byte bank slots.  Rows outside the map are one shared zero row (per-lane row offsets), column 7 of
//     the second quad is kept zero.  Wave = 2 channel groups x both alerts: 224 MFMAs, 88 reads per block (G = 5: one
//     group x five alerts: 280 MFMAs, 110 reads, no second set of taps to fetch in the middle of the phase)
//     (the VALU form this replaces: 25k cycles per block, 2 x 49 x 7 FMAs per lane plus conversions);
//   * LayerNorm: ONE transpose -- behind a barrier that ends every wave's reads of the planar image the depthwise outputs
//     (lane = channel, registers = pixels) go to LDS as fp32 [98 px][128 ch] with a 528-byte pitch (row p starts at bank
//     4 p), behind a second barrier each lane reads its own pixel's 64 channels in fc1's k order and normalises them in
//     registers (two-pass fp32 statistics, one __shfl_xor(.., 32) per sum), rounds once to the operand type and holds the
//     MLP's B operand xf (stage0b.hip).  The image lies in bytes that are dead in that phase: ring slots 0, 1
//     [0, 32768) and the head of the planar image [32768, 51744).  Every ring slot but W2 slot 0 lies inside it, so
//     the first filter chunks are requested behind the barrier that ends the row reads, under the LayerNorm arithmetic
//     (G = 5: [245 px], 129,360 B over ring slots 0, 1, the whole planar image and 9,552 B behind it; every ring slot
//     lies inside it);
//   * pointwise filters: chunks of 32 hidden units (8 KB of W1 rows + 8 KB of gamma*W2 columns) through two
//     3-slot LDS-DMA rings straight from the plain row-major filters (waves 0, 1 load W1, waves 2, 3 load W2; G = 5:
//     waves 0-3 and 4-7, two pieces each); the
//     per-lane source address applies the bank swizzles and the bit-2/bit-3 row swap that makes the fc1 accumulator
//     the fc2 B operand in plain k order (stage0b.hip); fc2 accumulates into the residual registers.  The rings
//     live in the planar image's and the fp32 LN image's bytes (dead by then).  The chunk loop is software-pipelined
//     inside the wave: W1 fragments and the fc1 bias of chunk ch+1 are in registers before step ch starts, its fc1
//     MFMAs issue between the GELUs of chunk ch, chunk ch's fc2 MFMAs between the second half's GELUs.
//
// LDS (bytes; split mode in brackets, G = 5 in braces):
//   [0, 32768)             ring slots 0, 1: W2 slots 1, 2 | the last downsample's 16-bit map(s) {[0, 66640): the map
//                          runs on into the planar image, dead by then}
//   [32768, 67584)         planar image  [.. 102400): two] {.. 119808): five alerts}; its head doubles as W1 slots 0, 1, 2
//                          and W2 slot 0 (4 x 8 KB [4 x 16 KB])
//   [0, 51744)             fp32 LN image [98][528 B], over both of the above {[0, 129360): [245][528 B]}
//   [102400, 135168)       split mode only: W2 slots 1, 2
//   OFF_B1   67584 [135168] {129360}  fc1 bias [512] | gamma*b2 [128], fp32
//   OFF_LNW  70144 [137728] {131920}  LN weight [128] | LN bias [128], fp32
//   OFF_DSC  71168 [138752] {132944}  the downsample's LN weight [128] | LN bias [128] | conv bias [256], fp32: the same for
//                          every workgroup and block, fetched once in the prologue;  end 73216 [140800] {134992}
#include "stage0.h"
#include "stage_regs.h"
#include <type_traits>

namespace {

constexpr int C = 128, HW = 7, PA = 49, CT = 4, HID = 512, KS1 = 8;
constexpr int CN = 256, PO = 9;                   // downsample: output channels, pixels per alert
constexpr int PITCH = 2 * C + 16;                 // [pixel][channel] image: 272 bytes per pixel row
static_assert(C == StageRegs<CT>::C && PITCH == StageRegs<CT>::PITCH, "ln_regs / regs_to_map derive both from CT");
constexpr int CHUNKB = 16384, HALFB = CHUNKB / 2, NCH = HID / 32, NSLOT = 3;
// planar image of the depthwise phase: [alert][x quad 0..1][row 0..6, 7 = zeros][channel, pitch 136][4 x]
constexpr int PL_ROW = 136 * 8, PL_XQ = 8 * PL_ROW, PL_AL = 2 * PL_XQ;   // 1088, 8704, 17408 per alert
constexpr int OFF_PL = 2 * CHUNKB;                // ring slots 0, 1 | planar image (its first 32 KB: W1 slots 0..2, W2 slot 0)
// Split mode (X2): a second planar image behind the first (the remainders of the map the depthwise phase reads), ring slots of
// twice the size (a filter piece's remainders 8 KB behind its heads): the W1 slots and W2 slot 0 (64 KB) lie in the two
// planar images, W2 slots 1, 2 in a region of their own -- 142,848 bytes, one workgroup per CU.
// fp32 [pixel][channel] image of the depthwise outputs (the block LayerNorm's input), from byte 0 over ring slots 0, 1 and
// the head of the planar image -- all dead between the depthwise phase and the MLP.  Pitch 132 words: row p starts at
// bank 4 p, a lane's 16-byte reads of its own row are conflict-free.
constexpr int LNP = 4 * C + 16;                   // 528
// G = alerts per workgroup: 2 on four waves (the keeping and split forms), 5 on eight waves (inference: 245 of the 256
// pixel slots live, one workgroup per CU).  What follows G: the waves, the channel groups a wave takes in the depthwise
// phase, its pieces of a filter chunk, its output tiles and the 32-column blocks of the downsample, and the LDS layout.
template <int G, bool X2> struct S1L {
  static_assert(G == 2 || (G == 5 && !X2), "two planar images of five alerts do not fit LDS");
  static constexpr int NW = G == 2 ? 4 : 8, NT = 64 * NW;       // waves, threads
  static constexpr int NPX = G * PA;                            // 98 of 128 / 245 of 256 pixel slots
  static constexpr int NG = 8 / NW;                             // depthwise: channel groups (of 16) per wave
  static constexpr int NPIECE = 16 / NW;                        // 1 KiB pieces of a filter chunk per wave
  static constexpr int NCB = (G * PO + 31) / 32;                // downsample: 32-column blocks of output pixels
  static constexpr int MAPB = NPX * PITCH;                      // 26656 / 66640: the downsample's 16-bit map, from byte 0
  static constexpr int PLB = G * PL_AL;                         // 34816 / 87040
  static constexpr int PLANES = X2 ? 2 : 1;
  static constexpr int SLB = X2 ? 2 * HALFB : HALFB;            // bytes of a W1 / W2 ring slot
  static constexpr int OFF_W2X = OFF_PL + PLANES * PLB;         // X2 only: W2 slots 1, 2
  static constexpr int LNB = NPX * LNP;                         // 51744 / 129360: the fp32 LayerNorm image, from byte 0
  // 512 floats fc1 bias + 128 floats gamma*b2: behind the planar images (G = 2) resp. behind the fp32 image, which is
  // longer than ring slots 0, 1 + the planar image at G = 5
  static constexpr int OFF_B1 = OFF_W2X + (X2 ? 2 * SLB : 0) > LNB ? OFF_W2X + (X2 ? 2 * SLB : 0) : LNB;
  static constexpr int OFF_LNW = OFF_B1 + (HID + C) * 4;        // LayerNorm weight [128] | bias [128], fp32
  static constexpr int OFF_DSC = OFF_LNW + 2 * C * 4;           // the downsample's LN weight [128] | LN bias [128] | bias [256], fp32
  static constexpr int LDS_BYTES = OFF_DSC + (2 * C + CN) * 4;  // 73216: two workgroups per CU / 140800 / G = 5: 134992
  static_assert(4 * SLB <= PLANES * PLB, "W1 slots + W2 slot 0 inside the planar images");
  static_assert(LNB <= OFF_B1 && OFF_B1 % 16 == 0, "the fp32 image ends in front of the bias words");
  static_assert((X2 ? 2 : 1) * MAPB <= OFF_B1, "the [pixel][channel] image(s) in front of the bias words");
};
static_assert(S1L<2, false>::LDS_BYTES <= 75264 && S1L<2, true>::LDS_BYTES <= 160 * 1024 && S1L<5, false>::LDS_BYTES <= 160 * 1024,
              "LDS layout");
// per-block parameter image in HBM (launch_pack_s1par): Toeplitz taps in the operand type
//   [r = ky * 3 + (rb + 1)][channel][i][k] = W[channel][ky][4 rb + k - i + 3]   (0 outside the 7 taps)
// then fp32: dw bias [128] | LN weight [128] | LN bias [128]
constexpr int TW_R = 21, TW_BYTES = TW_R * C * 4 * 4 * 2;   // 86016
constexpr int PARB = TW_BYTES + 3 * C * 4;        // 87552
// split mode (BTSBOT_F16X2): the taps' f16 remainders follow their heads, the fp32 part comes last
constexpr int PARB_X2 = 2 * TW_BYTES + 3 * C * 4;

#define SC_STAMP(i)                                                                \
  do {                                                                             \
    if (a.stamps != nullptr && blockIdx.x == 0 && threadIdx.x == 0) a.stamps[i] = clock64(); \
    if (a.wgt != nullptr && threadIdx.x == 0 && ((i) == 0 || (i) == 13))           \
      a.wgt[2 * blockIdx.x + ((i) == 13)] = wall_clock64();                        \
  } while (0)

// this lane's pixel (64 of its 128 channels: rows (r & 3) + 8 (r >> 2) + 4 h of column block ct) into the planar
// image; p = alert * 49 + y * 7 + x
// (LOPLANE > 0: also the values' f16 remainders, LOPLANE bytes behind -- split mode)
// (SAT: the value is clamped to the f16 range first -- the keeping forms run their depthwise phase on f16 operands in
//  every mode, and a bf16 handle's residual stream may exceed 65504: saturate instead of inf -> NaN through the LayerNorm)
template <typename T, int G, int LOPLANE = 0, bool SAT = false>
__device__ __forceinline__ void regs_to_planar(const f32x16 (&x)[CT], unsigned char* pl, int p, int h) {
  const int al = G == 2 ? (p >= PA ? 1 : 0) : p / PA, pp = p - al * PA;
  const int y = pp / HW, xx = pp - y * HW;
  unsigned char* dst = pl + al * PL_AL + (xx >> 2) * PL_XQ + y * PL_ROW + (xx & 3) * 2 + h * 32;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const T hi = (T)(SAT ? __builtin_amdgcn_fmed3f(x[ct][r], -65504.0f, 65504.0f) : x[ct][r]);
      *reinterpret_cast<T*>(dst + (ct * 32 + 8 * (r >> 2) + (r & 3)) * 8) = hi;
      if (LOPLANE > 0) *reinterpret_cast<T*>(dst + LOPLANE + (ct * 32 + 8 * (r >> 2) + (r & 3)) * 8) = (T)(x[ct][r] - (float)hi);
    }
}

// X2 (BTSBOT_F16X2, T = f16): as in stage0b.hip -- LayerNorm outputs and hidden activations as f16 head + remainder
// (two products per k-step against the f16 filters), the depthwise taps likewise, the downsample with both operands split.
// WPS = waves per SIMD the register allocation leaves room for (2: two workgroups per CU, 256 registers; 1: one
// workgroup per CU with 512 registers -- the split mode's doubled fragments spill at 256)
// KEEP: the training forward (Stage1Args::keep_*): the same kernel plus the copies the backward reads
template <typename T, bool X2, int WPS = 2, bool KEEP = false, int G = 2>
__global__ __launch_bounds__((S1L<G, X2>::NT), WPS) void stage1b_kernel(Stage1Args a) {
  using frag = typename Mfma<T>::frag;
  // the depthwise phase's operand type: the training forward reads map and taps as f16 in the bf16 mode too -- the
  // map is the fp32 residual stream, and its rounding to bf16 in front of 49 products moved a 50-step bf16 training
  // run ten times further from the fp32 recipe than the per-op forward's fp32 convolution (test_16bit_training_follows_
  // the_fp32_recipe: worst loss difference 4.0e-2 against 4.0e-3); f16 keeps 11 bits of it
  using DT = typename std::conditional<KEEP, f16_t, T>::type;
  using frag4 = typename Mfma<DT>::frag4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* pl = smem + OFF_PL;                 // planar image; its first 24 KB double as the W1 ring
  unsigned char* stg = smem;                         // the last downsample's 16-bit image [98][PITCH] in ring slots 0..1
  using L = S1L<G, X2>;
  static_assert(G == 2 || !KEEP, "the keeping forms hold two alerts");
  constexpr int SLB = L::SLB, NW = L::NW, NT = L::NT, NPX = L::NPX, NG = L::NG, NPIECE = L::NPIECE, PLB = L::PLB, MAPB = L::MAPB;
  constexpr int PLO = X2 ? PLB : 0;                  // split mode: the planar image of the remainders
  float* b1s = reinterpret_cast<float*>(smem + L::OFF_B1);
  float* b2s = b1s + HID;
  float* lnws = reinterpret_cast<float*>(smem + L::OFF_LNW);
  float* lnbs = lnws + C;
  float* dscs = reinterpret_cast<float*>(smem + L::OFF_DSC);   // kernel-lifetime constants: ds_lnw | ds_lnb | ds_b
  // filter rings, 3 slots of 8 KB each (split mode: 16 KB, the remainders behind the heads): the W1 slots and W2 slot 0
  // lie in the planar image(s), W2 slots 1, 2 in ring slots 0, 1 (split mode: in a region of their own); all but W2
  // slot 0 overlap the fp32 LayerNorm image, so the first request follows the barrier that ends its row reads
  auto w1slot = [&](int sl) { return pl + sl * SLB; };
  auto w2slot = [&](int sl) { return sl == 0 ? pl + 3 * SLB : (X2 ? smem + L::OFF_W2X : smem) + (sl - 1) * SLB; };

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, h = lane >> 5;
  const bool w1wave = wave < NW / 2;
  const int a0 = blockIdx.x * G;
  const int nal = min(G, a.B - a0);
  const int p = wave * 32 + lr;                      // this lane's pixel slot (MFMA phases)
  const bool live = p < nal * PA;
  const bool inmap = p < NPX;
  const int pm = inmap ? p : 0;                      // row to read for slots beyond the image
  // this lane's row of the fp32 LayerNorm image, its half's 32 bytes of every k-step
  const int lnrow = pm * LNP + h * 32;
  SC_STAMP(0);
  // what the live writes never touch and the depthwise products read: the zero rows and column 7
  auto zero_pads = [&]() {
#pragma unroll
    for (int pn = 0; pn < L::PLANES; ++pn) {
      unsigned char* pb = pl + pn * PLB;
      for (int i = tid; i < 2 * G * PL_ROW / 16; i += NT) {
        const int blk = i / (PL_ROW / 16), o = i - blk * (PL_ROW / 16);
        *reinterpret_cast<uint4*>(pb + (blk >> 1) * PL_AL + (blk & 1) * PL_XQ + 7 * PL_ROW + o * 16) = make_uint4(0u, 0u, 0u, 0u);
      }
      for (int i = tid; i < G * HW * C; i += NT) {
        const int al = i / (HW * C), r = (i / C) % HW, c = i % C;
        *reinterpret_cast<unsigned short*>(pb + al * PL_AL + PL_XQ + r * PL_ROW + c * 8 + 6) = 0;
      }
    }
  };
  // the downsample's LayerNorm weight and bias and its conv bias: one float per lane (two on four waves), in LDS before
  // block 0's first barrier -- no ordinary load may be outstanding once the filter rings run (vmcnt retires in order)
  constexpr int NDSC = (2 * C + CN) / NT;
  float dscv[NDSC];
#pragma unroll
  for (int i = 0; i < NDSC; ++i) {
    const int f = tid + i * NT;   // (wave-uniform choice: the three vectors are multiples of 64 floats)
    dscv[i] = f < C ? a.ds_lnw[f] : f < 2 * C ? a.ds_lnb[f - C] : a.ds_b[f - 2 * C];
  }
  zero_pads();
  // ---- the residual stream does NOT stay in registers through the depthwise phase (64 registers next to that
  //      phase's 64 outputs and 42 tap registers spill): it is re-read at the start of each MLP, from the stage
  //      input for block 0 and from a scratch copy (written by the same lanes, L2-resident) for block 1
  const float* xsrc = a.x_in + ((size_t)a0 * PA + (live ? p : 0)) * C;
  float* xscr = a.scratch + ((size_t)a0 * PA + (live ? p : 0)) * C;
  auto load_x = [&](const float* src, f32x16 (&x)[CT]) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const float4 v4 = *reinterpret_cast<const float4*>(src + ct * 32 + 8 * qd + 4 * h);
        x[ct][4 * qd + 0] = live ? v4.x : 0.f;
        x[ct][4 * qd + 1] = live ? v4.y : 0.f;
        x[ct][4 * qd + 2] = live ? v4.z : 0.f;
        x[ct][4 * qd + 3] = live ? v4.w : 0.f;
      }
  };
  {
    f32x16 x0[CT];
    load_x(xsrc, x0);
    if (inmap) regs_to_planar<DT, G, PLO, KEEP && !std::is_same<T, f16_t>::value>(x0, pl, p, h);
  }
#pragma unroll
  for (int i = 0; i < NDSC; ++i) dscs[tid + i * NT] = dscv[i];
  SC_STAMP(1);

  f32x16 x[CT];   // (written in full at the start of every MLP: dead through the depthwise phases)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const Stage0Blk& bk = a.blk[j];
    // depthwise roles: lane = (block b, row offset j); wave = channel groups 2 wave, 2 wave + 1 of both alerts.
    // (The lane id is laundered per block: with the block loop unrolled hipcc otherwise computes every address of
    //  BOTH blocks' depthwise / LayerNorm phases once, keeps them across the first MLP and starves its filter
    //  fragments of registers -- fc1 then waits for an LDS read in front of every MFMA.)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int dj = ln & 3, db = ln >> 2;
    // ---- ordinary loads first (vmcnt retires in order: a load younger than a DMA would wait for it): fc1 bias,
    //      gamma*b2, the first channel group's Toeplitz taps and both groups' per-channel scalars
    // (eight waves: thread tid holds fc1 bias tid alone, and the threads past 256 re-read the LN words of tid - 256)
    const float b1v0 = bk.b1[tid], b1v1 = NT == 256 ? bk.b1[256 + tid] : 0.f;
    const float b2v = bk.gamma[tid & (C - 1)] * bk.b2[tid & (C - 1)];
    const uint2* twsrc = reinterpret_cast<const uint2*>(bk.par) + (NG * wave) * 64 + ln;
    frag4 tw[TW_R], twl[X2 ? TW_R : 1];
#pragma unroll
    for (int r = 0; r < TW_R; ++r) tw[r] = __builtin_bit_cast(frag4, twsrc[r * 512]);
    if (X2) {
#pragma unroll
      for (int r = 0; r < TW_R; ++r) twl[r] = __builtin_bit_cast(frag4, twsrc[TW_BYTES / 8 + r * 512]);
    }
    const float* pf = reinterpret_cast<const float*>(bk.par + (X2 ? 2 : 1) * TW_BYTES);
    float dwbias[NG];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) dwbias[gi] = pf[16 * (NG * wave + gi) + db];
    const float lnv = pf[C + (NT == 256 ? tid : tid & 255)];   // LN weight [128] | LN bias [128]
    SC_STAMP(2 + 5 * j);
    __syncthreads();   // planar image complete (input / previous MLP + zero pads); ring slots 0, 1 free
    b1s[tid] = b1v0;
    if (NT == 256) b1s[256 + tid] = b1v1;
    if (tid < C) b2s[tid] = b2v;
    if (NT == 256 || tid < 2 * C) lnws[tid] = lnv;

    // ---- pointwise filters: chunk = 32 hidden units = 16 pieces of 1 KiB, NPIECE = 4 (2: eight waves) per wave.
    //      pieces 0..7 : W1 rows (LDS row m <- hidden unit 32*ch + swap23(m)), 256-byte rows,
    //                    16-byte chunk c of row m at position c ^ (m & 15)
    //      pieces 8..15: gamma*W2 columns 32*ch .. +31 of the 128 channel rows, 64-byte rows,
    //                    chunk c of row r at position c ^ F[(r >> 2) & 3]
    const unsigned char* wsrc[NPIECE];
    const unsigned char* wsrcl[NPIECE];   // split mode: the same pieces of the remainder images, 8 KB further into the slot
#pragma unroll
    for (int i = 0; i < NPIECE; ++i) {
      const int pc = wave * NPIECE + i;
      if (pc < 8) {
        const int m = pc * 4 + (lane >> 4);
        const int hid = (m & ~12) | ((m & 4) << 1) | ((m & 8) >> 1);   // swap bits 2 and 3
        const size_t o = (size_t)hid * (C * 2) + (((lane & 15) ^ (m & 15)) << 4);
        wsrc[i] = bk.w1 + o;
        wsrcl[i] = X2 ? bk.w1_lo + o : nullptr;
      } else {
        const int r = (pc - 8) * 16 + (lane >> 2);
        const size_t o = (size_t)r * (HID * 2) + (((lane & 3) ^ swz4(r)) << 4);
        wsrc[i] = bk.w2g + o;
        wsrcl[i] = X2 ? bk.w2g_lo + o : nullptr;
      }
    }
    // chunk k adds 32 W1 rows (8192 B) resp. 32 W2 columns (64 B)
    const int wstep0 = w1wave ? 32 * C * 2 : 64;
    // (every workgroup walks the 16 chunks in the same order, so an alert's fc2 sum does not depend on where it sits
    //  in a batch or on G; a rotation by workgroup index, meant to keep the workgroups off the same L2 lines, measured
    //  nothing: DESIGN.md section 4a)
    // the first half of the waves loads the W1 half of chunk k into W1 slot k % 3, the second half the W2 half into
    // W2 slot k % 3: NPIECE consecutive pieces each
    auto issue = [&](int k) {
      unsigned char* dst = (w1wave ? w1slot(k % NSLOT) : w2slot(k % NSLOT)) + (wave & (NW / 2 - 1)) * (NPIECE * 1024);
#pragma unroll
      for (int i = 0; i < NPIECE; ++i)
        __builtin_amdgcn_global_load_lds((gptr_t)(wsrc[i] + (size_t)(k & (NCH - 1)) * wstep0),
                                         (lptr_t)(dst + i * 1024), 16, 0, 0);
      if (X2) {
#pragma unroll
        for (int i = 0; i < NPIECE; ++i)
          __builtin_amdgcn_global_load_lds((gptr_t)(wsrcl[i] + (size_t)(k & (NCH - 1)) * wstep0),
                                           (lptr_t)(dst + HALFB + i * 1024), 16, 0, 0);
      }
    };
    // one of the wave's pieces (the chunk loop spreads them over its MFMAs: four LDS-DMAs back to back held the wave
    // for 230-420 cycles at the vector-memory port, a fifth of a step)
    auto issue_piece = [&](int k, int i) {   // (split mode: pieces 4..7 are the remainders)
      unsigned char* dst = (w1wave ? w1slot(k % NSLOT) : w2slot(k % NSLOT)) + (wave & (NW / 2 - 1)) * (NPIECE * 1024);
      if (X2 && i >= 4)
        __builtin_amdgcn_global_load_lds((gptr_t)(wsrcl[i & 3] + (size_t)(k & (NCH - 1)) * wstep0),
                                         (lptr_t)(dst + HALFB + (i & 3) * 1024), 16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds((gptr_t)(wsrc[i] + (size_t)(k & (NCH - 1)) * wstep0),
                                         (lptr_t)(dst + i * 1024), 16, 0, 0);
    };
    SC_STAMP(3 + 5 * j);

    // ---- depthwise 7x7 on the matrix pipe.  Per channel (= block) and output tile (rows 4 yb + j, columns 4 xb + i):
    //        D[i][j] = sum over ky, rb, k of  W[ky][4 rb + k - i + 3] * in[4 yb + j + ky - 3][4 (xb + rb) + k]
    //      a row step s = 4 yb + ky serves both yb with that sum: 22 reads, 56 MFMAs per (channel group, alert)
    // padded rows of the planar image: rofs[s] = byte offset of input row s + j - 3 (row 7 = zeros when outside)
    int rofs[11];
#pragma unroll
    for (int sx = 0; sx < 11; ++sx) {
      const int r = sx + dj - 3;
      rofs[sx] = ((unsigned)r < (unsigned)HW ? r : 7) * PL_ROW;
    }
    float v[NG][G][16];   // [group][alert][yb * 8 + xb * 4 + i]
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
      if (gi == 1) {   // (four waves) the second group's taps into the same registers (their last use is behind us)
#pragma unroll
        for (int r = 0; r < TW_R; ++r) tw[r] = __builtin_bit_cast(frag4, twsrc[r * 512 + 64]);
        if (X2) {
#pragma unroll
          for (int r = 0; r < TW_R; ++r) twl[r] = __builtin_bit_cast(frag4, twsrc[TW_BYTES / 8 + r * 512 + 64]);
        }
      }
      // Both alerts of a row step together (8 to 16 products per step), the NEXT step's four reads requested in front of
      // them: read and used in the same step, each of a block's 44 steps began with an exposed LDS round trip.
      f32x4 acc[G][2][2];
#pragma unroll
      for (int al = 0; al < G; ++al)
#pragma unroll
        for (int yb = 0; yb < 2; ++yb)
#pragma unroll
          for (int xb = 0; xb < 2; ++xb) acc[al][yb][xb] = f32x4{dwbias[gi], dwbias[gi], dwbias[gi], dwbias[gi]};
      const unsigned char* lb = pl + (16 * (NG * wave + gi) + db) * 8;
      frag4 bq[2][G][2], bql[X2 ? 2 : 1][G][X2 ? 2 : 1];
      auto read_step = [&](int sx, int buf) {
#pragma unroll
        for (int al = 0; al < G; ++al)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            bq[buf][al][q] = __builtin_bit_cast(frag4, *reinterpret_cast<const uint2*>(lb + al * PL_AL + q * PL_XQ + rofs[sx]));
            if (X2)
              bql[buf][al][q] =
                  __builtin_bit_cast(frag4, *reinterpret_cast<const uint2*>(lb + PLB + al * PL_AL + q * PL_XQ + rofs[sx]));
          }
      };
      read_step(0, 0);
#ifdef S1_EXP_NODW
#pragma unroll 1
      for (int sx = 0; sx < 0; ++sx) {
#else
#pragma unroll
      for (int sx = 0; sx < 11; ++sx) {
#endif
        // (touching this step's fragments makes hipcc wait for them here, while they are the only LDS reads in flight)
#pragma unroll
        for (int al = 0; al < G; ++al)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            asm volatile("" : "+v"(bq[sx & 1][al][q]));
            if (X2) asm volatile("" : "+v"(bql[X2 ? sx & 1 : 0][al][X2 ? q : 0]));
          }
        if (sx + 1 < 11) read_step(sx + 1, (sx + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int al = 0; al < G; ++al)
#pragma unroll
          for (int yb = 0; yb < 2; ++yb) {
            const int ky = sx - 4 * yb;
            if (ky < 0 || ky > 6) continue;
#pragma unroll
            for (int rbi = 0; rbi < 3; ++rbi)
#pragma unroll
              for (int xb = 0; xb < 2; ++xb) {
                const int q = xb + rbi - 1;
                if (q < 0 || q > 1) continue;
                if (X2) {   // remainders first
                  acc[al][yb][xb] = Mfma<DT>::m4(twl[ky * 3 + rbi], bq[sx & 1][al][q], acc[al][yb][xb]);
                  acc[al][yb][xb] = Mfma<DT>::m4(tw[ky * 3 + rbi], bql[X2 ? sx & 1 : 0][al][X2 ? q : 0], acc[al][yb][xb]);
                }
                acc[al][yb][xb] = Mfma<DT>::m4(tw[ky * 3 + rbi], bq[sx & 1][al][q], acc[al][yb][xb]);
              }
          }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int al = 0; al < G; ++al)
#pragma unroll
        for (int yb = 0; yb < 2; ++yb)
#pragma unroll
          for (int xb = 0; xb < 2; ++xb)
#pragma unroll
            for (int i = 0; i < 4; ++i) v[gi][al][yb * 8 + xb * 4 + i] = acc[al][yb][xb][i];
    }
    if (KEEP && a.keep_d[j] != nullptr) {   // the depthwise output before the LayerNorm: lane = (channel of the group, row j of
                                             // the quad) (nullptr: the backward recomputes it, dwln_bwd.hip)
#pragma unroll
      for (int gi = 0; gi < NG; ++gi)
#pragma unroll
        for (int al = 0; al < G; ++al) {
          if (al >= nal) continue;
          float* dst = a.keep_d[j] + (size_t)(a0 + al) * PA * C + 16 * (NG * wave + gi) + db;
#pragma unroll
          for (int yb = 0; yb < 2; ++yb)
#pragma unroll
            for (int xb = 0; xb < 2; ++xb)
              if (yb < 1 || dj < 3) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  if (xb == 1 && i == 3) continue;
                  dst[((4 * yb + dj) * HW + 4 * xb + i) * C] = v[gi][al][yb * 8 + xb * 4 + i];
                }
              }
        }
    }
    SC_STAMP(4 + 5 * j);   // depthwise done
    // ---- the one transpose: the depthwise outputs (lane = channel, registers = pixels) as fp32 into the
    //      [pixel][channel] image, which overlays the planar image that other waves may still be reading
    __syncthreads();   // nobody reads the planar image any more
    {
      unsigned char* dst = smem + dj * (HW * LNP) + (16 * NG * wave + db) * 4;
#pragma unroll
      for (int gi = 0; gi < NG; ++gi)
#pragma unroll
        for (int al = 0; al < G; ++al)
#pragma unroll
          for (int yb = 0; yb < 2; ++yb)
#pragma unroll
            for (int xb = 0; xb < 2; ++xb)
              if (yb < 1 || dj < 3) {   // row 7 is padding
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  if (xb == 1 && i == 3) continue;   // column 7 is padding
                  const int col = 4 * xb + i, ofs = (al * PA + 4 * yb * HW + col) * LNP + gi * 64;
                  *reinterpret_cast<float*>(dst + ofs) = v[gi][al][yb * 8 + xb * 4 + i];
                }
              }
    }
    __syncthreads();   // fp32 image complete

    // ---- LayerNorm in registers -> fc1 -> GELU -> fc2 over 16 chunks, software-pipelined inside the wave: step ch issues
    //      chunk ch+1's fc1 MFMAs between the GELUs of chunk ch (one element per MFMA: ~7 VALU instructions pass while the matrix pipe
    //      works on a 32-cycle product), then chunk ch's fc2 MFMAs between the second half's GELUs.  Without this a
    //      wave runs LDS reads -> 8 dependent MFMAs -> 120 VALU -> 8 MFMAs strictly one after the other (2.9k cycles per
    //      chunk).  No pipe is saturated now (MFMA 20 % busy, LDS array 31 %, VALU active in 21 % of wave-cycles): a
    //      step is ~2k cycles of which ~0.5k are barrier, fragment-read issue and LDS-DMA issue.  fc2 accumulates into x
    //      (gamma is in the filter).
    {
      // this lane's pixel, 64 of its 128 channels in fc1's k order (k-step ks: channels 16 ks + 8 h + 0..7); the partner
      // lane ^ 32 holds the other 64: two-pass statistics as ln_regs(); the normalised value is rounded once to the operand
      // type (split mode: its f16 remainder from the same fp32 value).  (LDS words are read as 16-bit vectors while an
      // LDS-DMA may be in flight, see bias_acc.)
      auto lds4 = [](const void* q) { return __builtin_bit_cast(f32x4, *reinterpret_cast<const bf16x8*>(q)); };
      frag xf[KS1], xfl[X2 ? KS1 : 1];
      float xv[64];
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 r4 = lds4(smem + lnrow + ks * 64 + q * 16);
#pragma unroll
          for (int e = 0; e < 4; ++e) xv[ks * 8 + q * 4 + e] = r4[e];
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this lane's row is in registers
      __builtin_amdgcn_s_barrier();   // ... everyone's: the image's bytes may take the rings' other slots
      issue(0);
      issue(1);
      if (w1wave) issue(2);
      float s = 0.f;
#pragma unroll
      for (int n = 0; n < 64; ++n) s += xv[n];
      s += __shfl_xor(s, 32, 64);
      const float mean = s * (1.0f / C);
      float q2 = 0.f;
#pragma unroll
      for (int n = 0; n < 64; ++n) {
        xv[n] -= mean;
        q2 += xv[n] * xv[n];
      }
      q2 += __shfl_xor(q2, 32, 64);
      const float rstd = rsqrtf(q2 * (1.0f / C) + LN_EPS);
#pragma unroll
      for (int ks = 0; ks < KS1; ++ks) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const f32x4 w4 = lds4(lnws + ks * 16 + h * 8 + q * 4), b4 = lds4(lnbs + ks * 16 + h * 8 + q * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float y = xv[ks * 8 + q * 4 + e] * rstd * w4[e] + b4[e];
            const T yh = (T)y;
            xf[ks][q * 4 + e] = yh;
            if (X2) xfl[X2 ? ks : 0][q * 4 + e] = (T)(y - (float)yh);
          }
        }
        if (KEEP && live)   // the LayerNorm output for the backward: this lane's 16-byte piece of the pixel's row
          *reinterpret_cast<frag*>(reinterpret_cast<unsigned char*>(a.keep_xn[j]) + ((size_t)a0 * PA + p) * C * 2 + ks * 32 +
                                   h * 16) = xf[ks];
      }
      SC_STAMP(5 + 5 * j);   // LN done: every B operand of the MLP is in registers
      // the residual, requested behind the filter requests in this wave's VM order (its 64 registers next to the row's 64
      // spill) and not touched before the prologue has waited for all of them: first used by step 0's fc2
      float4 xt[4 * CT];
      __builtin_amdgcn_sched_barrier(0);
      {
        const float* src = j == 0 ? xsrc : xscr;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) xt[4 * ct + qd] = *reinterpret_cast<const float4*>(src + ct * 32 + 8 * qd + 4 * h);
      }
      __builtin_amdgcn_sched_barrier(0);
      // fc1 bias of chunk k into an accumulator: row (r&3) + 8(r>>2) + 4h holds hidden unit
      // 32k + (r&3) + 4((r>>2)&1) + 8h + 16(r>>3).  (Read as 16-bit vectors like the filter fragments: behind an LDS
      // read of float type hipcc waits vmcnt(0) while an LDS-DMA is in flight -- its type-based alias test takes the
      // DMA for a possible writer of those words -- and the chunks this ring keeps ahead are drained.)
      auto bias_acc = [&](int k, f32x16& acc) {
        const float* bp = b1s + (k & (NCH - 1)) * 32 + 8 * h;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const f32x4 bv = __builtin_bit_cast(f32x4, *reinterpret_cast<const bf16x8*>(bp + 4 * (qd & 1) + 16 * (qd >> 1)));
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[4 * qd + e] = bv[e];
        }
      };
      frag a1l[X2 ? KS1 : 1];   // split mode: the W1 fragments' remainders, read with their heads
      auto read_a1 = [&](int k, frag (&a1)[KS1]) {
        const unsigned char* w1s = w1slot(k % NSLOT);
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
          a1[ks] = *reinterpret_cast<const frag*>(w1s + lr * 256 + (((ks * 2 + h) ^ (lr & 15)) << 4));
          if (X2) a1l[ks] = *reinterpret_cast<const frag*>(w1s + HALFB + lr * 256 + (((ks * 2 + h) ^ (lr & 15)) << 4));
        }
      };
#ifdef S1_LOOPSTAMP
      unsigned long long lts[16];
#define LS(i) do { __builtin_amdgcn_sched_barrier(0); if (ch == 6 || ch == 7) lts[i + 8 * (ch - 6)] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define LS(i)
#endif
      // Register pipeline: entering step ch the wave holds hc = fc1 of chunk ch, hn = the fc1 bias of chunk ch + 1 and
      // a1 = the W1 fragments of chunk ch + 1 (both requested in the middle of step ch - 1, so their LDS latency --
      // 400+ cycles when eight waves read 20 KB each -- is not in anybody's way).
      f32x16 hacc[2];
      frag a1[KS1];
      {   // prologue: chunk 0's fc1, then the operands of step 0
        // VM order of a wave: W1 waves W1(0), W1(1), W1(2), 16 loads of x; W2 waves W2(0), W2(1), x: chunk 0 has landed
        // once no more than W2(1) + x are out.  A group W(k) is the wave's NPIECE requests (4 on four waves, 2 on
        // eight; split mode: twice that, heads and remainders), so the count is NPIECE + 16 = 20 / 18 / split 24.
        // (Whatever else the wave issues behind chunk 0 -- the keeping forms' 8
        // keep_xn stores, a spill store of hipcc's -- counts in vmcnt on gfx9 as well and is younger than chunk 0, so it
        // only makes this wait stricter: the count is an upper bound and must not be tightened to the loads listed here.)
        wait_vm<(X2 ? 2 : 1) * NPIECE + 16>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        bias_acc(0, hacc[0]);
        read_a1(0, a1);
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
          if (X2) {
            hacc[0] = Mfma<T>::m32(a1l[ks], xf[ks], hacc[0]);
            hacc[0] = Mfma<T>::m32(a1[ks], xfl[ks], hacc[0]);
          }
          hacc[0] = Mfma<T>::m32(a1[ks], xf[ks], hacc[0]);
        }
        __builtin_amdgcn_sched_barrier(0);
        wait_vm<0>();   // W1(1), W1(2) / W2(1), x
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // ... for everyone, and chunk 0's W1 slot is read out
        bias_acc(1, hacc[1]);
        read_a1(1, a1);
        // x = residual + gamma*b2 (its first use in front of the next request: behind it hipcc's own wait for the
        // residual would drain that request too)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) {
            const f32x4 bv = lds4(b2s + ct * 32 + 8 * qd + 4 * h);
            const float4 v4 = xt[4 * ct + qd];
            x[ct][4 * qd + 0] = (live ? v4.x : 0.f) + bv[0];
            x[ct][4 * qd + 1] = (live ? v4.y : 0.f) + bv[1];
            x[ct][4 * qd + 2] = (live ? v4.z : 0.f) + bv[2];
            x[ct][4 * qd + 3] = (live ? v4.w : 0.f) + bv[3];
          }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) asm volatile("" : "+v"(x[ct]));
        __builtin_amdgcn_sched_barrier(0);
        if (w1wave) issue(3);
      }
      // one step: hc = fc1 of chunk ch (complete), hn = bias of chunk ch + 1 <- fc1 of chunk ch + 1; hc <- bias of ch + 2
      auto step = [&](auto last_c, int ch, f32x16& hc, f32x16& hn) {
        constexpr bool LAST = decltype(last_c)::value;
        LS(0);
        // VM order of a wave: W1 waves W1(0..ch+3), W2 waves W2(0..ch+1), each group in piece order (step ch - 1 issued
        // its kdma group's pieces one by one, nothing else); both need all but their youngest group of NPIECE (x 2: split)
        wait_vm<(X2 ? 2 : 1) * NPIECE>();
        LS(1);
        // raw barrier: __syncthreads() would also wait vmcnt(0) while an LDS-DMA is in flight
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every LDS read of the last step is home
#ifndef S1_EXP_NOBAR
        __builtin_amdgcn_s_barrier();   // W1(ch+2), W2(ch) have landed for everyone; W1(ch+1), W2(ch-1) are read out
#endif
        LS(2);
        frag a2[CT][2], a2l[X2 ? CT : 1][2];
        const unsigned char* w2s = w2slot(ch % NSLOT);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const int r = ct * 32 + lr;
            a2[ct][s2] = *reinterpret_cast<const frag*>(w2s + r * 64 + (((s2 * 2 + h) ^ swz4(r)) << 4));
            if (X2) a2l[ct][s2] = *reinterpret_cast<const frag*>(w2s + HALFB + r * 64 + (((s2 * 2 + h) ^ swz4(r)) << 4));
          }
        LS(3);
        const int kdma = ch + (w1wave ? 4 : 2);   // (indices past the last chunk wrap: harmless reloads into dead slots)
        __builtin_amdgcn_sched_barrier(0);
        LS(4);
        float g[16];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          if (!LAST) {
            if (X2) {
              hn = Mfma<T>::m32(a1l[r], xf[r], hn);
              hn = Mfma<T>::m32(a1[r], xfl[r], hn);
            }
            hn = Mfma<T>::m32(a1[r], xf[r], hn);
          }
#ifdef S1_EXP_NOGELU
          g[r] = hc[r];
#else
          g[r] = gelu_for<T>(hc[r]);
#endif
#ifndef S1_EXP_NODMA
          if (X2) issue_piece(kdma, r);
          else if (r % (8 / NPIECE) == 8 / NPIECE - 1) issue_piece(kdma, r / (8 / NPIECE));   // r = 1, 3, 5, 7 / 3, 7
#endif
          __builtin_amdgcn_sched_barrier(0);
        }
        LS(5);
        if (!LAST) read_a1(ch + 2, a1);
        frag hf, hfl;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          hf[r] = (T)g[r];
          if (X2) hfl[r] = (T)(g[r] - (float)hf[r]);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          if (X2) {
            x[ct] = Mfma<T>::m32(a2l[ct][0], hf, x[ct]);
            x[ct] = Mfma<T>::m32(a2[ct][0], hfl, x[ct]);
          }
          x[ct] = Mfma<T>::m32(a2[ct][0], hf, x[ct]);
#ifdef S1_EXP_NOGELU
          g[8 + 2 * ct] = hc[8 + 2 * ct];
          g[9 + 2 * ct] = hc[9 + 2 * ct];
#else
          g[8 + 2 * ct] = gelu_for<T>(hc[8 + 2 * ct]);
          g[9 + 2 * ct] = gelu_for<T>(hc[9 + 2 * ct]);
#endif
          __builtin_amdgcn_sched_barrier(0);
        }
        if (!LAST) bias_acc(ch + 2, hc);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          hf[r] = (T)g[8 + r];
          if (X2) hfl[r] = (T)(g[8 + r] - (float)hf[r]);
        }
        LS(6);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          if (X2) {
            x[ct] = Mfma<T>::m32(a2l[ct][1], hf, x[ct]);
            x[ct] = Mfma<T>::m32(a2[ct][1], hfl, x[ct]);
          }
          x[ct] = Mfma<T>::m32(a2[ct][1], hf, x[ct]);
        }
        LS(7);
      };
#ifndef S1_EXP_NOLOOP
#pragma unroll 1
      for (int ch = 0; ch < NCH - 2; ch += 2) {
        step(std::false_type{}, ch, hacc[0], hacc[1]);
        step(std::false_type{}, ch + 1, hacc[1], hacc[0]);
      }
      step(std::false_type{}, NCH - 2, hacc[0], hacc[1]);
      step(std::true_type{}, NCH - 1, hacc[1], hacc[0]);
#endif
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the last prefetches (unused) are not left in flight
#ifdef S1_LOOPSTAMP
      if (a.wgt != nullptr && blockIdx.x == 0 && tid == 0 && j == 0)
        for (int i = 0; i < 16; ++i) a.wgt[4096 + i] = lts[i];
#endif
      wait_vm<0>();   // the wrapped reloads: nothing may land in the ring once its bytes are reused
      if (j == 0) {      // next block's depthwise operand; chunk 15 (W1 slot 0 = the planar image's first 8 KB) must be read out first
        __syncthreads();
        zero_pads();
        if (inmap) regs_to_planar<DT, G, PLO, KEEP && !std::is_same<T, f16_t>::value>(x, pl, p, h);
        if (live) {
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd)
              *reinterpret_cast<float4*>(xscr + ct * 32 + 8 * qd + 4 * h) =
                  make_float4(x[ct][4 * qd], x[ct][4 * qd + 1], x[ct][4 * qd + 2], x[ct][4 * qd + 3]);
        }
      }
    }
    SC_STAMP(6 + 5 * j);   // MLP done
  }
  if (a.tap_stage != nullptr && live) {
    float* tp = a.tap_stage + ((size_t)a0 * PA + p) * C;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd)
        *reinterpret_cast<float4*>(tp + ct * 32 + 8 * qd + 4 * h) =
            make_float4(x[ct][4 * qd], x[ct][4 * qd + 1], x[ct][4 * qd + 2], x[ct][4 * qd + 3]);
  }

  // ---- downsample: LN + conv 2x2 s2 (128 -> 256): 9 G output pixels x 256 channels, K = 512
  {
    __syncthreads();   // every wave is out of the MLP: the ring and planar bytes from 0 take the LN image
    // this wave's output tiles wave, wave + 4 (32 channels each; eight waves: tile wave alone) x 32 k-steps: 64 (32)
    // filter fragments packed as MFMA A operands (1 KiB each, launch_pack_frag32), a ring of 16 in flight; a fragment
    // serves every 32-column block of output pixels (eight waves: 45 pixels on two), so the workgroup loads it once
    constexpr int KSD = 4 * C / 16, RING = X2 ? 8 : 16, NSTEP = NG * KSD, NCB = L::NCB;
    // (split: a packed fragment is 2 KiB, the heads' 1 KiB then the remainders')
    const frag* wsrc = reinterpret_cast<const frag*>(a.ds_w) + lane;
    auto fsrc = [&](int stp) {
      return wsrc + (size_t)((wave + NW * (stp >> 5)) * KSD + (stp & (KSD - 1))) * (X2 ? 128 : 64);
    };
    // the ring's first round is requested in front of the LayerNorm, whose weights are words of LDS: its L2 latency
    // passes under the arithmetic, and nothing below waits for a vector-memory load before the first product
    frag wq[RING], wql[X2 ? RING : 1];
#pragma unroll
    for (int i = 0; i < RING; ++i) {
      wq[i] = *fsrc(i);
      if (X2) wql[i] = fsrc(i)[64];
    }
    __builtin_amdgcn_sched_barrier(0);
    // (in place: x is dead behind it, and a second set of 64 registers beside the ring's 64 spills in the f16 forms.
    //  Every column block goes to the map as soon as it is normalised.  The pixel slots beyond the image store too, into
    //  the rows behind the map -- dead bytes in front of the bias words -- which spares the phase four branches; not in
    //  the split form, where those rows are the first of the remainder image.)
    static_assert(NW * 32 * PITCH <= L::OFF_B1, "the rows of the slots beyond the image lie in dead bytes");
    ln_regs<true>(x, dscs, dscs + C, h, x, [&](int ct) {
      if (X2 && !inmap) return;
      regs_to_map_ct<T, X2 ? MAPB : 0>(x, stg, p, h, ct);   // (split: the remainder image behind it, dead bytes too)
    });
    // raw barrier: the map is complete once everybody's LDS stores are; __syncthreads() would wait for the ring as well
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (KEEP) {   // the downsample's patch rows [output pixel][q = 2 ky + kx][128] = LayerNorm'd pixels (2 oy + ky, 2 ox + kx)
      unsigned char* dst = reinterpret_cast<unsigned char*>(a.keep_patches) + (size_t)a0 * PO * 4 * C * 2;
      for (int i = tid; i < nal * PO * 4 * 16; i += NT) {
        const int c16 = i & 15, q = (i >> 4) & 3, o2 = i >> 6;
        const int g2 = o2 / PO, oo2 = o2 - g2 * PO;
        const int pin2 = g2 * PA + (2 * (oo2 / 3) + (q >> 1)) * HW + 2 * (oo2 % 3) + (q & 1);
        *reinterpret_cast<uint4*>(dst + (size_t)(o2 * 4 + q) * C * 2 + 16 * c16) =
            *reinterpret_cast<const uint4*>(stg + pin2 * PITCH + 16 * c16);
      }
    }
    SC_STAMP(12);
    // output pixel slots o = 32 cb + lr: 18 of 32 / 45 of 64 used; bsrc = this lane's half of the input pixel under tap 0
    const unsigned char* bsrc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int o = cb * 32 + lr, oc = o < G * PO ? o : 0;
      const int g = oc / PO, oo = oc - g * PO;
      const int oy = oo / 3, ox = oo - oy * 3;
      bsrc[cb] = stg + (g * PA + 2 * oy * HW + 2 * ox) * PITCH + h * 16;
    }
    f32x16 acc[NCB];
    constexpr int RPT = KSD / RING, NRD = NSTEP / RING;   // ring rounds per output tile, rounds in all
    static_assert(RING % 8 == 0 && KSD % RING == 0, "a round stays inside a tile and starts at a tap's first k-step");
    // B fragments of step stp (k-step ks of its tile: tap q = ks >> 3 = (ky*2 + kx), 8 k-steps of 16 channels each), read
    // two steps ahead of their products into four rotating register sets (RING is a multiple of 4: the rotation carries
    // over the rounds): read and used in the same step, every product waited for an LDS round trip (stage2p.hip, part 4)
    frag bq[4][NCB], bql[X2 ? 4 : 1][X2 ? NCB : 1];
    auto read_b = [&](int stp, int set) {
      const int ks = stp & (KSD - 1), q = ks >> 3;
      const int ofs = ((q >> 1) * HW + (q & 1)) * PITCH + (ks & 7) * 32;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        bq[set][cb] = *reinterpret_cast<const frag*>(bsrc[cb] + ofs);
        if (X2) bql[X2 ? set : 0][X2 ? cb : 0] = *reinterpret_cast<const frag*>(bsrc[cb] + MAPB + ofs);
      }
    };
    // one ring round: RING k-steps of tile cot.  The refills are unconditional; the last round (LAST) has none and reads
    // no fragment past the end.  The tile's bias is a word of LDS: no wait for vector memory but hipcc's counted ones for wq.
    auto round = [&](auto last_c, int rd) {
      constexpr bool LAST = decltype(last_c)::value;
      const int cot = wave + NW * (rd / RPT);
      if (rd % RPT == 0) {
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const f32x4 bv = lds_f32x4(dscs + 2 * C + cot * 32 + 8 * qd + 4 * h);
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[cb][4 * qd + e] = bv[e];
        }
      }
#pragma unroll
      for (int i = 0; i < RING; ++i) {
        const int stp = rd * RING + i;
        // (touching this step's fragments makes hipcc wait for them here, in front of the next request)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          asm volatile("" : "+v"(bq[i & 3][cb]));
          if (X2) asm volatile("" : "+v"(bql[X2 ? i & 3 : 0][X2 ? cb : 0]));
        }
        if (!LAST || i + 2 < RING) read_b(stp + 2, (i + 2) & 3);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          if (X2) {
            acc[cb] = Mfma<T>::m32(wql[i], bq[i & 3][cb], acc[cb]);
            acc[cb] = Mfma<T>::m32(wq[i], bql[X2 ? i & 3 : 0][X2 ? cb : 0], acc[cb]);
          }
          acc[cb] = Mfma<T>::m32(wq[i], bq[i & 3][cb], acc[cb]);
        }
        if (!LAST) {
          wq[i] = *fsrc(stp + RING);
          if (X2) wql[i] = fsrc(stp + RING)[64];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (rd % RPT == RPT - 1) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const int o = cb * 32 + lr;
          if (o >= nal * PO) continue;
          float* dst = a.out + ((size_t)a0 * PO + o) * CN + cot * 32 + 4 * h;
#pragma unroll
          for (int qd = 0; qd < 4; ++qd)
            *reinterpret_cast<float4*>(dst + 8 * qd) =
                make_float4(acc[cb][4 * qd], acc[cb][4 * qd + 1], acc[cb][4 * qd + 2], acc[cb][4 * qd + 3]);
        }
      }
    };
#ifndef S1_EXP_NODS
    read_b(0, 0);
    read_b(1, 1);
#pragma unroll 1
    for (int rd = 0; rd < NRD - 1; ++rd) round(std::false_type{}, rd);
    round(std::true_type{}, NRD - 1);
#endif
    SC_STAMP(13);
  }
}

// one block's parameter image (layout at TW_R above); taps: tap-major [49][128] fp32
template <typename T, bool X2>
__global__ void pack_s1par_kernel(const float* __restrict__ taps, const float* __restrict__ dw_b,
                                  const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                  unsigned char* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int NTW = TW_R * C * 16;
  if (idx < NTW) {
    const int k = idx & 3, i = (idx >> 2) & 3, c = (idx >> 4) & (C - 1), r = idx / (16 * C);
    const int ky = r / 3, rb = r % 3 - 1, kx = 4 * rb + k - i + 3;
    const float w = (kx >= 0 && kx < 7) ? taps[(ky * 7 + kx) * C + c] : 0.f;
    const T wh = (T)w;
    reinterpret_cast<T*>(out)[idx] = wh;
    if (X2) reinterpret_cast<T*>(out)[NTW + idx] = (T)(w - (float)wh);
    return;
  }
  const int f = idx - NTW;
  if (f >= 3 * C) return;
  float v;
  if (f < C) v = dw_b[f];
  else if (f < 2 * C) v = ln_w[f - C];
  else v = ln_b[f - 2 * C];
  reinterpret_cast<float*>(out + (X2 ? 2 : 1) * TW_BYTES)[f] = v;
}

// fp32 downsample filter [Cout][Cin][2][2] -> 32x32x16 A fragments [row tile][k-step][lane][8], lane l holds row
// (l & 31), k = 16 s + 8 (l >> 5) + j of its tile, k = (2 ky + kx) * Cin + c
template <typename T, bool X2 = false>
__global__ void pack_frag32_kernel(const float* __restrict__ w, T* __restrict__ out, int rows, int cin) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int K = 4 * cin;
  if (i >= (long)rows * K) return;
  const int j = (int)(i & 7), l = (int)((i >> 3) & 63);
  const long fs = i >> 9;
  const int ksteps = K / 16;
  const int sk = (int)(fs % ksteps), tile = (int)(fs / ksteps);
  const int row = 32 * tile + (l & 31), k = 16 * sk + 8 * (l >> 5) + j;
  const int q = k / cin, c = k - q * cin;
  const float v = w[((long)row * cin + c) * 4 + q];
  const T vh = (T)v;
  if (X2) {   // 2 KiB per fragment: [lane][8] heads, then [lane][8] remainders
    out[fs * 1024 + l * 8 + j] = vh;
    out[fs * 1024 + 512 + l * 8 + j] = (T)(v - (float)vh);
  } else {
    out[i] = vh;
  }
}

template <typename T, bool X2 = false, int WPS = 2, bool KEEP = false, int G = 2>
int launch_stage1b_t(const Stage1Args& a, hipStream_t st) {
  auto kern = stage1b_kernel<T, X2, WPS, KEEP, G>;
  using L = S1L<G, X2>;
  static DevOnce attr_set;
  // (BTSBOT_AMD_S1_ONE_WG=1: the same probe as stage0b.hip's; the forms that hold a CU alone have nothing to pad)
  static const int pad = switch_on(SW_S1_ONE_WG) && !X2 && G == 2 ? 90 * 1024 - L::LDS_BYTES : 0;
  const int LDS_BYTES = L::LDS_BYTES + pad;
  if (attr_set.need()) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
    attr_set.done();
  }
  hipLaunchKernelGGL(kern, dim3((a.B + G - 1) / G), dim3(L::NT), LDS_BYTES, st, a);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

}  // namespace

#ifdef STAGE1B_X2_TU
// ---- this translation unit (stage1x.hip) holds only the split-operand instantiations (see stage0b.hip)
int launch_stage1b_x2(const Stage1Args& a, hipStream_t st) {
  // (one workgroup per CU -- two planar images, doubled ring slots: 143 KB of LDS -- with 512 registers)
  if (a.blk[0].w1_lo == nullptr || a.blk[0].w2g_lo == nullptr || a.blk[1].w1_lo == nullptr || a.blk[1].w2g_lo == nullptr) {
    btsbot_set_error("stage1b: the split mode needs the filters' remainder images (w1_lo, w2g_lo)");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return launch_stage1b_t<f16_t, true, 1>(a, st);
}
int launch_pack_s1par_x2(const float* taps, const float* dw_b, const float* ln_w, const float* ln_b, void* out,
                         hipStream_t st) {
  const dim3 grid((TW_R * C * 16 + 3 * C + 255) / 256), blk(256);
  hipLaunchKernelGGL((pack_s1par_kernel<f16_t, true>), grid, blk, 0, st, taps, dw_b, ln_w, ln_b,
                     reinterpret_cast<unsigned char*>(out));
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
int launch_pack_frag32_x2(const float* src, void* dst, int cout, int cin, hipStream_t st) {
  const long total = (long)cout * 4 * cin;
  hipLaunchKernelGGL((pack_frag32_kernel<f16_t, true>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src,
                     reinterpret_cast<f16_t*>(dst), cout, cin);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
#else
int launch_stage1b_x2(const Stage1Args& a, hipStream_t st);
int launch_pack_s1par_x2(const float* taps, const float* dw_b, const float* ln_w, const float* ln_b, void* out,
                         hipStream_t st);
int launch_pack_frag32_x2(const float* src, void* dst, int cout, int cin, hipStream_t st);

size_t s1par_bytes() { return PARB_X2; }   // (the split mode's image is the larger one)

int launch_pack_s1par(int prec, const float* taps, const float* dw_b, const float* ln_w,
                      const float* ln_b, void* out, hipStream_t st) {
  unsigned char* o = reinterpret_cast<unsigned char*>(out);
  const dim3 grid((TW_R * C * 16 + 3 * C + 255) / 256), blk(256);
  if (prec == BTSBOT_BF16)
    hipLaunchKernelGGL((pack_s1par_kernel<bf16_t, false>), grid, blk, 0, st, taps, dw_b, ln_w, ln_b, o);
  else if (prec == BTSBOT_F16)
    hipLaunchKernelGGL((pack_s1par_kernel<f16_t, false>), grid, blk, 0, st, taps, dw_b, ln_w, ln_b, o);
  else if (prec == BTSBOT_F16X2)
    return launch_pack_s1par_x2(taps, dw_b, ln_w, ln_b, out, st);
  else {
    btsbot_set_error("pack_s1par: precision %d is not a 16-bit mode", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

// downsample filter [Cout][Cin][2][2] fp32 -> 32x32x16 MFMA A fragments (stage1b.hip's / stage0b.hip's last phase)
int launch_pack_frag32(int prec, const float* src, void* dst, int cout, int cin, hipStream_t st) {
  const long total = (long)cout * 4 * cin;
  const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
  if (prec == BTSBOT_BF16)
    hipLaunchKernelGGL(pack_frag32_kernel<bf16_t>, grid, blk, 0, st, src, reinterpret_cast<bf16_t*>(dst), cout, cin);
  else if (prec == BTSBOT_F16)
    hipLaunchKernelGGL(pack_frag32_kernel<f16_t>, grid, blk, 0, st, src, reinterpret_cast<f16_t*>(dst), cout, cin);
  else if (prec == BTSBOT_F16X2)
    return launch_pack_frag32_x2(src, dst, cout, cin, st);
  else {
    btsbot_set_error("pack_frag32: precision %d is not a 16-bit mode", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

bool stage1_supported(int prec, int c1, int c2) {
  return (prec == BTSBOT_BF16 || prec == BTSBOT_F16 || prec == BTSBOT_F16X2) && c1 == 128 && c2 == 256;
}

// Needs Stage0Blk::par (launch_pack_s1par), ::w1 (plain [512][128]) and Stage0Blk::w2g (gamma-scaled [128][512]), 16-bit,
// and Stage1Args::ds_w as MFMA fragments (launch_pack_frag32).
int launch_stage1b(int prec, const Stage1Args& a, bool g5, hipStream_t st) {
  if (a.B <= 0) return BTSBOT_OK;
  if (a.keep_xn[0] != nullptr) {   // the training forward
    if ((a.keep_d[0] == nullptr) != (a.keep_d[1] == nullptr) || a.keep_xn[1] == nullptr || a.keep_patches == nullptr ||
        a.tap_stage == nullptr || a.scratch == nullptr) {
      btsbot_set_error("stage1b: the training forward needs every kept buffer");
      return BTSBOT_ERR_INVALID_ARG;
    }
    if (prec == BTSBOT_BF16) return launch_stage1b_t<bf16_t, false, 2, true>(a, st);
    if (prec == BTSBOT_F16) return launch_stage1b_t<f16_t, false, 2, true>(a, st);
    btsbot_set_error("stage1b: the training forward runs in the bf16 / f16 modes, not %d", prec);
    return BTSBOT_ERR_INVALID_ARG;
  }
  // inference: five alerts per workgroup where the schedule asks for it (Schedule::s1_g5: other forwards in flight),
  // else two; the same bits either way
  if (g5) {
    if (prec == BTSBOT_BF16) return launch_stage1b_t<bf16_t, false, 2, false, 5>(a, st);
    if (prec == BTSBOT_F16) return launch_stage1b_t<f16_t, false, 2, false, 5>(a, st);
  }
  if (prec == BTSBOT_BF16) return launch_stage1b_t<bf16_t>(a, st);
  if (prec == BTSBOT_F16) return launch_stage1b_t<f16_t>(a, st);
  if (prec == BTSBOT_F16X2) return launch_stage1b_x2(a, st);
  btsbot_set_error("stage1b: unsupported precision %d", prec);
  return BTSBOT_ERR_INVALID_ARG;
}
#endif
