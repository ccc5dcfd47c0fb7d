// btsbot_decode_stamps: the step in front of btsbot_prep_triplets -- `stampData` of an alert packet (gzip of a
// single-HDU FITS image) -> the raw [n][63][63] float32 / shapes [n][2] pair, for a whole batch in one launch.
// What is accepted, and every bound, is inflate_core.h; this file is the mapping onto the machine.
//
// One stamp per lane.  Huffman decoding is serial per stream, so the parallelism is across stamps: a wave decodes SPW
// stamps at once, each lane with its own bit reader, its own canonical-code tables (1020 bytes, in LDS) and its own
// output.  The outputs of a wave's lanes are interleaved word by word in the global workspace (byte i of lane l at
// word (i / 4) * SPW + l): stamps of one batch are alike, so lanes write neighbouring words while they keep pace, and
// the conversion pass below reads a pixel of all SPW stamps as one row.  A wave is a workgroup; a workgroup owns one
// slot of SPW * STAMP_CAP bytes of workspace and walks the groups of SPW stamps blockIdx.x, + gridDim.x, ...
//
// SPW = 8, measured (tools/stamp_decode_bench.py, 24,576 stamps): noise-like stamps decode equally fast at 8 and 16
// stamps per wave (30.5 / 29.8 ms) and slower at 4 (48) and 32, 64 (39, 44: too few waves); smooth stamps -- long
// matches, whose copies read what the lane has just written -- take 32 ms at 8 and 49 ms at 16.  The decode is bound
// by the latency of its own dependent instruction chain (one bit per trip of decode()'s loop, about 1.4 us per symbol
// and lane), not by memory: the time barely moves between 3,072 and 24,576 stamps, so the launch scales with the batch
// until MAX_SLOTS stamps are in flight.
//
// The conversion -- big-endian to native, scatter into the 63 x 63 frame, zero fill -- is cooperative: per tile of 64
// frame positions the decoding lanes gather their stamps' words into an LDS tile (rows = positions, one word per
// stamp), and then all 64 lanes write 64 consecutive floats of one stamp after the other.  A stamp with a non-zero
// status has shape (0, 0) there: all zeros.
#include "common.h"
#include "inflate_core.h"

namespace {

using namespace stamp_core;

static_assert(STAMP_CAP == BTSBOT_STAMP_CAP && (int)ST_BAD_GZIP == (int)BTSBOT_STAMP_BAD_GZIP &&
              (int)ST_BAD_DEFLATE == (int)BTSBOT_STAMP_BAD_DEFLATE && (int)ST_TOO_LARGE == (int)BTSBOT_STAMP_TOO_LARGE &&
              (int)ST_BAD_TRAILER == (int)BTSBOT_STAMP_BAD_TRAILER && (int)ST_BAD_FITS == (int)BTSBOT_STAMP_BAD_FITS &&
              (int)ST_UNSUPPORTED == (int)BTSBOT_STAMP_UNSUPPORTED, "inflate_core.h and btsbot_hip.h name the same codes");
constexpr int PLANE = STAMP_SIDE * STAMP_SIDE;
// stamps per wave, and stamps in flight: the workspace stops growing at MAX_SLOTS * 28,800 B (build-time, for A/B runs)
#ifndef BTSBOT_DECODE_SPW
#define BTSBOT_DECODE_SPW 8
#endif
#ifndef BTSBOT_DECODE_MAX_SLOTS
#define BTSBOT_DECODE_MAX_SLOTS 32768
#endif
constexpr int STAMPS_PER_WAVE = BTSBOT_DECODE_SPW, MAX_SLOTS = BTSBOT_DECODE_MAX_SLOTS;
static_assert(64 % STAMPS_PER_WAVE == 0 && MAX_SLOTS % 64 == 0, "whole waves, whole slots");

template <int SPW>
struct Interleaved {   // lane l's output inside its wave's slot; p already points at the lane's first word
  uint8_t* p;
  __device__ __forceinline__ uint32_t at(uint32_t i) const { return (i >> 2) * (uint32_t)(SPW * 4) + (i & 3u); }
  __device__ __forceinline__ uint8_t get(uint32_t i) const { return p[at(i)]; }
  __device__ __forceinline__ void put(uint32_t i, uint8_t v) const { p[at(i)] = v; }
};

template <int SPW>
__global__ __launch_bounds__(64) void decode_stamps_kernel(const uint8_t* __restrict__ blob,
                                                           const int64_t* __restrict__ offsets, int n,
                                                           float* __restrict__ raw, int32_t* __restrict__ shapes,
                                                           uint8_t* __restrict__ status, uint8_t* __restrict__ ws) {
  constexpr int TILE_LD = SPW + 1;
  constexpr size_t TAB_BYTES = sizeof(Tables) * SPW, TILE_BYTES = sizeof(uint32_t) * 64 * TILE_LD;
  // the tables while the lanes decode, the transpose tile afterwards
  __shared__ __align__(16) uint8_t smem[TAB_BYTES > TILE_BYTES ? TAB_BYTES : TILE_BYTES];
  __shared__ int s_h[SPW], s_w[SPW], s_word0[SPW];
  Tables* tabs = reinterpret_cast<Tables*>(smem);
  uint32_t* tile = reinterpret_cast<uint32_t*>(smem);
  const int lane = threadIdx.x;
  uint8_t* slot = ws + (size_t)blockIdx.x * SPW * STAMP_CAP;
  const uint32_t* slot_w = reinterpret_cast<const uint32_t*>(slot);
  const long groups = ((long)n + SPW - 1) / SPW;

  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long s = g * SPW + lane;
    if (lane < SPW) {
      int h = 0, w = 0;
      uint32_t data_off = 0;
      if (s < n) {
        const int64_t begin = offsets[s], len = offsets[s + 1] - begin;
        const Interleaved<SPW> out{slot + lane * 4};
        int st = ST_BAD_GZIP;   // (a negative length)
        if (len >= 0) {
          uint32_t outn;
          st = gunzip(blob + begin, len, out, outn, tabs[lane]);
          if (st == ST_OK) st = parse_fits(out, outn, h, w, data_off);
        }
        if (st != ST_OK) h = w = 0;
        status[s] = (uint8_t)st;
        shapes[2 * s] = h;
        shapes[2 * s + 1] = w;
      }
      s_h[lane] = h;
      s_w[lane] = w;
      s_word0[lane] = (int)(data_off >> 2);   // a multiple of 2880: word aligned
    }
    __syncthreads();   // the tables are done with; the outputs are written
    for (int d0 = 0; d0 < PLANE; d0 += 64) {
      if (lane < SPW) {
        const int h = s_h[lane], w = s_w[lane], word0 = s_word0[lane];
        for (int j = 0; j < 64; ++j) {
          const int d = d0 + j, r = d / STAMP_SIDE, c = d - r * STAMP_SIDE;
          uint32_t v = 0;
          if (r < h && c < w) v = slot_w[(size_t)(word0 + r * w + c) * SPW + lane];
          tile[j * TILE_LD + lane] = v;
        }
      }
      __syncthreads();
      const int d = d0 + lane;
      if (d < PLANE) {
        for (int j = 0; j < SPW; ++j) {
          const long sj = g * SPW + j;
          if (sj >= n) break;
          const uint32_t v = __builtin_bswap32(tile[lane * TILE_LD + j]);
          raw[(size_t)sj * PLANE + d] = __uint_as_float(v);
        }
      }
      __syncthreads();
    }
  }
}

long slots_for(int n) {
  const long want = ((long)n + 63) / 64 * 64;
  return want < MAX_SLOTS ? want : MAX_SLOTS;
}

}  // namespace

extern "C" int64_t btsbot_decode_stamps_workspace(int n_stamps) {
  if (n_stamps < 0) {
    btsbot_set_error("btsbot_decode_stamps_workspace: negative n_stamps");
    return BTSBOT_ERR_INVALID_ARG;
  }
  return (int64_t)slots_for(n_stamps) * STAMP_CAP;
}

extern "C" int btsbot_decode_stamps(const uint8_t* blob, const int64_t* offsets, int n_stamps, float* raw,
                                    int32_t* shapes, uint8_t* status, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  if (n_stamps < 0) {
    btsbot_set_error("btsbot_decode_stamps: negative n_stamps");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (blob == nullptr || offsets == nullptr || raw == nullptr || shapes == nullptr || status == nullptr ||
      workspace == nullptr) {
    btsbot_set_error("btsbot_decode_stamps: NULL blob / offsets / raw / shapes / status / workspace");
    return BTSBOT_ERR_INVALID_ARG;
  }
  const long slots = slots_for(n_stamps);
  if (workspace_bytes < (int64_t)slots * STAMP_CAP) {
    btsbot_set_error("btsbot_decode_stamps: workspace of %lld bytes, %d stamps need %lld "
                     "(btsbot_decode_stamps_workspace)", (long long)workspace_bytes, n_stamps,
                     (long long)slots * STAMP_CAP);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(workspace) & 3u) != 0) {
    btsbot_set_error("btsbot_decode_stamps: workspace must be 4-byte aligned");
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_stamps == 0) return BTSBOT_OK;
  const long groups = ((long)n_stamps + STAMPS_PER_WAVE - 1) / STAMPS_PER_WAVE, resident = slots / STAMPS_PER_WAVE;
  hipLaunchKernelGGL(decode_stamps_kernel<STAMPS_PER_WAVE>, dim3((unsigned)(groups < resident ? groups : resident)),
                     dim3(64), 0, (hipStream_t)stream, blob, offsets, n_stamps, raw, shapes, status,
                     static_cast<uint8_t*>(workspace));
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
