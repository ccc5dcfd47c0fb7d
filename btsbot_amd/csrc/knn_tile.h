// What every btsbot_knn_* search shares (gfx950): the packed record, the 128 x 128 tile walk and the pieces of a tile
// pass, the direct-form distance, and the declarations of the host helpers that knn.hip defines once.
//   knn.hip         pack, the k-nearest selection and merge
//   knn_radius.hip  everything within r (4p)
//   knn_rank.hip    neighbour ranks (4r)
//
// A packed row is one record of 16 + 4 * dp bytes (dp = dim rounded up to 32, zero filled):
//   float bias, float scale, 8 bytes (bank rows: unused; query rows: |q|^2 and 1 / (2 |q|), for the radius passes),
//   f16 head[dp], f16 remainder[dp]
// (knn.hip: what the fields hold).  score = fma(-(acc * qscale), bscale, bias): the two scalings are exact.
//
// A tile pass is a grid of query tiles (128 rows) x bank splits; a workgroup (256 threads = 2 x 2 waves) walks its
// split's bank tiles of 128 rows, forms the 128 x 128 products on the matrix pipe (TileWalk) and hands every lane its
// 64 scores: query rows wm * 64 + mi * 16 + lrow, bank rows wn * 64 + ni * 16 + lq * 4 + i of the tile.  What a kernel
// does with them -- keep the best k, admit within r, count before a target -- is its own epilogue.
#pragma once
#include <float.h>

#include "common.h"

namespace {

constexpr int TQ = 128, TB = 128;   // query rows and bank rows per tile
constexpr int BK = 64;              // K elements per tile
constexpr int ROWB = 128;           // bytes per LDS row of one plane (64 f16)
constexpr int GEMM_LDS = 2 * (TQ + TB) * ROWB;   // 64 KB: four operand planes
constexpr int HDR = 16;             // bytes in front of a record's head plane
constexpr int EMPTY = 0x7fffffff;   // index of an empty list entry (score +inf)
constexpr int MAX_K = 64, MAX_DIM = 1024, MAX_SPLITS = 32;
enum { GM_EXCLUDE = BTSBOT_KNN_EXCLUDE_SAME, GM_ONE = BTSBOT_KNN_ONE_PER_GROUP };   // group mode bits
constexpr int MAX_K_ONE = 32;       // k's cap with one entry per group: the merge's pool carries its groups on chip

struct Cand {
  float s;
  int i;
};

__host__ __device__ inline int padded_dim(int dim) { return (dim + 31) & ~31; }
__host__ __device__ inline size_t record_bytes(int dim) { return (size_t)HDR + 4 * (size_t)padded_dim(dim); }

__device__ __forceinline__ bool before(float s1, int i1, float s2, int i2) { return s1 < s2 || (s1 == s2 && i1 < i2); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ f32x4 mma_x2(const h2x8& a, const h2x8& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.lo, b.hi, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.lo, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.hi, c, 0, 0, 0);
}

__device__ __forceinline__ int swz(int row, int chunk) { return row * ROWB + ((chunk ^ ((row >> 1) & 7)) << 4); }

// The barriers behind a tile's products: LDS traffic only, so the next tile's operand loads stay in flight across them
// (__syncthreads() would wait for them)
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");   // (no LDS read of the next phase moves above the barrier)
}

// The operand loads of K tile kt of bank tile `tile` into the caller's registers, and their store into the four LDS
// planes: free functions over the caller's arrays and scalars, the form in which the selection kernel keeps its
// registers, scratch and time.  CH 16-byte chunks per thread, plane and K tile (TQ == TB).
constexpr int CH = TQ * 8 / 256;
__device__ __forceinline__ void tile_gload(uint4 (&qh)[CH], uint4 (&ql)[CH], uint4 (&bh)[CH], uint4 (&bl)[CH],
                                           const unsigned char* qimg, const unsigned char* bimg, long Q, long q0, int N,
                                           int dp, size_t rec, int tid, int tile, int kt) {
  const int k0 = kt * BK;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = tid + i * 256, row = c >> 3, gk = k0 + (c & 7) * 8;
    const long gq = q0 + row;
    const long gb = (long)tile * TB + row;
    const bool kin = gk < dp;   // (dp % 8 == 0: a chunk is wholly inside or wholly outside)
    const unsigned char* pq = qimg + gq * rec + HDR + gk * 2;
    const unsigned char* pb = bimg + gb * rec + HDR + gk * 2;
    const bool okq = kin && gq < Q, okb = kin && gb < N;
    qh[i] = okq ? *reinterpret_cast<const uint4*>(pq) : make_uint4(0, 0, 0, 0);
    ql[i] = okq ? *reinterpret_cast<const uint4*>(pq + 2 * dp) : make_uint4(0, 0, 0, 0);
    bh[i] = okb ? *reinterpret_cast<const uint4*>(pb) : make_uint4(0, 0, 0, 0);
    bl[i] = okb ? *reinterpret_cast<const uint4*>(pb + 2 * dp) : make_uint4(0, 0, 0, 0);
  }
}
__device__ __forceinline__ void tile_sstore(unsigned char* smem, const uint4 (&qh)[CH], const uint4 (&ql)[CH],
                                            const uint4 (&bh)[CH], const uint4 (&bl)[CH], int tid) {
  unsigned char* Qh = smem;
  unsigned char* Ql = Qh + TQ * ROWB;
  unsigned char* Bh = Ql + TQ * ROWB;
  unsigned char* Bl = Bh + TB * ROWB;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = tid + i * 256;
    const int o = swz(c >> 3, c & 7);
    *reinterpret_cast<uint4*>(Qh + o) = qh[i];
    *reinterpret_cast<uint4*>(Ql + o) = ql[i];
    *reinterpret_cast<uint4*>(Bh + o) = bh[i];
    *reinterpret_cast<uint4*>(Bl + o) = bl[i];
  }
}

// A workgroup's walk over its bank tiles: the operand registers of the K tile in flight (loaded under the products of
// the one before) and the 128 x 128 x dp products of one bank tile.
// products() leaves behind an lds_barrier: the operand planes are idle and may be used by the caller's epilogue, which
// must end with a barrier of its own if it writes there.
struct TileWalk {
  static constexpr int MI = 4, NI = 4;     // 16-row fragments per wave: queries (B operand), bank rows (A operand)
  const unsigned char* qimg;
  const unsigned char* bimg;
  unsigned char* smem;
  long Q, q0;
  int N, dp, nk, tid;
  size_t rec;
  uint4 qh[CH], ql[CH], bh[CH], bl[CH];

  __device__ __forceinline__ void init(const unsigned char* qi, const unsigned char* bi, unsigned char* lds, long nq,
                                       long first_q, int nb, int dim) {
    qimg = qi;
    bimg = bi;
    smem = lds;
    Q = nq;
    q0 = first_q;
    N = nb;
    dp = padded_dim(dim);
    nk = (dp + BK - 1) / BK;
    tid = threadIdx.x;
    rec = record_bytes(dim);
  }
  __device__ __forceinline__ void gload(int tile, int kt) {
    tile_gload(qh, ql, bh, bl, qimg, bimg, Q, q0, N, dp, rec, tid, tile, kt);
  }
  __device__ __forceinline__ void sstore() { tile_sstore(smem, qh, ql, bh, bl, tid); }
  // acc[ni][mi] = the products of bank tile `tile` (gload(tile, 0) has been issued); loads the next tile's first operands
  __device__ __forceinline__ void products(f32x4 (&acc)[NI][MI], int tile, int t_end) {
    const unsigned char* Qh = smem;
    const unsigned char* Ql = Qh + TQ * ROWB;
    const unsigned char* Bh = Ql + TQ * ROWB;
    const unsigned char* Bl = Bh + TB * ROWB;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = lane & 15, lq = lane >> 4;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kt = 0; kt < nk; ++kt) {
      sstore();
      __syncthreads();
      if (kt + 1 < nk) gload(tile, kt + 1);
      else if (tile + 1 < t_end) gload(tile + 1, 0);
#pragma unroll 1   // (unrolled, the fragments of both halves are loaded up front: 56 registers to scratch)
      for (int ks = 0; ks < BK / 32; ++ks) {
        if (kt * BK + ks * 32 < dp) {
          h2x8 bfr[MI];
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            const int o = swz(wm * 64 + mi * 16 + lrow, ks * 4 + lq);
            bfr[mi].hi = *reinterpret_cast<const f16x8*>(Qh + o);
            bfr[mi].lo = *reinterpret_cast<const f16x8*>(Ql + o);
          }
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            const int o = swz(wn * 64 + ni * 16 + lrow, ks * 4 + lq);
            h2x8 afr;
            afr.hi = *reinterpret_cast<const f16x8*>(Bh + o);
            afr.lo = *reinterpret_cast<const f16x8*>(Bl + o);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = mma_x2(afr, bfr[mi], acc[ni][mi]);
          }
        }
      }
      lds_barrier();
    }
  }
};

// ---- the pieces of a tile pass.  The radius and rank kernels are built of all of them; the selection of those that
// leave its allocation as it was (see there)

// a thread's place in the 2 x 2 waves: its query rows are wm * 64 + mi * 16 + lrow, its bank rows wn * 64 + ni * 16 +
// lq * 4 + i of the tile
struct LanePos {
  int wm, wn, lrow, lq;
  __device__ __forceinline__ LanePos() {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    wm = wave >> 1;
    wn = wave & 1;
    lrow = lane & 15;
    lq = lane >> 4;
  }
  __device__ __forceinline__ int qrow(int mi) const { return wm * 64 + mi * 16 + lrow; }
  __device__ __forceinline__ long gq(long q0, int mi) const { return q0 + wm * 64 + mi * 16 + lrow; }
  __device__ __forceinline__ int brow(int ni, int i) const { return wn * 64 + ni * 16 + lq * 4 + i; }
  __device__ __forceinline__ int gb(int b0, int ni, int i) const { return b0 + wn * 64 + ni * 16 + lq * 4 + i; }
};

// split = blockIdx.y: its bank tiles [t_begin, t_end), and where its bank rows end
struct SplitRange {
  int split, t_begin, t_end, b_end;
  __device__ __forceinline__ SplitRange(int N, int tiles_per_split) {
    split = blockIdx.y;
    const int total_tiles = (N + TB - 1) / TB;
    t_begin = (int)min((long)split * tiles_per_split, (long)total_tiles);
    t_end = (int)min((long)(split + 1) * tiles_per_split, (long)total_tiles);
    b_end = (int)min((long)t_end * TB, (long)N);
  }
};

// The header of the lane's four query rows.  A row past Q has scale 0 and group 0: it never has a candidate.
template <bool EXCL>
struct QueryRows {
  float sq[TileWalk::MI], qq[TileWalk::MI], qinv[TileWalk::MI];   // the record's scale, |q|^2, 1 / (2 |q|)
  int selfb[TileWalk::MI];    // the bank row that IS the query row (never a candidate), -1: none
  long long qg[TileWalk::MI]; // EXCL: the rows' groups
  __device__ __forceinline__ void load(const unsigned char* qimg, size_t rec, long Q, long q0, int N, long self_offset,
                                       const long long* __restrict__ qgrp, const LanePos& p) {
#pragma unroll
    for (int mi = 0; mi < TileWalk::MI; ++mi) {
      const long gq = p.gq(q0, mi);
      const float4 h = gq < Q ? *reinterpret_cast<const float4*>(qimg + gq * rec) : make_float4(0.f, 0.f, 0.f, 0.f);
      sq[mi] = h.y;
      qq[mi] = h.z;
      qinv[mi] = h.w;
      const long sb = gq + self_offset;
      selfb[mi] = self_offset >= 0 && sb < N ? (int)sb : -1;
    }
    if constexpr (EXCL) {
#pragma unroll
      for (int mi = 0; mi < TileWalk::MI; ++mi) {
        const long gq = p.gq(q0, mi);
        qg[mi] = gq < Q ? qgrp[gq] : 0;
      }
    }
  }
};

// The tile's 128 bank groups: loaded under the products, one per thread (load_tile_group), put into the idle operand
// LDS behind them by the caller, from where a fragment's four are read inside the ni loop (frag_groups)
__device__ __forceinline__ long long load_tile_group(const long long* __restrict__ bgrp, int b0, int N) {
  const int tid = threadIdx.x;
  long long gt = 0;
  if (tid < TB && (long)b0 + tid < N) gt = bgrp[(long)b0 + tid];
  return gt;
}
__device__ __forceinline__ void frag_groups(const long long* tg, const LanePos& p, int ni, long long (&bg)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) bg[i] = tg[p.brow(ni, i)];
}

// the biases and scales of the four bank rows of fragment ni of the tile at b0 (a row past N: +inf and 0)
__device__ __forceinline__ void frag_bias_scale(const unsigned char* bimg, size_t rec, int N, const LanePos& p, int b0,
                                                int ni, float (&nb)[4], float (&sb)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = p.gb(b0, ni, i);
    const float2 h = b < N ? *reinterpret_cast<const float2*>(bimg + (size_t)b * rec)
                           : make_float2(__builtin_inff(), 0.f);
    nb[i] = h.x;
    sb[i] = h.y;
  }
}

__device__ __forceinline__ float tile_score(float acc, float sq, float sb, float nb) { return fmaf(-(acc * sq), sb, nb); }

// ---- the selection's lists (knn.hip, ivf.hip)
constexpr int TG_OFF = 16 * 1024;   // the tile's bank groups in the idle operand LDS, behind buckets, counts and flags

// A list is the k best by (score, index) of what it was offered, UNSORTED (the merge ranks by counting), with its worst
// entry (ts, ti) at position tp: a better candidate replaces the worst, then the worst is looked up again -- k independent
// LDS reads, where shifting a sorted list was a chain of dependent ones (23 of 51 ms at N = 500,000, D = 528, k = 15).
__device__ __forceinline__ void offer(Cand* mine, int k, float s, int gb, float& ts, int& ti, int& tp) {
  if (!before(s, gb, ts, ti)) return;
  mine[tp] = Cand{s, gb};
  Cand w = mine[0];
  int wp = 0;
#pragma unroll 4
  for (int j = 1; j < k; ++j) {
    const Cand o = mine[j];
    if (before(w.s, w.i, o.s, o.i)) {
      w = o;
      wp = j;
    }
  }
  ts = w.s;
  ti = w.i;
  tp = wp;
}

// One entry per group (knn.hip's header has the argument): mg[j * stride] is the group of mine[j], in the workspace,
// the owner's own column of a [k][stride] block -- coalesced over the owners.  An entry of the candidate's group decides
// alone -- the better of the two stays in its place --; without one the candidate is offered as above.  Stride: int for
// the exact search's constant TQ (its index arithmetic, hence its allocation, as it was), long for the listed pass.
template <typename Stride>
__device__ __forceinline__ void offer_one(Cand* mine, long long* mg, Stride stride, int k, float s, int gb, long long g,
                                          float& ts, int& ti, int& tp) {
  if (!before(s, gb, ts, ti)) return;
  int at = -1;
#pragma unroll 4
  for (int j = 0; j < k; ++j)
    if (mg[j * stride] == g && mine[j].i != EMPTY) at = j;   // (at most one entry matches; an empty entry has no group)
  if (at >= 0) {
    const Cand e = mine[at];
    if (!before(s, gb, e.s, e.i)) return;
  } else {
    at = tp;
  }
  mine[at] = Cand{s, gb};
  mg[at * stride] = g;
  Cand w = mine[0];
  int wp = 0;
#pragma unroll 4
  for (int j = 1; j < k; ++j) {
    const Cand o = mine[j];
    if (before(w.s, w.i, o.s, o.i)) {
      w = o;
      wp = j;
    }
  }
  ts = w.s;
  ti = w.i;
  tp = wp;
}

// The merges' one-per-group step, by one wave: pool[0..P) are a query's candidates and pgrp[c] the group of pool[c]
// (both in LDS and visible).  An entry counts only if no pool entry of its group is before it by (score, index) -- the
// bests of one group from the several splits, or probed lists, meet here --; the others become empty.  P <= 32 * 32: at
// most 16 entries per lane.  Ends with a barrier: the pool is ready to be ranked.
__device__ __forceinline__ void keep_group_bests(Cand* pool, const long long* pgrp, int P, int lane) {
  unsigned lose = 0;   // bit j: entry lane + 64 j
  for (int c = lane, j = 0; c < P; c += 64, ++j) {
    const Cand me = pool[c];
    if (me.i == EMPTY) continue;
    const long long g = pgrp[c];
    bool l = false;
    for (int e = 0; e < P; ++e) {
      const Cand o = pool[e];
      l = l || (o.i != EMPTY && pgrp[e] == g && before(o.s, o.i, me.s, me.i));
    }
    lose |= l ? 1u << j : 0u;
  }
  __syncthreads();
  for (int c = lane, j = 0; c < P; c += 64, ++j)
    if ((lose >> j & 1u) != 0) pool[c] = Cand{__builtin_inff(), EMPTY};
  __syncthreads();
}

// `near`, the kind's own test of the pair, and: may bank row gb be a candidate of this query row at all -- finite, inside
// the split, not the row itself and (EXCL) not of its group.  (One chain, the kind's test first, as the kernels had it:
// with that test outside the radius count pass is 6 % slower)
template <bool EXCL>
__device__ __forceinline__ bool eligible(bool near, float s, int gb, int b_end, int selfb, const long long& bg,
                                         const long long& qg) {
  bool in = near && s < __builtin_inff() && gb < b_end && gb != selfb;
  if constexpr (EXCL) in = in && bg != qg;
  return in;
}

// The radius and rank passes' per-row state behind the operand planes, RowRegions::BYTES of LDS: a counter per query
// row of the tile -- the count pass's result, the fill's cursor -- and, for the fill, the size and start of the region
// that the scan of the counts gave (query, split).
struct RowRegions {
  static constexpr int BYTES = TQ * 16;
  int* cnt;          // [TQ]
  int* cap;          // [TQ] FILL
  long long* base;   // [TQ] FILL
  // (visible after the caller's next __syncthreads())
  template <bool FILL>
  __device__ __forceinline__ void init(unsigned char* lds, long Q, long q0, int splits, int split, const int* counts,
                                       const long long* __restrict__ offsets) {
    cnt = reinterpret_cast<int*>(lds);
    cap = cnt + TQ;
    base = reinterpret_cast<long long*>(cap + TQ);
    const int tid = threadIdx.x;
    if (tid < TQ) {
      cnt[tid] = 0;
      if constexpr (FILL) {
        const bool in = q0 + tid < Q;
        cap[tid] = in ? counts[(q0 + tid) * splits + split] : 0;
        base[tid] = in ? offsets[(q0 + tid) * splits + split] : 0;
      }
    }
  }
  // FILL: the next slot of row's region as an index below n, or -1 for a slot past the region (never, while counts
  // and offsets are the count pass's: the same arithmetic)
  __device__ __forceinline__ long long slot(int row, long long n) {
    const int slot = atomicAdd(&cnt[row], 1);
    const long long at = base[row] + slot;
    return slot < cap[row] && at >= 0 && at < n ? at : -1;
  }
  // the count pass's ending: the lanes' counts n[mi] of their four rows meet in the row counters, which go to counts
  __device__ __forceinline__ void store_counts(const int (&n)[TileWalk::MI], const LanePos& p, long Q, long q0, int splits,
                                               int split, int* counts) {
#pragma unroll
    for (int mi = 0; mi < TileWalk::MI; ++mi)
      if (n[mi] != 0) atomicAdd(&cnt[p.qrow(mi)], n[mi]);
    __syncthreads();
    const int tid = threadIdx.x;
    if (tid < TQ && q0 + tid < Q) counts[(q0 + tid) * splits + split] = cnt[tid];
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// The distance the library returns, in the direct form from the fp32 rows, by one wave: xv = the query row (element
// j * 64 + lane in xv[j], zero past dim), qq = its squared norm (wave_sum of the lanes' fma chains), y = the bank row.
// Lane-strided fma chains, the fixed butterfly, a correctly rounded sqrtf.  The merge applies it to the rows it returns,
// the radius search decides membership by it and the ranks are counted by it: one function, so they agree bit for bit.
__device__ __forceinline__ float direct_distance(const float (&xv)[MAX_DIM / 64], float qq, const float* __restrict__ y,
                                                 int dim, int metric, int lane) {
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int jj = 0; jj < MAX_DIM / 64; ++jj) {
    const int d = jj * 64 + lane;
    if (d < dim) {
      const float yv = y[d];
      if (metric == 0) {
        const float t = xv[jj] - yv;
        a0 = fmaf(t, t, a0);
      } else {
        a0 = fmaf(xv[jj], yv, a0);
        a1 = fmaf(yv, yv, a1);
      }
    }
  }
  a0 = wave_sum(a0);
  if (metric == 0) return sqrtf(a0);
  a1 = wave_sum(a1);
  const float c = qq > 0.f && a1 > 0.f ? (a0 / sqrtf(qq)) / sqrtf(a1) : 0.f;
  return 1.f - c;
}

// the query row of a wave as direct_distance takes it; false for a row that holds a non-finite value or whose squared
// norm is not finite (the selection saw a zero image for it)
__device__ __forceinline__ bool load_query_row(const float* __restrict__ x, int dim, int lane, float (&xv)[MAX_DIM / 64],
                                               float& qq) {
  bool fin = true;
  qq = 0.f;
#pragma unroll
  for (int j = 0; j < MAX_DIM / 64; ++j) {
    const int d = j * 64 + lane;
    xv[j] = d < dim ? x[d] : 0.f;
    fin = fin && fabsf(xv[j]) <= FLT_MAX;
    qq = fmaf(xv[j], xv[j], qq);
  }
  qq = wave_sum(qq);
  return __all(fin) && qq <= FLT_MAX;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// The host helpers of the entry points, defined once in knn.hip
namespace knn {

// What an entry point was given, as check_search() needs it.  The kinds differ in: k's value (radius: 1, ranks:
// n_targets), whether splits may be 0 (the library's choice: the k-nearest query only), the flags they know and the
// word their messages name themselves by (nullptr: the query's wording), their required pointers and what they keep
// in the workspace behind the packed query rows.
struct SearchArgs {
  int64_t n_query, n_bank;
  int dim, k, metric;
  int splits, min_splits;
  int flags, flag_mask;
  const char* mode_word;
  bool null_arg;   // one of the kind's required pointers is NULL
  const void *query_group, *bank_group, *packed, *workspace;
  int64_t workspace_bytes;
  size_t extra_bytes;
};

int check_shape(const char* who, int64_t n_query, int64_t n_bank, int dim, int k);
size_t image_bytes(int64_t rows, int dim);   // the packed image of `rows` rows, rounded up to 256 bytes
// Shapes, metric, splits, flags, then -- unless n_query == 0, which needs nothing -- pointers, groups and workspace
int check_search(const char* who, const SearchArgs& a);

// the margin of DESIGN.md 4p / 4r (u = 2^-24): rel = 1 + 4 (D + 4) u, relm = 1 - 4 (D + 4) u, ctau = 8 (D + 8) u
// (cosine: 16 (D + 8) u)
struct Margin {
  float rel, relm, ctau;
};
Margin margin(int dim, int metric);

// a tile pass's grid (query tiles x splits) and the bank tiles each split walks
struct TileGrid {
  int tiles_per_split;
  dim3 grid;
};
TileGrid tile_grid(int64_t n_query, int64_t n_bank, int splits);

// the verify kernels' grid.y: enough waves per query that a crowded row does not serialise, its n / n_query entries
// on average shared out 32 to a wave, 64 waves at the most
unsigned verify_waves(int64_t n, int64_t n_query);

// the launch that packs the query rows into the head of a workspace
int pack_queries(const float* queries, int64_t n_query, int dim, unsigned char* qimg, hipStream_t st);

}  // namespace knn
