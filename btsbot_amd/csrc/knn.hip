// btsbot_knn_*: exact brute-force k-nearest neighbours over embedding rows (gfx950), DESIGN.md section 4m.
//
//   idx[q][0..k), dist[q][0..k) = the k bank rows nearest to query row q, ascending by (dist, bank index)
//
// Two passes, neither of which writes anything of size Q x N:
//
//   selection  grid = query tiles (128 rows) x bank splits.  A workgroup walks its slice of the bank in tiles of 128 rows,
//              forms the 128 x 128 products on the matrix pipe and keeps each query row's best k (score, index) pairs
//              in LDS.  score = |b|^2 - 2 q.b (Euclidean; |q|^2 is the same for every candidate of a row) or
//              -2 q.b / |b| (cosine).  Ties go to the lower bank index.  k candidates per (query, split) to the workspace.
//   merge      one wave per query: the k best of its splits * k candidates by (score, index) -- the same k whatever the
//              number of splits --, each one's distance again in the direct form (sum (q_i - b_i)^2, or the fp32 dot and
//              norms) from the ORIGINAL fp32 rows, sorted by (distance, index).
//
// Operands: every row enters the products as an f16 head + f16 remainder of the row scaled by a power of two of its own
// (its largest magnitude lands in [2^14, 2^15): common.h, split_exp), three v_mfma_f32_16x16x32_f16 per product, small
// terms first (gemm_x2.hip).  The scale is per ROW, so a row's image depends on nothing but the row: an index built by
// several adds equals one built at once, and a query's answer does not depend on its neighbours in the batch.  A packed row
// is one record of 16 + 4 * dp bytes (dp = dim rounded up to 32, zero filled):
//   float bias, float scale, 8 bytes (bank rows: unused; query rows: |q|^2 and 1 / (2 |q|), for the radius passes),
//   f16 head[dp], f16 remainder[dp]
// bank rows: bias = |b|^2 and scale = 2^-e (Euclidean), bias = 0 and scale = 2^-e / |b| (cosine; 0 for a zero row); a row
// that holds a non-finite value, or whose squared norm is not finite in fp32, has bias = +inf, scale = 0 and a zero image:
// its score is +inf and +inf is never kept.  Query rows: scale = 2^(1-e) (0 and a zero image for a non-finite row, which
// the merge answers with idx = -1, dist = NaN).  score = fma(-(acc * qscale), bscale, bias): the two scalings are exact.
//
// The GEMM part is gemm_x2.hip's 128 x 128 tile (256 threads = 2 x 2 waves, K tile 64, the same LDS swizzle, the MFMA run
// "transposed": bank rows = A operand, query rows = B operand) reading both operands already split; the next K tile's
// (and the next bank tile's first) operands are loaded into registers under the products.  After a tile's products every
// lane compares its 64 scores with its rows' worst kept score; what passes goes into per-row buckets in the (then idle)
// operand LDS, and thread q, the owner of row q's list, takes its bucket: see offer().  Nothing here meets through an
// atomic whose order matters: the bucket slots are handed out by LDS atomics, but a list is the k best of what it was
// offered whatever the order.  LDS: 64 KB of operands + 1 KB of lists per k, so two workgroups share a CU up to k = 16.
//
// Groups (btsbot_knn_query_grouped).  A row may carry a group, any int64 (an alert's object).  Both kernels are templates
// on the group mode GM; GM = 0 is the code above, unchanged, and is what btsbot_knn_query launches.
//   GM & 1, exclude   a bank row of the query row's group is never a candidate: one more term in the mask that decides
//                     which of a lane's 64 scores may be offered.  The query groups of the lane's four rows stay in
//                     registers; the tile's 128 bank groups are loaded under the products (one per thread) and put into
//                     the idle operand LDS behind them, from where a fragment's four are read inside the ni loop.
//   GM & 2, one per group   a list holds at most one entry per group, the group's best by (score, index).  The groups of
//                     the entries, in full -- 64 bits decide equality, there is no tag --, do NOT live in LDS: 8 more
//                     bytes per entry there leave one workgroup per CU from k = 9 on, and that alone cost 1.8 x at
//                     k = 15 (measured).  They live in the workspace, a [k][128] block per workgroup that
//                     only its owner threads read and write, each its own column: an offer that passes the pre-filter
//                     reads k of them, coalesced over the owners, from L2.  k <= 32 in this mode: the merge keeps the
//                     groups of its splits * k pool entries on chip (8 KB at 32 x 32) and its per-lane mask of losers
//                     has 16 bits in use.
// Why a list is still independent of the order of its offers.  Let S be the set offered so far and B(S) the best row of
// every group in S.  Invariant: the list is the k best of B(S).  Offer c of group g.  (a) g has an entry e in the list:
// e is g's best in S; c before e -> c replaces e in place (it is before e, so it stays among the k best), else B(S)
// and the list stay.  (b) g has no entry: g's best in S, if any, is not before the list's worst w (it was refused or
// evicted by k better groups, and lists only improve).  c before w -> c is g's new best and enters for w; the old best
// of g leaves B(S) unnoticed; otherwise the k best of B do not change.  No row ever has to come BACK: B(S) loses a row
// only to a better row of the same group.  So the list is a function of S alone, and the pre-filter s <= thr stays valid:
// a candidate not before the worst of k distinct groups' bests is not before its own group's entry either.
// The merge then keeps, of a query's splits * k pool entries, those with no pool entry of their group before them, and
// ranks among these: a group's best over the whole bank is its best split-best, and a row that is not its group's best
// has k groups' bests of one split before it, each represented in the pool by a kept entry no worse -- rank >= k.  The
// answer is the same whatever `splits` is.
//
// Radius search (btsbot_knn_radius_*): the same grid and tile walk with the epilogue "admit if
// within r" -- see knn_radius_kernel -- and direct_distance(), the one function that computes a returned distance, for
// the merge's winners and for every radius candidate alike.
//
// Neighbour ranks (btsbot_knn_rank_*): the same walk with a third epilogue, "count if surely before
// the target, hand to the direct form if within the margin" -- see knn_rank_kernel.
#include <float.h>

#include "common.h"

namespace {

constexpr int TQ = 128, TB = 128;   // query rows and bank rows per tile
constexpr int BK = 64;              // K elements per tile
constexpr int ROWB = 128;           // bytes per LDS row of one plane (64 f16)
constexpr int GEMM_LDS = 2 * (TQ + TB) * ROWB;   // 64 KB: four operand planes
constexpr int BCAP = 8;             // candidates a query row's bucket holds per round
constexpr int HDR = 16;             // bytes in front of a record's head plane
constexpr int EMPTY = 0x7fffffff;   // index of an empty list entry (score +inf)
constexpr int MAX_K = 64, MAX_DIM = 1024, MAX_SPLITS = 32;
enum { MODE_BANK_L2 = 0, MODE_BANK_COS = 1, MODE_QUERY = 2 };
enum { GM_EXCLUDE = BTSBOT_KNN_EXCLUDE_SAME, GM_ONE = BTSBOT_KNN_ONE_PER_GROUP };   // group mode bits (template GM)
constexpr int MAX_K_ONE = 32;       // k's cap with one entry per group: the merge's pool carries its groups on chip
constexpr int TG_OFF = 16 * 1024;   // the tile's bank groups in the idle operand LDS, behind buckets, counts and flags

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

// ---------------------------------------------------------------------------------------------------------------------
// pack: one wave per row
__global__ __launch_bounds__(256) void knn_pack_kernel(const float* __restrict__ rows, long n_rows, int dim, int mode,
                                                       unsigned char* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int dp = padded_dim(dim);
  const float* x = rows + row * dim;
  float v[MAX_DIM / 64];
  unsigned amax = 0;
  bool fin = true;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < MAX_DIM / 64; ++j) {
    const int d = j * 64 + lane;
    v[j] = d < dim ? x[d] : 0.f;
    fin = fin && fabsf(v[j]) <= FLT_MAX;   // false for inf and NaN
    amax = max(amax, __float_as_uint(fabsf(v[j])));
    ss = fmaf(v[j], v[j], ss);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) amax = max(amax, (unsigned)__shfl_xor((int)amax, o));
  fin = __all(fin);
  ss = wave_sum(ss);
  const bool ok = fin && ss <= FLT_MAX;
  int e = 0;
  const float a = __uint_as_float(amax);
  if (ok && a > 0.f) {
    int ex;
    (void)frexpf(a, &ex);   // a in [2^(ex-1), 2^ex)
    e = 15 - ex;
    e = e < -120 ? -120 : e > 120 ? 120 : e;
  }
  const float up = ok ? ldexpf(1.f, e) : 0.f;
  unsigned char* rec = out + (size_t)row * record_bytes(dim);
  f16_t* hi = reinterpret_cast<f16_t*>(rec + HDR);
  f16_t* lo = hi + dp;
#pragma unroll
  for (int j = 0; j < MAX_DIM / 64; ++j) {
    const int d = j * 64 + lane;
    if (d < dp) {
      f16_t h, l;
      split_f16(ok ? v[j] * up : 0.f, h, l);
      hi[d] = h;
      lo[d] = l;
    }
  }
  if (lane == 0) {
    float bias = 0.f, scale = 0.f, qq = 0.f, qinv = 0.f;   // qq, qinv: query records only (the radius passes)
    if (mode == MODE_QUERY) {
      scale = ok ? ldexpf(1.f, 1 - e) : 0.f;
      qq = ok ? ss : 0.f;
      qinv = ok && ss > 0.f ? 0.5f / sqrtf(ss) : 0.f;
    } else if (!ok) {
      bias = __builtin_inff();
    } else if (mode == MODE_BANK_L2) {
      bias = ss;
      scale = ldexpf(1.f, -e);
    } else {
      scale = ss > 0.f ? ldexpf(1.f, -e) / sqrtf(ss) : 0.f;
    }
    *reinterpret_cast<float4*>(rec) = make_float4(bias, scale, qq, qinv);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// selection
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

// A workgroup's walk over its bank tiles, the selection kernel's statements as a struct for the radius kernels (the
// selection keeps its own text, see there): the operand registers of the K tile in flight (loaded under the products of
// the one before) and the 128 x 128 x dp products of one bank tile.
// products() leaves behind an lds_barrier: the operand planes are idle and may be used by the caller's epilogue, which
// must end with a barrier of its own if it writes there.
struct TileWalk {
  static constexpr int MI = 4, NI = 4;     // 16-row fragments per wave: queries (B operand), bank rows (A operand)
  static constexpr int CH = TQ * 8 / 256;  // 16-byte chunks per thread, plane and K tile (TQ == TB)
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
  __device__ __forceinline__ void sstore() {
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

// One entry per group (the header's argument): mg[j * TQ] is the group of mine[j], in the workspace (the owner's own
// column of its workgroup's [k][TQ] block: coalesced over the owners).  An entry of the candidate's group decides
// alone -- the better of the two stays in its place --; without one the candidate is offered as above.
__device__ __forceinline__ void offer_one(Cand* mine, long long* mg, int k, float s, int gb, long long g, float& ts,
                                          int& ti, int& tp) {
  if (!before(s, gb, ts, ti)) return;
  int at = -1;
#pragma unroll 4
  for (int j = 0; j < k; ++j)
    if (mg[j * TQ] == g && mine[j].i != EMPTY) at = j;   // (at most one entry matches; an empty entry has no group)
  if (at >= 0) {
    const Cand e = mine[at];
    if (!before(s, gb, e.s, e.i)) return;
  } else {
    at = tp;
  }
  mine[at] = Cand{s, gb};
  mg[at * TQ] = g;
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

template <int GM>
__global__ __launch_bounds__(256, 2) void knn_select_kernel(const unsigned char* __restrict__ qimg,
                                                            const unsigned char* __restrict__ bimg, long Q, int N,
                                                            int dim, int k, long self_offset, int tiles_per_split,
                                                            int splits, Cand* __restrict__ cand,
                                                            const long long* __restrict__ qgrp,
                                                            const long long* __restrict__ bgrp,
                                                            long long* __restrict__ lgrp) {
  constexpr int MI = 4, NI = 4;     // 16-row fragments per wave: queries (B operand), bank rows (A operand)
  constexpr int CH = TQ * 8 / 256;  // 16-byte chunks per thread, plane and K tile (TQ == TB)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Qh = smem;
  unsigned char* Ql = Qh + TQ * ROWB;
  unsigned char* Bh = Ql + TQ * ROWB;
  unsigned char* Bl = Bh + TB * ROWB;
  Cand* L = reinterpret_cast<Cand*>(smem + GEMM_LDS);   // [TQ][k] lists
  // behind a tile's products, over the idle operand planes: the candidate buckets of the tile's query rows, their fill
  // counts, the rows' worst kept scores and two "candidates left over" flags
  Cand* bucket = reinterpret_cast<Cand*>(smem);         // [TQ][BCAP] (score, bank row of the tile)
  int* bcnt = reinterpret_cast<int*>(bucket + TQ * BCAP);
  float* thr = reinterpret_cast<float*>(bcnt + TQ);
  int* flag = reinterpret_cast<int*>(thr + TQ);
  // GM & GM_ONE: the groups of this thread's list entries, entry j at LG[j * TQ]
  long long* LG = lgrp + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * (size_t)k * TQ + threadIdx.x;
  long long* tg = reinterpret_cast<long long*>(smem + TG_OFF);       // GM != 0: [TB] the tile's bank groups

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 15, lq = lane >> 4;
  const int dp = padded_dim(dim);
  const size_t rec = record_bytes(dim);
  const long q0 = (long)blockIdx.x * TQ;
  const int split = blockIdx.y;
  const int total_tiles = (N + TB - 1) / TB;
  const int t_begin = (int)min((long)split * tiles_per_split, (long)total_tiles);
  const int t_end = (int)min((long)(split + 1) * tiles_per_split, (long)total_tiles);
  const int b_end = (int)min((long)t_end * TB, (long)N);
  const int nk = (dp + BK - 1) / BK;

  // the thread's own list (threads 0..TQ-1: query row q0 + tid)
  const bool owner = tid < TQ && q0 + tid < Q;
  float ts = __builtin_inff();
  int ti = EMPTY, tp = 0;
  if (tid < TQ)
    for (int j = 0; j < k; ++j) L[tid * k + j] = Cand{__builtin_inff(), EMPTY};

  float sq[MI];
  int selfb[MI];   // the bank row that IS the query row (never a candidate), -1: none
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const long gq = q0 + wm * 64 + mi * 16 + lrow;
    sq[mi] = gq < Q ? reinterpret_cast<const float*>(qimg + gq * rec)[1] : 0.f;
    const long sb = gq + self_offset;
    selfb[mi] = self_offset >= 0 && sb < N ? (int)sb : -1;
  }
  long long qg[MI];   // GM & GM_EXCLUDE: the groups of the lane's four query rows
  if constexpr ((GM & GM_EXCLUDE) != 0) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const long gq = q0 + wm * 64 + mi * 16 + lrow;
      qg[mi] = gq < Q ? qgrp[gq] : 0;   // (a row past Q never has a candidate)
    }
  }

  // (the operand loads and the products below are TileWalk's, kept in this kernel's own text: routed through the
  //  struct the same statements allocate registers differently -- scratch 172 -> 156, 280 -> 288 bytes -- and this
  //  kernel's figures are held fixed)
  uint4 qh[CH], ql[CH], bh[CH], bl[CH];
  auto gload = [&](int tile, int kt) {
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
  };
  auto sstore = [&]() {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + i * 256;
      const int o = swz(c >> 3, c & 7);
      *reinterpret_cast<uint4*>(Qh + o) = qh[i];
      *reinterpret_cast<uint4*>(Ql + o) = ql[i];
      *reinterpret_cast<uint4*>(Bh + o) = bh[i];
      *reinterpret_cast<uint4*>(Bl + o) = bl[i];
    }
  };

  if (t_begin < t_end) gload(t_begin, 0);
  __syncthreads();   // the lists
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int b0 = tile * TB;
    long long gt = 0;   // GM != 0: bank row b0 + tid's group, in flight under the products
    if constexpr (GM != 0) {
      if (tid < TB && (long)b0 + tid < N) gt = bgrp[(long)b0 + tid];
    }
    f32x4 acc[NI][MI];
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

    // ---- the tile's candidates.  The operand planes are idle: the owners publish their worst kept scores there
    if (tid < TQ) {
      thr[tid] = owner ? ts : -__builtin_inff();   // (a row past Q never has a candidate)
      bcnt[tid] = 0;
      if constexpr (GM != 0) tg[tid] = gt;
    }
    if (tid < 2) flag[tid] = 0;
    lds_barrier();
    // scores, and which of them can enter a list (<=: a tie may still win on the index); the tile's bank biases and
    // scales: rows b0 + wn * 64 + ni * 16 + lq * 4 + i
    float t[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) t[mi] = thr[wm * 64 + mi * 16 + lrow];
    unsigned long long mask = 0;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float nb[4], sb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = b0 + wn * 64 + ni * 16 + lq * 4 + i;
        const float2 h = b < N ? *reinterpret_cast<const float2*>(bimg + (size_t)b * rec)
                               : make_float2(__builtin_inff(), 0.f);
        nb[i] = h.x;
        sb[i] = h.y;
      }
      long long bg[4];   // GM & GM_EXCLUDE: the fragment's bank groups
      if constexpr ((GM & GM_EXCLUDE) != 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bg[i] = tg[wn * 64 + ni * 16 + lq * 4 + i];
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gb = b0 + wn * 64 + ni * 16 + lq * 4 + i;
          const float s = fmaf(-(acc[ni][mi][i] * sq[mi]), sb[i], nb[i]);
          acc[ni][mi][i] = s;
          bool in = s <= t[mi] && s < __builtin_inff() && gb < b_end && gb != selfb[mi];
          if constexpr ((GM & GM_EXCLUDE) != 0) in = in && bg[i] != qg[mi];
          if (in) mask |= 1ull << ((ni * MI + mi) * 4 + i);
        }
    }
    // Rounds of: every lane puts its candidates into their rows' buckets (BCAP each; what finds no room waits for the
    // next round, unless the row's worst kept score has passed it by then), every owner takes its bucket.  A list does
    // not depend on the order it is offered its candidates in.
    for (int rc = 0;; ++rc) {
      if (mask != 0) {
        if (rc > 0) {
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) t[mi] = thr[wm * 64 + mi * 16 + lrow];
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const unsigned long long bit = 1ull << ((ni * MI + mi) * 4 + i);
              if ((mask & bit) != 0) {
                const int row = wm * 64 + mi * 16 + lrow;
                if (!(acc[ni][mi][i] <= t[mi])) {
                  mask &= ~bit;
                } else {
                  const int slot = atomicAdd(&bcnt[row], 1);
                  if (slot < BCAP) {
                    bucket[row * BCAP + slot] = Cand{acc[ni][mi][i], wn * 64 + ni * 16 + lq * 4 + i};
                    mask &= ~bit;
                  }
                }
              }
            }
        if (mask != 0) flag[rc & 1] = 1;
      }
      if (tid == 0) flag[(rc + 1) & 1] = 0;   // (last read before the previous round's second barrier)
      lds_barrier();
      if (owner) {
        const int n = min(bcnt[tid], BCAP);
        for (int e = 0; e < n; ++e) {
          const Cand c = bucket[tid * BCAP + e];
          if constexpr ((GM & GM_ONE) != 0) offer_one(L + tid * k, LG, k, c.s, b0 + c.i, tg[c.i], ts, ti, tp);
          else offer(L + tid * k, k, c.s, b0 + c.i, ts, ti, tp);
        }
        thr[tid] = ts;
      }
      if (tid < TQ) bcnt[tid] = 0;
      const int more = flag[rc & 1];
      lds_barrier();   // the buckets are free (for the next round, or the next tile's operands); thr is visible
      if (more == 0) break;
    }
  }

  if (owner) {
    Cand* o = cand + ((q0 + tid) * splits + split) * k;
    for (int j = 0; j < k; ++j) o[j] = L[tid * k + j];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The distance the library returns, in the direct form from the fp32 rows, by one wave: xv = the query row (element
// j * 64 + lane in xv[j], zero past dim), qq = its squared norm (wave_sum of the lanes' fma chains), y = the bank row.
// Lane-strided fma chains, the fixed butterfly, a correctly rounded sqrtf.  The merge applies it to the rows it returns
// and the radius search decides membership by it: one function, so the two agree bit for bit.
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

// ---------------------------------------------------------------------------------------------------------------------
// merge: one wave per query
template <int GM>
__global__ __launch_bounds__(64) void knn_merge_kernel(const float* __restrict__ queries, const float* __restrict__ bank,
                                                       const Cand* __restrict__ cand, int dim, int k, int splits,
                                                       int metric, int64_t* __restrict__ idx, float* __restrict__ dist,
                                                       const long long* __restrict__ bgrp) {
  __shared__ Cand pool[MAX_SPLITS * MAX_K];
  __shared__ int win[MAX_K];
  __shared__ float wdist[MAX_K];
  const int lane = threadIdx.x;
  const long q = blockIdx.x;
  const float* x = queries + q * dim;
  int64_t* oi = idx + q * k;
  float* od = dist + q * k;

  float xv[MAX_DIM / 64];
  float qq;
  if (!load_query_row(x, dim, lane, xv, qq)) {   // (the selection saw a zero image for this row)
    if (lane < k) {
      oi[lane] = -1;
      od[lane] = __builtin_nanf("");
    }
    return;
  }

  const int P = splits * k;
  for (int c = lane; c < P; c += 64) pool[c] = cand[q * P + c];
  if (lane < MAX_K) win[lane] = EMPTY;
  __syncthreads();
  if constexpr ((GM & GM_ONE) != 0) {
    // one per group: an entry counts only if no pool entry of its group is before it (the splits' bests of one group
    // meet here); the others become empty, and the ranks below are counted among the rest
    __shared__ long long pgrp[MAX_SPLITS * MAX_K_ONE];
    for (int c = lane; c < P; c += 64) {
      const int b = pool[c].i;
      pgrp[c] = b != EMPTY ? bgrp[b] : 0;
    }
    __syncthreads();
    unsigned lose = 0;   // bit j: entry lane + 64 j (P <= 32 * 32: at most 16 per lane)
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
  // the k best of the pool by (score, index): entries are distinct, so the ranks are too
  for (int c = lane; c < P; c += 64) {
    const Cand me = pool[c];
    if (me.i == EMPTY) continue;
    int rank = 0;
    for (int e = 0; e < P; ++e) {
      const Cand o = pool[e];
      rank += before(o.s, o.i, me.s, me.i) ? 1 : 0;
    }
    if (rank < k) win[rank] = me.i;
  }
  __syncthreads();

  // each winner's distance in the direct form, from the fp32 rows
  int nwin = 0;
  for (int j = 0; j < k; ++j) {
    const int b = win[j];
    if (b == EMPTY) break;   // (the ranks are dense: winners fill win[] from the front)
    nwin = j + 1;
    const float dj = direct_distance(xv, qq, bank + (long)b * dim, dim, metric, lane);
    if (lane == 0) wdist[j] = dj;
  }
  __syncthreads();
  if (lane < k) {
    if (lane < nwin) {
      const float d = wdist[lane];
      const int b = win[lane];
      int rank = 0;
      for (int e = 0; e < nwin; ++e) rank += before(wdist[e], win[e], d, b) ? 1 : 0;
      oi[rank] = b;
      od[rank] = d;
    } else {
      oi[lane] = -1;
      od[lane] = __builtin_inff();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// radius search (btsbot_knn_radius_*): the selection's grid and tile walk with a second epilogue,
// "admit if within r" in place of "keep the best k".  A pair is a CANDIDATE when its GEMM-form value
//   Euclidean  g = score + |q|^2            <= lim = r^2 * rel + ctau * (|q|^2 + |b|^2)
//   cosine     g = 1 + score / (2 |q|)      <= lim = r + ctau
// (rel = 1 + 4 (D + 4) u, ctau = 8 (D + 8) u; cosine ctau = 16 (D + 8) u: the margin of 4p, which covers the error
// bounds of this form and of the direct form) -- a superset of the members, decided by the same expression in both
// instantiations.  FILL = false counts a (query, split)'s candidates; FILL = true writes their bank rows into the region
// the scan of the counts gave it, slots handed out by an LDS cursor per query row (the order inside a region is no
// one's business: the lists are sorted afterwards), each slot checked against the region's size.  No list of fixed
// size, nothing of size Q x N.  knn_radius_verify_kernel then applies direct_distance to every candidate.
template <bool FILL, bool EXCL>
__global__ __launch_bounds__(256, 2) void knn_radius_kernel(const unsigned char* __restrict__ qimg,
                                                            const unsigned char* __restrict__ bimg, long Q, int N,
                                                            int dim, int metric, const float* __restrict__ radius,
                                                            float rel, float ctau, long self_offset,
                                                            int tiles_per_split, int splits,
                                                            const long long* __restrict__ qgrp,
                                                            const long long* __restrict__ bgrp, int* counts,
                                                            const long long* __restrict__ offsets,
                                                            int* __restrict__ cand, long long n_cand,
                                                            int* __restrict__ err) {
  constexpr int MI = TileWalk::MI, NI = TileWalk::NI;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* rowcnt = reinterpret_cast<int*>(smem + GEMM_LDS);          // [TQ] candidates so far (FILL: the row's cursor)
  int* rowcap = rowcnt + TQ;                                      // [TQ] FILL: the size of the row's region
  long long* rowbase = reinterpret_cast<long long*>(rowcap + TQ); // [TQ] FILL: where it starts in cand
  long long* tg = reinterpret_cast<long long*>(smem);             // EXCL: [TB] the tile's bank groups (idle operand LDS)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 15, lq = lane >> 4;
  const size_t rec = record_bytes(dim);
  const long q0 = (long)blockIdx.x * TQ;
  const int split = blockIdx.y;
  const int total_tiles = (N + TB - 1) / TB;
  const int t_begin = (int)min((long)split * tiles_per_split, (long)total_tiles);
  const int t_end = (int)min((long)(split + 1) * tiles_per_split, (long)total_tiles);
  const int b_end = (int)min((long)t_end * TB, (long)N);

  if (tid < TQ) {
    rowcnt[tid] = 0;
    if constexpr (FILL) {
      const bool in = q0 + tid < Q;
      rowcap[tid] = in ? counts[(q0 + tid) * splits + split] : 0;
      rowbase[tid] = in ? offsets[(q0 + tid) * splits + split] : 0;
    }
  }

  float sq[MI], qq[MI], qinv[MI], lim[MI];   // the query record's scale, |q|^2, 1 / (2 |q|); r^2 * rel (cosine: r + ctau)
  int selfb[MI];                             // the bank row that IS the query row (never a candidate), -1: none
  long long qg[MI];                          // EXCL: the groups of the lane's four query rows
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const long gq = q0 + wm * 64 + mi * 16 + lrow;
    const float4 h = gq < Q ? *reinterpret_cast<const float4*>(qimg + gq * rec) : make_float4(0.f, 0.f, 0.f, 0.f);
    sq[mi] = h.y;
    qq[mi] = h.z;
    qinv[mi] = h.w;
    const float r = gq < Q ? radius[gq] : -1.f;
    // a row past Q, a non-finite query row (scale 0) and a negative or NaN radius admit nothing
    lim[mi] = h.y != 0.f && r >= 0.f ? (metric == 0 ? (r * r) * rel : r + ctau) : -__builtin_inff();
    const long sb = gq + self_offset;
    selfb[mi] = self_offset >= 0 && sb < N ? (int)sb : -1;
    if constexpr (EXCL) qg[mi] = gq < Q ? qgrp[gq] : 0;
  }

  int n[MI] = {0, 0, 0, 0};
  bool past = false;
  TileWalk w;
  w.init(qimg, bimg, smem, Q, q0, N, dim);
  if (t_begin < t_end) w.gload(t_begin, 0);
  __syncthreads();   // the rows' counters and regions
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int b0 = tile * TB;
    long long gt = 0;   // EXCL: bank row b0 + tid's group, in flight under the products
    if constexpr (EXCL) {
      if (tid < TB && (long)b0 + tid < N) gt = bgrp[(long)b0 + tid];
    }
    f32x4 acc[NI][MI];
    w.products(acc, tile, t_end);
    if constexpr (EXCL) {
      if (tid < TB) tg[tid] = gt;
      lds_barrier();
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float nb[4], sb[4];   // the fragment's bank biases and scales: rows b0 + wn * 64 + ni * 16 + lq * 4 + i
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = b0 + wn * 64 + ni * 16 + lq * 4 + i;
        const float2 h = b < N ? *reinterpret_cast<const float2*>(bimg + (size_t)b * rec)
                               : make_float2(__builtin_inff(), 0.f);
        nb[i] = h.x;
        sb[i] = h.y;
      }
      long long bg[4];
      if constexpr (EXCL) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bg[i] = tg[wn * 64 + ni * 16 + lq * 4 + i];
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gb = b0 + wn * 64 + ni * 16 + lq * 4 + i;
          const float s = fmaf(-(acc[ni][mi][i] * sq[mi]), sb[i], nb[i]);
          float g, l;
          if (metric == 0) {
            g = s + qq[mi];
            l = fmaf(ctau, qq[mi] + nb[i], lim[mi]);
          } else {
            g = fmaf(s, qinv[mi], 1.f);
            l = lim[mi];
          }
          bool in = g <= l && s < __builtin_inff() && gb < b_end && gb != selfb[mi];
          if constexpr (EXCL) in = in && bg[i] != qg[mi];
          if (in) {
            if constexpr (FILL) {
              const int row = wm * 64 + mi * 16 + lrow;
              const int slot = atomicAdd(&rowcnt[row], 1);
              const long long at = rowbase[row] + slot;
              if (slot < rowcap[row] && at >= 0 && at < n_cand) cand[at] = gb;
              else past = true;   // (never, while counts / offsets are the count pass's: the same arithmetic)
            } else {
              ++n[mi];
            }
          }
        }
    }
    if constexpr (EXCL) lds_barrier();   // the groups are read: the next tile's operands may land there
  }

  if constexpr (FILL) {
    if (past) *err = 1;
  } else {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
      if (n[mi] != 0) atomicAdd(&rowcnt[wm * 64 + mi * 16 + lrow], n[mi]);
    __syncthreads();
    if (tid < TQ && q0 + tid < Q) counts[(q0 + tid) * splits + split] = rowcnt[tid];
  }
}

// one wave per candidate in turn: grid (query, Y), wave y takes the query's candidates y, y + Y, ...
__global__ __launch_bounds__(64) void knn_radius_verify_kernel(const float* __restrict__ queries,
                                                               const float* __restrict__ bank,
                                                               const float* __restrict__ radius,
                                                               const long long* __restrict__ offsets, int splits,
                                                               const int* __restrict__ cand, int N, int dim, int metric,
                                                               float* __restrict__ dist,
                                                               unsigned char* __restrict__ keep) {
  const int lane = threadIdx.x;
  const long q = blockIdx.x;
  const long long c1 = offsets[(q + 1) * splits];
  long long c = offsets[q * splits] + blockIdx.y;
  if (c >= c1) return;
  float xv[MAX_DIM / 64];
  float qq;
  const bool ok = load_query_row(queries + q * dim, dim, lane, xv, qq);   // (a row that is not has no candidates)
  const float r = radius[q];
  for (; c < c1; c += gridDim.y) {
    const int b = cand[c];
    const bool have = b >= 0 && b < N;   // (a slot the fill did not reach: it raised the error flag)
    const float d = have ? direct_distance(xv, qq, bank + (long)b * dim, dim, metric, lane) : __builtin_nanf("");
    if (lane == 0) {
      dist[c] = d;
      keep[c] = ok && have && d <= r ? 1 : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// neighbour ranks (btsbot_knn_rank_*): rank[q][c] = the number of eligible bank rows b with
// (direct_distance(q, b), b) before (dist[q][c], targets[q][c]).  The margin of 4p read from both sides: with
// r = dist[q][c] a pair's GEMM-form value g decides
//   g <  lo_c = r^2 * relm - ctau * (|q|^2 + |b|^2)   (cosine: r - ctau)    surely before: the direct form is < r, strictly
//   g <= hi_c = r^2 * rel  + ctau * (|q|^2 + |b|^2)   (cosine: r + ctau)    the band: the direct form decides
// and nothing otherwise (relm = 1 - 4 (D + 4) u; rel and ctau are the radius search's).  The thresholds kernel leaves
// thr[q][c] = (r^2 * relm, r^2 * rel) (cosine: (r - ctau, r + ctau)) and rowlim[q] = the largest second component.
//
// thresholds: one wave per query row, its targets in turn.  dist[q][c] by direct_distance; rank[q][c] = 0, or -1 where
// the target is out of range, not eligible for q, or q is not finite: such a column has thr = (-inf, -inf) and takes no
// part in rowlim, so the tile pass adds nothing to it.
__global__ __launch_bounds__(64) void knn_rank_thresh_kernel(const float* __restrict__ queries,
                                                             const float* __restrict__ bank,
                                                             const unsigned char* __restrict__ bimg, long N, int dim,
                                                             int metric, const long long* __restrict__ targets, int t,
                                                             long self_offset, const long long* __restrict__ qgrp,
                                                             const long long* __restrict__ bgrp, float rel, float relm,
                                                             float ctau, float* __restrict__ dist, int* __restrict__ rank,
                                                             float2* __restrict__ thr, float* __restrict__ rowlim) {
  const int lane = threadIdx.x;
  const long q = blockIdx.x;
  float xv[MAX_DIM / 64];
  float qq;
  const bool qok = load_query_row(queries + q * dim, dim, lane, xv, qq);
  const size_t rec = record_bytes(dim);
  const float ninf = -__builtin_inff();
  float widest = ninf;
  for (int c = 0; c < t; ++c) {
    const long long b = targets[q * t + c];
    const bool in = b >= 0 && b < N;
    // (a bank row is finite exactly when its record's bias is: what the tile pass sees as score < inf)
    const bool fin = in && qok && reinterpret_cast<const float*>(bimg + (size_t)b * rec)[0] < __builtin_inff();
    const float d = fin ? direct_distance(xv, qq, bank + b * dim, dim, metric, lane) : __builtin_nanf("");
    bool el = fin && !(self_offset >= 0 && b == q + self_offset);
    if (el && qgrp != nullptr) el = bgrp[b] != qgrp[q];
    float lo = ninf, hi = ninf;
    if (el) {
      if (metric == 0) {
        hi = (d * d) * rel;
        lo = (d * d) * relm;
      } else {
        hi = d + ctau;
        lo = d - ctau;
      }
      if (!(fabsf(d) <= FLT_MAX)) lo = ninf;   // (an overflowed distance ties with its like: all of it is band)
      widest = fmaxf(widest, hi);
    }
    if (lane == 0) {
      dist[q * t + c] = d;
      rank[q * t + c] = el ? 0 : -1;
      thr[q * t + c] = make_float2(lo, hi);
    }
  }
  if (lane == 0) rowlim[q] = widest;
}

// The tile pass: knn_radius_kernel's walk and pre-filter (one compare of g with the row's widest limit; most of the
// bank ends there), then, for a score that passes, the row's t thresholds from L2.  FILL = false adds the surely-before
// pairs to sure[row][c] in LDS (one global integer atomic per workgroup, row and column at the end) and counts the
// (query, split)'s band pairs -- a pair is ONE band entry however many columns it is in the band of; FILL = true writes
// the band pairs as (bank row, 64-bit mask of these columns) into the region the scan of the counts gave them, every
// slot checked as in the radius fill.  Only integer additions meet across workgroups.
// The scores that pass are few per lane but, in a crowded region, some lane of a wave passes at most of the 64 unrolled
// sites, and a t-step loop run there for the whole wave costs several times the products (measured).  So a
// site only QUEUES its score -- (row, bank row of the tile, g, the margin's scale) in the idle operand LDS -- and after
// the tile all 256 threads share the queue's (score, column) compares, one each, then its entries.  What finds no room
// in the queue is compared on the spot, by the same expressions.
struct RankEnt {
  int rowgb;          // query row of the tile * TB + bank row of the tile
  float g, x;         // the GEMM-form value, |q|^2 + |b|^2 (cosine: 0)
  unsigned mlo, mhi;  // the band mask, met by LDS atomic ORs
};
constexpr int RANK_QCAP = 2048;      // queue entries: 40 KB of the 64 KB operand planes, behind the tile's bank groups
constexpr int RANK_QOFF = 2048;

template <bool FILL, bool EXCL>
__global__ __launch_bounds__(256, 2) void knn_rank_kernel(const unsigned char* __restrict__ qimg,
                                                          const unsigned char* __restrict__ bimg, long Q, int N, int dim,
                                                          int metric, int t, const float2* __restrict__ thr,
                                                          const float* __restrict__ rowlim, float ctau, long self_offset,
                                                          int tiles_per_split, int splits,
                                                          const long long* __restrict__ qgrp,
                                                          const long long* __restrict__ bgrp, int* __restrict__ rank,
                                                          int* counts, const long long* __restrict__ offsets,
                                                          int* __restrict__ cand, unsigned long long* __restrict__ cmask,
                                                          long long n_band, int* __restrict__ err) {
  constexpr int MI = TileWalk::MI, NI = TileWalk::NI;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* rowcnt = reinterpret_cast<int*>(smem + GEMM_LDS);          // [TQ] band pairs so far (FILL: the row's cursor)
  int* rowcap = rowcnt + TQ;                                      // [TQ] FILL: the size of the row's region
  long long* rowbase = reinterpret_cast<long long*>(rowcap + TQ); // [TQ] FILL: where it starts in cand / cmask
  int* qn = reinterpret_cast<int*>(rowbase + TQ);                 // the queue's fill count (16 bytes kept for it)
  int* sure = qn + 4;                                             // [TQ][t] count pass: the surely-before pairs
  long long* tg = reinterpret_cast<long long*>(smem);             // EXCL: [TB] the tile's bank groups (idle operand LDS)
  RankEnt* ent = reinterpret_cast<RankEnt*>(smem + RANK_QOFF);    // [RANK_QCAP] the tile's queue (idle operand LDS)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane & 15, lq = lane >> 4;
  const size_t rec = record_bytes(dim);
  const long q0 = (long)blockIdx.x * TQ;
  const int split = blockIdx.y;
  const int total_tiles = (N + TB - 1) / TB;
  const int t_begin = (int)min((long)split * tiles_per_split, (long)total_tiles);
  const int t_end = (int)min((long)(split + 1) * tiles_per_split, (long)total_tiles);
  const int b_end = (int)min((long)t_end * TB, (long)N);

  if (tid < TQ) {
    rowcnt[tid] = 0;
    if constexpr (FILL) {
      const bool in = q0 + tid < Q;
      rowcap[tid] = in ? counts[(q0 + tid) * splits + split] : 0;
      rowbase[tid] = in ? offsets[(q0 + tid) * splits + split] : 0;
    }
  }
  if (tid == 0) *qn = 0;
  if constexpr (!FILL)
    for (int i = tid; i < TQ * t; i += 256) sure[i] = 0;

  float sq[MI], qq[MI], qinv[MI], lim[MI];   // the query record's scale, |q|^2, 1 / (2 |q|); the row's widest limit
  int selfb[MI];                             // the bank row that IS the query row (never counted), -1: none
  long long qg[MI];                          // EXCL: the groups of the lane's four query rows
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const long gq = q0 + wm * 64 + mi * 16 + lrow;
    const float4 h = gq < Q ? *reinterpret_cast<const float4*>(qimg + gq * rec) : make_float4(0.f, 0.f, 0.f, 0.f);
    sq[mi] = h.y;
    qq[mi] = h.z;
    qinv[mi] = h.w;
    // a row past Q, a non-finite query row and a row without a valid target pass nothing
    lim[mi] = gq < Q && h.y != 0.f ? rowlim[gq] : -__builtin_inff();
    const long sb = gq + self_offset;
    selfb[mi] = self_offset >= 0 && sb < N ? (int)sb : -1;
    if constexpr (EXCL) qg[mi] = gq < Q ? qgrp[gq] : 0;
  }

  int n[MI] = {0, 0, 0, 0};
  bool past = false;
  TileWalk w;
  w.init(qimg, bimg, smem, Q, q0, N, dim);
  if (t_begin < t_end) w.gload(t_begin, 0);
  __syncthreads();   // the rows' counters and regions
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int b0 = tile * TB;
    long long gt = 0;   // EXCL: bank row b0 + tid's group, in flight under the products
    if constexpr (EXCL) {
      if (tid < TB && (long)b0 + tid < N) gt = bgrp[(long)b0 + tid];
    }
    f32x4 acc[NI][MI];
    w.products(acc, tile, t_end);
    if constexpr (EXCL) {
      if (tid < TB) tg[tid] = gt;
      lds_barrier();
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float nb[4], sb[4];   // the fragment's bank biases and scales: rows b0 + wn * 64 + ni * 16 + lq * 4 + i
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = b0 + wn * 64 + ni * 16 + lq * 4 + i;
        const float2 h = b < N ? *reinterpret_cast<const float2*>(bimg + (size_t)b * rec)
                               : make_float2(__builtin_inff(), 0.f);
        nb[i] = h.x;
        sb[i] = h.y;
      }
      long long bg[4];
      if constexpr (EXCL) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bg[i] = tg[wn * 64 + ni * 16 + lq * 4 + i];
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gb = b0 + wn * 64 + ni * 16 + lq * 4 + i;
          const float s = fmaf(-(acc[ni][mi][i] * sq[mi]), sb[i], nb[i]);
          float g, x;   // x: what the margin's tau part scales with (cosine: its tau is in the thresholds)
          if (metric == 0) {
            g = s + qq[mi];
            x = qq[mi] + nb[i];
          } else {
            g = fmaf(s, qinv[mi], 1.f);
            x = 0.f;
          }
          const float l = fmaf(ctau, x, lim[mi]);
          bool in = g <= l && s < __builtin_inff() && gb < b_end && gb != selfb[mi];
          if constexpr (EXCL) in = in && bg[i] != qg[mi];
          if (in) {
            const int row = wm * 64 + mi * 16 + lrow;
            const int slot = atomicAdd(qn, 1);
            if (slot < RANK_QCAP) {
              ent[slot] = RankEnt{row * TB + (gb - b0), g, x, 0u, 0u};
              continue;
            }
            const float2* th = thr + (q0 + row) * t;
            unsigned long long band = 0;
#pragma unroll 1
            for (int c = 0; c < t; ++c) {
              const float2 lh = th[c];
              if (g < fmaf(-ctau, x, lh.x)) {
                if constexpr (!FILL) atomicAdd(&sure[row * t + c], 1);
              } else if (g <= fmaf(ctau, x, lh.y)) {
                band |= 1ull << c;
              }
            }
            if (band != 0) {
              if constexpr (FILL) {
                const int slot = atomicAdd(&rowcnt[row], 1);
                const long long at = rowbase[row] + slot;
                if (slot < rowcap[row] && at >= 0 && at < n_band) {
                  cand[at] = gb;
                  cmask[at] = band;
                } else {
                  past = true;   // (never, while counts / offsets are the count pass's: the same arithmetic)
                }
              } else {
                ++n[mi];
              }
            }
          }
        }
    }
    lds_barrier();   // the queue is complete (and the groups are read)
    const int nq = min(*qn, RANK_QCAP);
    for (int w = tid; w < nq * t; w += 256) {   // one (score, column) compare per thread and step
      const int e = w / t, c = w - e * t;
      const int row = ent[e].rowgb / TB;
      const float g = ent[e].g, x = ent[e].x;
      const float2 lh = thr[(q0 + row) * t + c];
      if (g < fmaf(-ctau, x, lh.x)) {
        if constexpr (!FILL) atomicAdd(&sure[row * t + c], 1);
      } else if (g <= fmaf(ctau, x, lh.y)) {
        atomicOr(c < 32 ? &ent[e].mlo : &ent[e].mhi, 1u << (c & 31));
      }
    }
    lds_barrier();   // the masks are complete
    for (int e = tid; e < nq; e += 256) {
      const unsigned long long band = (unsigned long long)ent[e].mhi << 32 | ent[e].mlo;
      if (band == 0) continue;
      const int row = ent[e].rowgb / TB;
      const int slot = atomicAdd(&rowcnt[row], 1);
      if constexpr (FILL) {
        const long long at = rowbase[row] + slot;
        if (slot < rowcap[row] && at >= 0 && at < n_band) {
          cand[at] = b0 + ent[e].rowgb % TB;
          cmask[at] = band;
        } else {
          past = true;
        }
      }
    }
    lds_barrier();   // the queue is read: the next tile's operands may land there
    if (tid == 0) *qn = 0;   // (the next tile's first push is behind the barriers of its products)
  }

  if constexpr (FILL) {
    if (past) *err = 1;
  } else {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
      if (n[mi] != 0) atomicAdd(&rowcnt[wm * 64 + mi * 16 + lrow], n[mi]);
    __syncthreads();
    if (tid < TQ && q0 + tid < Q) counts[(q0 + tid) * splits + split] = rowcnt[tid];
    for (int i = tid; i < TQ * t; i += 256) {
      const int v = sure[i];
      if (v != 0) atomicAdd(&rank[q0 * t + i], v);   // (row q0 + i / t, column i % t; a row past Q has none)
    }
  }
}

// one wave per band entry in turn (the radius verify's grid): the pair's direct-form distance once, then lane c adds
// before((d, b), (dist[q][c], targets[q][c])) to rank[q][c] for the columns of the entry's mask
__global__ __launch_bounds__(64) void knn_rank_verify_kernel(const float* __restrict__ queries,
                                                             const float* __restrict__ bank,
                                                             const long long* __restrict__ targets, int t,
                                                             const float* __restrict__ dist,
                                                             const long long* __restrict__ offsets, int splits,
                                                             const int* __restrict__ cand,
                                                             const unsigned long long* __restrict__ cmask, int N,
                                                             int dim, int metric, int* __restrict__ rank) {
  const int lane = threadIdx.x;
  const long q = blockIdx.x;
  const long long c1 = offsets[(q + 1) * splits];
  long long c = offsets[q * splits] + blockIdx.y;
  if (c >= c1) return;
  float xv[MAX_DIM / 64];
  float qq;
  (void)load_query_row(queries + q * dim, dim, lane, xv, qq);   // (a row that is not finite has no band entries)
  const bool col = lane < t;
  const float dc = col ? dist[q * t + lane] : 0.f;
  const long long tc = col ? targets[q * t + lane] : 0;
  int add = 0;
  for (; c < c1; c += gridDim.y) {
    const int b = cand[c];
    if (b < 0 || b >= N) continue;   // (a slot the fill did not reach: it raised the error flag)
    const float d = direct_distance(xv, qq, bank + (long)b * dim, dim, metric, lane);
    if (col && (cmask[c] >> lane & 1ull) != 0 && before(d, b, dc, (int)tc)) ++add;
  }
  if (add != 0) atomicAdd(&rank[q * t + lane], add);
}

int check_shape(const char* who, int64_t n_query, int64_t n_bank, int dim, int k) {
  if (dim < 1 || dim > MAX_DIM || k < 1 || k > MAX_K || n_query < 0 || n_bank < 0 || n_bank > 0x7fffffffLL ||
      n_query > 0x7fffffffLL) {
    btsbot_set_error("%s: need 1 <= dim <= %d, 1 <= k <= %d, 0 <= n_bank, n_query < 2^31 (dim=%d k=%d n_bank=%lld "
                     "n_query=%lld)", who, MAX_DIM, MAX_K, dim, k, (long long)n_bank, (long long)n_query);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

int auto_splits(int64_t n_query, int64_t n_bank) {
  const int64_t qt = (n_query + TQ - 1) / TQ, bt = (n_bank + TB - 1) / TB;
  if (qt < 1 || bt < 1) return 1;
  // two workgroups per CU (256 CUs) where the bank has the tiles for it
  int64_t s = (512 + qt - 1) / qt;
  s = s > bt ? bt : s;
  s = s > MAX_SPLITS ? MAX_SPLITS : s;
  return (int)(s < 1 ? 1 : s);
}

size_t image_bytes(int64_t rows, int dim) { return ((size_t)rows * record_bytes(dim) + 255) & ~(size_t)255; }

}  // namespace

extern "C" int64_t btsbot_knn_bank_bytes(int64_t n_bank, int dim) {
  if (check_shape("btsbot_knn_bank_bytes", 0, n_bank, dim, 1) != BTSBOT_OK) return BTSBOT_ERR_INVALID_ARG;
  return (int64_t)((size_t)n_bank * record_bytes(dim));
}

extern "C" int btsbot_knn_pack_bank(const float* rows, int64_t first_row, int64_t n_rows, int dim, int metric,
                                    void* packed, int64_t n_bank_capacity, void* stream) {
  const int s = check_shape("btsbot_knn_pack_bank", 0, n_bank_capacity, dim, 1);
  if (s != BTSBOT_OK) return s;
  if (metric != BTSBOT_KNN_EUCLIDEAN && metric != BTSBOT_KNN_COSINE) {
    btsbot_set_error("btsbot_knn_pack_bank: metric %d", metric);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (first_row < 0 || n_rows < 0 || first_row > n_bank_capacity || n_rows > n_bank_capacity - first_row) {
    btsbot_set_error("btsbot_knn_pack_bank: rows [%lld, %lld + %lld) do not fit a bank of %lld", (long long)first_row,
                     (long long)first_row, (long long)n_rows, (long long)n_bank_capacity);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_rows == 0) return BTSBOT_OK;
  if (rows == nullptr || packed == nullptr || ((uintptr_t)packed & 15) != 0) {
    btsbot_set_error("btsbot_knn_pack_bank: NULL rows / packed, or packed not 16-byte aligned");
    return BTSBOT_ERR_INVALID_ARG;
  }
  unsigned char* out = reinterpret_cast<unsigned char*>(packed) + (size_t)first_row * record_bytes(dim);
  hipLaunchKernelGGL(knn_pack_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rows,
                     (long)n_rows, dim, metric == BTSBOT_KNN_COSINE ? MODE_BANK_COS : MODE_BANK_L2, out);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_knn_splits(int64_t n_query, int64_t n_bank, int dim, int k) {
  const int s = check_shape("btsbot_knn_splits", n_query, n_bank, dim, k);
  if (s != BTSBOT_OK) return s;
  return auto_splits(n_query, n_bank);
}

extern "C" int64_t btsbot_knn_workspace(int64_t n_query, int64_t n_bank, int dim, int k, int splits) {
  if (check_shape("btsbot_knn_workspace", n_query, n_bank, dim, k) != BTSBOT_OK) return BTSBOT_ERR_INVALID_ARG;
  if (splits < 0 || splits > MAX_SPLITS) {
    btsbot_set_error("btsbot_knn_workspace: splits=%d must be 0 (the library's choice) .. %d", splits, MAX_SPLITS);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (splits == 0) splits = auto_splits(n_query, n_bank);
  return (int64_t)(image_bytes(n_query, dim) + (size_t)n_query * splits * k * sizeof(Cand));
}

// With one entry per group the groups of the list entries follow the candidates: [query tiles][splits][k][TQ] int64
extern "C" int64_t btsbot_knn_workspace_grouped(int64_t n_query, int64_t n_bank, int dim, int k, int splits, int flags) {
  const int64_t base = btsbot_knn_workspace(n_query, n_bank, dim, k, splits);
  if (base < 0 || (flags & GM_ONE) == 0) return base;
  if (splits == 0) splits = auto_splits(n_query, n_bank);
  return base + (int64_t)(((size_t)n_query + TQ - 1) / TQ * TQ * splits * k * sizeof(long long));
}

namespace {

// The launches of btsbot_knn_query (GM = 0) and btsbot_knn_query_grouped, one instantiation per group mode
template <int GM>
int launch_query(const float* queries, int64_t n_query, const float* bank, const unsigned char* packed, int64_t n_bank,
                 int dim, int k, int metric, int64_t self_offset, int splits, int64_t* idx, float* dist,
                 unsigned char* qimg, Cand* cand, const long long* qgrp, const long long* bgrp, hipStream_t st) {
  // (the candidates end on a multiple of 8 bytes behind the 256-byte aligned query image)
  long long* lgrp = reinterpret_cast<long long*>(cand + (size_t)n_query * splits * k);
  hipLaunchKernelGGL(knn_pack_kernel, dim3((unsigned)((n_query + 3) / 4)), dim3(256), 0, st, queries, (long)n_query, dim,
                     (int)MODE_QUERY, qimg);
  LAUNCH_CHECK();

  const int total_tiles = (int)((n_bank + TB - 1) / TB);
  const int tps = (total_tiles + splits - 1) / splits;
  // 64 KB of operands + 1 KB of lists per k: two workgroups per CU up to k = 16, in every group mode
  static DevOnce attr;
  if (attr.need()) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_select_kernel<GM>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS + TQ * MAX_K * (int)sizeof(Cand)));
    attr.done();
  }
  hipLaunchKernelGGL(knn_select_kernel<GM>, dim3((unsigned)((n_query + TQ - 1) / TQ), (unsigned)splits), dim3(256),
                     GEMM_LDS + TQ * k * (int)sizeof(Cand), st, qimg, packed, (long)n_query, (int)n_bank, dim, k, (long)self_offset,
                     tps, splits, cand, qgrp, bgrp, lgrp);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_merge_kernel<(GM & GM_ONE)>, dim3((unsigned)n_query), dim3(64), 0, st, queries, bank,
                     (const Cand*)cand, dim, k, splits, metric, idx, dist, bgrp);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int query_checked(const char* who, const float* queries, int64_t n_query, const float* bank, const void* packed,
                  int64_t n_bank, int dim, int k, int metric, int64_t self_offset, int splits, int64_t* idx, float* dist,
                  void* workspace, int64_t workspace_bytes, const int64_t* query_group, const int64_t* bank_group,
                  int flags, void* stream) {
  const int s = check_shape(who, n_query, n_bank, dim, k);
  if (s != BTSBOT_OK) return s;
  if (metric != BTSBOT_KNN_EUCLIDEAN && metric != BTSBOT_KNN_COSINE) {
    btsbot_set_error("%s: metric %d", who, metric);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (splits < 0 || splits > MAX_SPLITS) {
    btsbot_set_error("%s: splits=%d must be 0 (the library's choice) .. %d", who, splits, MAX_SPLITS);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((flags & ~(GM_EXCLUDE | GM_ONE)) != 0) {
    btsbot_set_error("%s: flags=%d holds bits other than BTSBOT_KNN_EXCLUDE_SAME | BTSBOT_KNN_ONE_PER_GROUP", who, flags);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((flags & GM_ONE) != 0 && k > MAX_K_ONE) {
    btsbot_set_error("%s: k=%d, but BTSBOT_KNN_ONE_PER_GROUP holds k <= %d (the merge keeps its pool's groups on chip)", who, k,
                     MAX_K_ONE);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query == 0) return BTSBOT_OK;
  if (splits == 0) splits = auto_splits(n_query, n_bank);
  const int64_t need = btsbot_knn_workspace_grouped(n_query, n_bank, dim, k, splits, flags);
  if (queries == nullptr || idx == nullptr || dist == nullptr || workspace == nullptr ||
      (n_bank > 0 && (bank == nullptr || packed == nullptr))) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (((flags & GM_EXCLUDE) != 0 && query_group == nullptr) || (flags != 0 && n_bank > 0 && bank_group == nullptr)) {
    btsbot_set_error("%s: flags=%d need bank_group (and BTSBOT_KNN_EXCLUDE_SAME query_group), got NULL", who, flags);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (workspace_bytes < need || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)packed & 15) != 0) {
    btsbot_set_error("%s: workspace of %lld bytes (need %lld), or workspace / packed not 16-byte aligned", who,
                     (long long)workspace_bytes, (long long)need);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned char* qimg = reinterpret_cast<unsigned char*>(workspace);
  Cand* cand = reinterpret_cast<Cand*>(qimg + image_bytes(n_query, dim));
  const unsigned char* pk = reinterpret_cast<const unsigned char*>(packed);
  const long long* qg = reinterpret_cast<const long long*>(query_group);
  const long long* bg = reinterpret_cast<const long long*>(bank_group);
#define KNN_GO(GM) \
  launch_query<GM>(queries, n_query, bank, pk, n_bank, dim, k, metric, self_offset, splits, idx, dist, qimg, cand, qg, bg, st)
  switch (flags) {
    case 0: return KNN_GO(0);
    case GM_EXCLUDE: return KNN_GO(GM_EXCLUDE);
    case GM_ONE: return KNN_GO(GM_ONE);
    default: return KNN_GO(GM_EXCLUDE | GM_ONE);
  }
#undef KNN_GO
}

}  // namespace

extern "C" int btsbot_knn_query(const float* queries, int64_t n_query, const float* bank, const void* packed,
                                int64_t n_bank, int dim, int k, int metric, int64_t self_offset, int splits,
                                int64_t* idx, float* dist, void* workspace, int64_t workspace_bytes, void* stream) {
  return query_checked("btsbot_knn_query", queries, n_query, bank, packed, n_bank, dim, k, metric, self_offset, splits,
                       idx, dist, workspace, workspace_bytes, nullptr, nullptr, 0, stream);
}

extern "C" int btsbot_knn_query_grouped(const float* queries, int64_t n_query, const float* bank, const void* packed,
                                        int64_t n_bank, int dim, int k, int metric, int64_t self_offset, int splits,
                                        int64_t* idx, float* dist, void* workspace, int64_t workspace_bytes,
                                        void* stream, const int64_t* query_group, const int64_t* bank_group, int flags) {
  return query_checked("btsbot_knn_query_grouped", queries, n_query, bank, packed, n_bank, dim, k, metric, self_offset,
                       splits, idx, dist, workspace, workspace_bytes, query_group, bank_group, flags, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// radius search: the entry points
namespace {

struct RadiusArgs {
  const float* queries;
  int64_t n_query;
  const void* packed;
  int64_t n_bank;
  int dim, metric;
  const float* radius;
  int64_t self_offset;
  int splits;
  const int64_t* query_group;
  const int64_t* bank_group;
  int flags;
  void* workspace;
  int64_t workspace_bytes;
};

int radius_checked(const char* who, const RadiusArgs& a) {
  TRY(check_shape(who, a.n_query, a.n_bank, a.dim, 1));
  if (a.metric != BTSBOT_KNN_EUCLIDEAN && a.metric != BTSBOT_KNN_COSINE) {
    btsbot_set_error("%s: metric %d", who, a.metric);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (a.splits < 1 || a.splits > MAX_SPLITS) {
    btsbot_set_error("%s: splits=%d must be 1 .. %d", who, a.splits, MAX_SPLITS);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((a.flags & ~GM_EXCLUDE) != 0) {
    btsbot_set_error("%s: flags=%d, only 0 and BTSBOT_KNN_EXCLUDE_SAME are radius modes", who, a.flags);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (a.n_query == 0) return BTSBOT_OK;
  if (a.queries == nullptr || a.radius == nullptr || a.workspace == nullptr || (a.n_bank > 0 && a.packed == nullptr)) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (a.flags != 0 && (a.query_group == nullptr || (a.n_bank > 0 && a.bank_group == nullptr))) {
    btsbot_set_error("%s: BTSBOT_KNN_EXCLUDE_SAME needs query_group and bank_group, got NULL", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int64_t need = (int64_t)image_bytes(a.n_query, a.dim);
  if (a.workspace_bytes < need || ((uintptr_t)a.workspace & 15) != 0 || ((uintptr_t)a.packed & 15) != 0) {
    btsbot_set_error("%s: workspace of %lld bytes (need %lld), or workspace / packed not 16-byte aligned", who,
                     (long long)a.workspace_bytes, (long long)need);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

// query pack + one tile pass (FILL = false: counts are written; true: counts and offsets are read, cand is written)
template <bool FILL, bool EXCL>
int launch_radius(const RadiusArgs& a, int* counts, const int64_t* offsets, int* cand, int64_t n_cand, int* err,
                  hipStream_t st) {
  unsigned char* qimg = reinterpret_cast<unsigned char*>(a.workspace);
  hipLaunchKernelGGL(knn_pack_kernel, dim3((unsigned)((a.n_query + 3) / 4)), dim3(256), 0, st, a.queries, (long)a.n_query,
                     a.dim, (int)MODE_QUERY, qimg);
  LAUNCH_CHECK();
  constexpr int LDS = GEMM_LDS + TQ * 16;   // operands + per query row: counter, region size, region start
  static DevOnce attr;
  if (attr.need()) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_radius_kernel<FILL, EXCL>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    attr.done();
  }
  // the margin of DESIGN.md 4p; u = 2^-24
  const float u = 5.9604644775390625e-8f;
  const bool cosine = a.metric == BTSBOT_KNN_COSINE;
  const float rel = 1.f + 4.f * (float)(a.dim + 4) * u;
  const float ctau = (cosine ? 16.f : 8.f) * (float)(a.dim + 8) * u;
  const int total_tiles = (int)((a.n_bank + TB - 1) / TB);
  const int tps = (total_tiles + a.splits - 1) / a.splits;
  hipLaunchKernelGGL((knn_radius_kernel<FILL, EXCL>), dim3((unsigned)((a.n_query + TQ - 1) / TQ), (unsigned)a.splits),
                     dim3(256), LDS, st, (const unsigned char*)qimg, reinterpret_cast<const unsigned char*>(a.packed),
                     (long)a.n_query, (int)a.n_bank, a.dim, a.metric, a.radius, rel, ctau, (long)a.self_offset, tps,
                     a.splits, reinterpret_cast<const long long*>(a.query_group),
                     reinterpret_cast<const long long*>(a.bank_group), counts,
                     reinterpret_cast<const long long*>(offsets), cand, (long long)n_cand, err);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

}  // namespace

extern "C" int64_t btsbot_knn_radius_workspace(int64_t n_query, int dim) {
  if (check_shape("btsbot_knn_radius_workspace", n_query, 0, dim, 1) != BTSBOT_OK) return BTSBOT_ERR_INVALID_ARG;
  return (int64_t)image_bytes(n_query, dim);
}

extern "C" int btsbot_knn_radius_count(const float* queries, int64_t n_query, const void* packed, int64_t n_bank, int dim,
                                       int metric, const float* radius, int64_t self_offset, int splits,
                                       const int64_t* query_group, const int64_t* bank_group, int flags, int32_t* counts,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
  const RadiusArgs a{queries, n_query, packed, n_bank, dim, metric, radius, self_offset, splits, query_group, bank_group,
                     flags, workspace, workspace_bytes};
  TRY(radius_checked("btsbot_knn_radius_count", a));
  if (n_query == 0) return BTSBOT_OK;
  if (counts == nullptr) {
    btsbot_set_error("btsbot_knn_radius_count: NULL counts");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  return flags != 0 ? launch_radius<false, true>(a, counts, nullptr, nullptr, 0, nullptr, st)
                    : launch_radius<false, false>(a, counts, nullptr, nullptr, 0, nullptr, st);
}

extern "C" int btsbot_knn_radius_fill(const float* queries, int64_t n_query, const float* bank, const void* packed,
                                      int64_t n_bank, int dim, int metric, const float* radius, int64_t self_offset,
                                      int splits, const int64_t* query_group, const int64_t* bank_group, int flags,
                                      const int32_t* counts, const int64_t* offsets, int64_t n_cand, int32_t* cand,
                                      float* dist, uint8_t* keep, int32_t* error_flag, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  const RadiusArgs a{queries, n_query, packed, n_bank, dim, metric, radius, self_offset, splits, query_group, bank_group,
                     flags, workspace, workspace_bytes};
  TRY(radius_checked("btsbot_knn_radius_fill", a));
  if (n_cand < 0) {
    btsbot_set_error("btsbot_knn_radius_fill: n_cand=%lld", (long long)n_cand);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query == 0 || n_cand == 0) return BTSBOT_OK;
  if (bank == nullptr || counts == nullptr || offsets == nullptr || cand == nullptr || dist == nullptr || keep == nullptr ||
      error_flag == nullptr) {
    btsbot_set_error("btsbot_knn_radius_fill: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  int* cnt = const_cast<int*>(counts);   // (read only by the FILL instantiation)
  TRY(flags != 0 ? (launch_radius<true, true>(a, cnt, offsets, cand, n_cand, error_flag, st))
                 : (launch_radius<true, false>(a, cnt, offsets, cand, n_cand, error_flag, st)));
  // enough waves per query that a crowded row does not serialise: its candidates are shared out over Y waves
  const int64_t per = (n_cand + n_query - 1) / n_query;
  const unsigned Y = (unsigned)(per <= 32 ? 1 : per >= 32 * 64 ? 64 : (per + 31) / 32);
  hipLaunchKernelGGL(knn_radius_verify_kernel, dim3((unsigned)n_query, Y), dim3(64), 0, st, queries, bank, radius,
                     reinterpret_cast<const long long*>(offsets), splits, (const int*)cand, (int)n_bank, dim, metric, dist,
                     keep);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// neighbour ranks: the entry points
namespace {

struct RankArgs {
  const float* queries;
  int64_t n_query;
  const float* bank;
  const void* packed;
  int64_t n_bank;
  int dim, metric;
  const int64_t* targets;
  int n_targets;
  int64_t self_offset;
  int splits;
  const int64_t* query_group;
  const int64_t* bank_group;
  int flags;
  void* workspace;
  int64_t workspace_bytes;
};

// the workspace: the packed query rows, thr float2 [n_query][n_targets], rowlim float [n_query]
size_t rank_thr_bytes(int64_t n_query, int n_targets) {
  return ((size_t)n_query * n_targets * sizeof(float2) + 255) & ~(size_t)255;
}

int rank_checked(const char* who, const RankArgs& a) {
  TRY(check_shape(who, a.n_query, a.n_bank, a.dim, a.n_targets));   // (1 <= n_targets <= 64 is k's range)
  if (a.metric != BTSBOT_KNN_EUCLIDEAN && a.metric != BTSBOT_KNN_COSINE) {
    btsbot_set_error("%s: metric %d", who, a.metric);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (a.splits < 1 || a.splits > MAX_SPLITS) {
    btsbot_set_error("%s: splits=%d must be 1 .. %d", who, a.splits, MAX_SPLITS);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((a.flags & ~GM_EXCLUDE) != 0) {
    btsbot_set_error("%s: flags=%d, only 0 and BTSBOT_KNN_EXCLUDE_SAME are rank modes", who, a.flags);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (a.n_query == 0) return BTSBOT_OK;
  if (a.queries == nullptr || a.targets == nullptr || a.workspace == nullptr ||
      (a.n_bank > 0 && (a.bank == nullptr || a.packed == nullptr))) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (a.flags != 0 && (a.query_group == nullptr || (a.n_bank > 0 && a.bank_group == nullptr))) {
    btsbot_set_error("%s: BTSBOT_KNN_EXCLUDE_SAME needs query_group and bank_group, got NULL", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int64_t need = btsbot_knn_rank_workspace(a.n_query, a.dim, a.n_targets);
  if (a.workspace_bytes < need || ((uintptr_t)a.workspace & 15) != 0 || ((uintptr_t)a.packed & 15) != 0) {
    btsbot_set_error("%s: workspace of %lld bytes (need %lld), or workspace / packed not 16-byte aligned", who,
                     (long long)a.workspace_bytes, (long long)need);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

// the margin of DESIGN.md 4p / 4r; u = 2^-24
struct RankMargin {
  float rel, relm, ctau;
  RankMargin(int dim, int metric) {
    const float u = 5.9604644775390625e-8f;
    rel = 1.f + 4.f * (float)(dim + 4) * u;
    relm = 1.f - 4.f * (float)(dim + 4) * u;
    ctau = (metric == BTSBOT_KNN_COSINE ? 16.f : 8.f) * (float)(dim + 8) * u;
  }
};

template <bool FILL, bool EXCL>
int launch_rank(const RankArgs& a, int* rank, int* counts, const int64_t* offsets, int* cand, uint64_t* cmask,
                int64_t n_band, int* err, hipStream_t st) {
  unsigned char* qimg = reinterpret_cast<unsigned char*>(a.workspace);
  const float2* thr = reinterpret_cast<const float2*>(qimg + image_bytes(a.n_query, a.dim));
  const float* rowlim = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(thr) +
                                                       rank_thr_bytes(a.n_query, a.n_targets));
  // operands + per query row: counter, region size, region start; the queue's count; the count pass: + its
  // n_targets sure counts per row
  const int lds = GEMM_LDS + TQ * 16 + 16 + (FILL ? 0 : TQ * a.n_targets * (int)sizeof(int));
  static DevOnce attr;
  if (attr.need()) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_rank_kernel<FILL, EXCL>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                GEMM_LDS + TQ * 16 + 16 + (FILL ? 0 : TQ * MAX_K * (int)sizeof(int))));
    attr.done();
  }
  const RankMargin m(a.dim, a.metric);
  const int total_tiles = (int)((a.n_bank + TB - 1) / TB);
  const int tps = (total_tiles + a.splits - 1) / a.splits;
  hipLaunchKernelGGL((knn_rank_kernel<FILL, EXCL>), dim3((unsigned)((a.n_query + TQ - 1) / TQ), (unsigned)a.splits),
                     dim3(256), lds, st, (const unsigned char*)qimg, reinterpret_cast<const unsigned char*>(a.packed),
                     (long)a.n_query, (int)a.n_bank, a.dim, a.metric, a.n_targets, thr, rowlim, m.ctau,
                     (long)a.self_offset, tps, a.splits, reinterpret_cast<const long long*>(a.query_group),
                     reinterpret_cast<const long long*>(a.bank_group), rank, counts,
                     reinterpret_cast<const long long*>(offsets), cand, reinterpret_cast<unsigned long long*>(cmask),
                     (long long)n_band, err);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

}  // namespace

extern "C" int64_t btsbot_knn_rank_workspace(int64_t n_query, int dim, int n_targets) {
  if (check_shape("btsbot_knn_rank_workspace", n_query, 0, dim, n_targets) != BTSBOT_OK) return BTSBOT_ERR_INVALID_ARG;
  return (int64_t)(image_bytes(n_query, dim) + rank_thr_bytes(n_query, n_targets) + (size_t)n_query * sizeof(float));
}

extern "C" int btsbot_knn_rank_count(const float* queries, int64_t n_query, const float* bank, const void* packed,
                                     int64_t n_bank, int dim, int metric, const int64_t* targets, int n_targets,
                                     int64_t self_offset, int splits, const int64_t* query_group,
                                     const int64_t* bank_group, int flags, float* dist, int32_t* rank, int32_t* counts,
                                     void* workspace, int64_t workspace_bytes, void* stream) {
  const RankArgs a{queries, n_query, bank, packed, n_bank, dim, metric, targets, n_targets, self_offset, splits,
                   query_group, bank_group, flags, workspace, workspace_bytes};
  TRY(rank_checked("btsbot_knn_rank_count", a));
  if (n_query == 0) return BTSBOT_OK;
  if (dist == nullptr || rank == nullptr || counts == nullptr) {
    btsbot_set_error("btsbot_knn_rank_count: NULL dist / rank / counts");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned char* qimg = reinterpret_cast<unsigned char*>(workspace);
  float2* thr = reinterpret_cast<float2*>(qimg + image_bytes(n_query, dim));
  float* rowlim = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(thr) + rank_thr_bytes(n_query, n_targets));
  hipLaunchKernelGGL(knn_pack_kernel, dim3((unsigned)((n_query + 3) / 4)), dim3(256), 0, st, queries, (long)n_query, dim,
                     (int)MODE_QUERY, qimg);
  LAUNCH_CHECK();
  const RankMargin m(dim, metric);
  hipLaunchKernelGGL(knn_rank_thresh_kernel, dim3((unsigned)n_query), dim3(64), 0, st, queries, bank,
                     reinterpret_cast<const unsigned char*>(packed), (long)n_bank, dim, metric,
                     reinterpret_cast<const long long*>(targets), n_targets, (long)self_offset,
                     flags != 0 ? reinterpret_cast<const long long*>(query_group) : nullptr,
                     reinterpret_cast<const long long*>(bank_group), m.rel, m.relm, m.ctau, dist, rank, thr, rowlim);
  LAUNCH_CHECK();
  if (n_bank == 0) {   // every target is out of range: rank -1, dist NaN, no band
    HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_query * splits * sizeof(int), st));
    return BTSBOT_OK;
  }
  return flags != 0 ? launch_rank<false, true>(a, rank, counts, nullptr, nullptr, nullptr, 0, nullptr, st)
                    : launch_rank<false, false>(a, rank, counts, nullptr, nullptr, nullptr, 0, nullptr, st);
}

extern "C" int btsbot_knn_rank_fill(const float* queries, int64_t n_query, const float* bank, const void* packed,
                                    int64_t n_bank, int dim, int metric, const int64_t* targets, int n_targets,
                                    int64_t self_offset, int splits, const int64_t* query_group,
                                    const int64_t* bank_group, int flags, const float* dist, int32_t* rank,
                                    const int32_t* counts, const int64_t* offsets, int64_t n_band, int32_t* cand,
                                    uint64_t* cand_mask, int32_t* error_flag, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
  const RankArgs a{queries, n_query, bank, packed, n_bank, dim, metric, targets, n_targets, self_offset, splits,
                   query_group, bank_group, flags, workspace, workspace_bytes};
  TRY(rank_checked("btsbot_knn_rank_fill", a));
  if (n_band < 0) {
    btsbot_set_error("btsbot_knn_rank_fill: n_band=%lld", (long long)n_band);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query == 0 || n_band == 0 || n_bank == 0) return BTSBOT_OK;
  if (dist == nullptr || rank == nullptr || counts == nullptr || offsets == nullptr || cand == nullptr ||
      cand_mask == nullptr || error_flag == nullptr) {
    btsbot_set_error("btsbot_knn_rank_fill: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  int* cnt = const_cast<int*>(counts);   // (read only by the FILL instantiation)
  TRY(flags != 0 ? (launch_rank<true, true>(a, rank, cnt, offsets, cand, cand_mask, n_band, error_flag, st))
                 : (launch_rank<true, false>(a, rank, cnt, offsets, cand, cand_mask, n_band, error_flag, st)));
  // enough waves per query that a crowded row does not serialise, as the radius verify
  const int64_t per = (n_band + n_query - 1) / n_query;
  const unsigned Y = (unsigned)(per <= 32 ? 1 : per >= 32 * 64 ? 64 : (per + 31) / 32);
  hipLaunchKernelGGL(knn_rank_verify_kernel, dim3((unsigned)n_query, Y), dim3(64), 0, st, queries, bank,
                     reinterpret_cast<const long long*>(targets), n_targets, dist,
                     reinterpret_cast<const long long*>(offsets), splits, (const int*)cand,
                     reinterpret_cast<const unsigned long long*>(cand_mask), (int)n_bank, dim, metric, rank);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
