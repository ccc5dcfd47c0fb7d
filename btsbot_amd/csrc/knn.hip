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
// (its largest magnitude lands in [2^14, 2^15): device_math.h, split_exp), three v_mfma_f32_16x16x32_f16 per product, small
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
// knn_tile.h holds what this file shares with the radius search (knn_radius.hip) and the neighbour ranks
// (knn_rank.hip): the record, the tile walk, direct_distance() -- the one function that computes a returned distance --
// and the host helpers defined at the end of this file.
#include "knn_tile.h"

namespace {

constexpr int BCAP = 8;             // candidates a query row's bucket holds per round
enum { MODE_BANK_L2 = 0, MODE_BANK_COS = 1, MODE_QUERY = 2 };

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
// selection: the lists and their offers (offer, offer_one) are knn_tile.h's, shared with the listed pass of ivf.hip
template <int GM>
__global__ __launch_bounds__(256, 2) void knn_select_kernel(const unsigned char* __restrict__ qimg,
                                                            const unsigned char* __restrict__ bimg, long Q, int N,
                                                            int dim, int k, long self_offset, int tiles_per_split,
                                                            int splits, Cand* __restrict__ cand,
                                                            const long long* __restrict__ qgrp,
                                                            const long long* __restrict__ bgrp,
                                                            long long* __restrict__ lgrp) {
  constexpr int MI = TileWalk::MI, NI = TileWalk::NI;
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

  const int tid = threadIdx.x;
  const LanePos p;
  const int dp = padded_dim(dim);
  const size_t rec = record_bytes(dim);
  const long q0 = (long)blockIdx.x * TQ;
  const SplitRange sr(N, tiles_per_split);
  const int nk = (dp + BK - 1) / BK;

  // This kernel shares LanePos, SplitRange, the operand loads and their LDS store (tile_gload, tile_sstore),
  // load_tile_group and tile_score with the radius and rank passes, and keeps its own text of the rest of a tile pass --
  // the query rows' header, the product loop, the fragment's biases, scales and groups, the eligibility term (QueryRows,
  // TileWalk::products, frag_bias_scale, frag_groups, eligible) -- because each of these moves its allocation.  Scratch
  // bytes per lane for GM = 0 / 1 / 2 / 3: this text 172 / 280 / 184 / 316, as ever.  All of it on the shared pieces:
  // 144 / 200 / 160 / 212, every one lower, and 2 % slower (42.1 against 41.3 ms per query call at N = 1,000,000,
  // Q = 8,192, D = 528, k = 15, twice each).  The product loop shared too: 156 / 288 / 176 / 292; the plain struct: 156 /
  // 288 / 180 / 300 -- both above 280 for GM = 1.  DESIGN.md 4s.

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
    const long gq = p.gq(q0, mi);
    sq[mi] = gq < Q ? reinterpret_cast<const float*>(qimg + gq * rec)[1] : 0.f;
    const long sb = gq + self_offset;
    selfb[mi] = self_offset >= 0 && sb < N ? (int)sb : -1;
  }
  long long qg[MI];   // GM & GM_EXCLUDE: the groups of the lane's four query rows
  if constexpr ((GM & GM_EXCLUDE) != 0) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const long gq = p.gq(q0, mi);
      qg[mi] = gq < Q ? qgrp[gq] : 0;   // (a row past Q never has a candidate)
    }
  }

  uint4 qh[CH], ql[CH], bh[CH], bl[CH];
  auto gload = [&](int tile, int kt) { tile_gload(qh, ql, bh, bl, qimg, bimg, Q, q0, N, dp, rec, tid, tile, kt); };
  auto sstore = [&]() { tile_sstore(smem, qh, ql, bh, bl, tid); };

  if (sr.t_begin < sr.t_end) gload(sr.t_begin, 0);
  __syncthreads();   // the lists
  for (int tile = sr.t_begin; tile < sr.t_end; ++tile) {
    const int b0 = tile * TB;
    long long gt = 0;   // GM != 0: bank row b0 + tid's group, in flight under the products
    if constexpr (GM != 0) gt = load_tile_group(bgrp, b0, N);
    f32x4 acc[NI][MI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kt = 0; kt < nk; ++kt) {
      sstore();
      __syncthreads();
      if (kt + 1 < nk) gload(tile, kt + 1);
      else if (tile + 1 < sr.t_end) gload(tile + 1, 0);
#pragma unroll 1   // (unrolled, the fragments of both halves are loaded up front: 56 registers to scratch)
      for (int ks = 0; ks < BK / 32; ++ks) {
        if (kt * BK + ks * 32 < dp) {
          h2x8 bfr[MI];
#pragma unroll
          for (int mi = 0; mi < MI; ++mi) {
            const int o = swz(p.qrow(mi), ks * 4 + p.lq);
            bfr[mi].hi = *reinterpret_cast<const f16x8*>(Qh + o);
            bfr[mi].lo = *reinterpret_cast<const f16x8*>(Ql + o);
          }
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            const int o = swz(p.wn * 64 + ni * 16 + p.lrow, ks * 4 + p.lq);
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
    // scores, and which of them can enter a list (<=: a tie may still win on the index); the fragment's bank biases
    // and scales
    float t[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) t[mi] = thr[p.qrow(mi)];
    unsigned long long mask = 0;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float nb[4], sb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = p.gb(b0, ni, i);
        const float2 h = b < N ? *reinterpret_cast<const float2*>(bimg + (size_t)b * rec)
                               : make_float2(__builtin_inff(), 0.f);
        nb[i] = h.x;
        sb[i] = h.y;
      }
      long long bg[4];   // GM & GM_EXCLUDE: the fragment's bank groups
      if constexpr ((GM & GM_EXCLUDE) != 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bg[i] = tg[p.wn * 64 + ni * 16 + p.lq * 4 + i];   // (p.brow(ni, i), spelt out)
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gb = p.gb(b0, ni, i);
          const float s = tile_score(acc[ni][mi][i], sq[mi], sb[i], nb[i]);
          acc[ni][mi][i] = s;
          bool in = s <= t[mi] && s < __builtin_inff() && gb < sr.b_end && gb != selfb[mi];
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
          for (int mi = 0; mi < MI; ++mi) t[mi] = thr[p.qrow(mi)];
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const unsigned long long bit = 1ull << ((ni * MI + mi) * 4 + i);
              if ((mask & bit) != 0) {
                const int row = p.qrow(mi);
                if (!(acc[ni][mi][i] <= t[mi])) {
                  mask &= ~bit;
                } else {
                  const int slot = atomicAdd(&bcnt[row], 1);
                  if (slot < BCAP) {
                    bucket[row * BCAP + slot] = Cand{acc[ni][mi][i], p.brow(ni, i)};
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
          if constexpr ((GM & GM_ONE) != 0) offer_one(L + tid * k, LG, TQ, k, c.s, b0 + c.i, tg[c.i], ts, ti, tp);
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
    Cand* o = cand + ((q0 + tid) * splits + sr.split) * k;
    for (int j = 0; j < k; ++j) o[j] = L[tid * k + j];
  }
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
    keep_group_bests(pool, pgrp, P, lane);
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

int auto_splits(int64_t n_query, int64_t n_bank) {
  // (no sum that could overflow: the callers' shape checks may still be ahead)
  const int64_t qt = n_query / TQ + (n_query % TQ != 0), bt = n_bank / TB + (n_bank % TB != 0);
  if (qt < 1 || bt < 1) return 1;
  // two workgroups per CU (256 CUs) where the bank has the tiles for it
  int64_t s = (512 + qt - 1) / qt;
  s = s > bt ? bt : s;
  s = s > MAX_SPLITS ? MAX_SPLITS : s;
  return (int)(s < 1 ? 1 : s);
}

// what the query keeps behind the packed query rows: k candidates per (query, split) and, with one entry per group, the
// groups of the list entries, [query tiles][splits][k][TQ] int64
size_t query_extra_bytes(int64_t n_query, int k, int splits, int flags) {
  const size_t cands = (size_t)n_query * splits * k * sizeof(Cand);
  if ((flags & GM_ONE) == 0) return cands;
  return cands + ((size_t)n_query + TQ - 1) / TQ * TQ * splits * k * sizeof(long long);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// the host helpers every search kind shares (knn_tile.h)
namespace knn {

int check_shape(const char* who, int64_t n_query, int64_t n_bank, int dim, int k) {
  if (dim < 1 || dim > MAX_DIM || k < 1 || k > MAX_K || n_query < 0 || n_bank < 0 || n_bank > 0x7fffffffLL ||
      n_query > 0x7fffffffLL) {
    btsbot_set_error("%s: need 1 <= dim <= %d, 1 <= k <= %d, 0 <= n_bank, n_query < 2^31 (dim=%d k=%d n_bank=%lld "
                     "n_query=%lld)", who, MAX_DIM, MAX_K, dim, k, (long long)n_bank, (long long)n_query);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

size_t image_bytes(int64_t rows, int dim) { return ((size_t)rows * record_bytes(dim) + 255) & ~(size_t)255; }

int check_search(const char* who, const SearchArgs& a) {
  TRY(check_shape(who, a.n_query, a.n_bank, a.dim, a.k));
  if (a.metric != BTSBOT_KNN_EUCLIDEAN && a.metric != BTSBOT_KNN_COSINE) {
    btsbot_set_error("%s: metric %d", who, a.metric);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (a.splits < a.min_splits || a.splits > MAX_SPLITS) {
    if (a.min_splits == 0) btsbot_set_error("%s: splits=%d must be 0 (the library's choice) .. %d", who, a.splits, MAX_SPLITS);
    else btsbot_set_error("%s: splits=%d must be 1 .. %d", who, a.splits, MAX_SPLITS);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((a.flags & ~a.flag_mask) != 0) {
    if (a.mode_word == nullptr)
      btsbot_set_error("%s: flags=%d holds bits other than BTSBOT_KNN_EXCLUDE_SAME | BTSBOT_KNN_ONE_PER_GROUP", who, a.flags);
    else
      btsbot_set_error("%s: flags=%d, only 0 and BTSBOT_KNN_EXCLUDE_SAME are %s modes", who, a.flags, a.mode_word);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((a.flags & GM_ONE) != 0 && a.k > MAX_K_ONE) {
    btsbot_set_error("%s: k=%d, but BTSBOT_KNN_ONE_PER_GROUP holds k <= %d (the merge keeps its pool's groups on chip)", who,
                     a.k, MAX_K_ONE);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (a.n_query == 0) return BTSBOT_OK;
  if (a.null_arg) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (((a.flags & GM_EXCLUDE) != 0 && a.query_group == nullptr) ||
      (a.flags != 0 && a.n_bank > 0 && a.bank_group == nullptr)) {
    if (a.mode_word == nullptr)
      btsbot_set_error("%s: flags=%d need bank_group (and BTSBOT_KNN_EXCLUDE_SAME query_group), got NULL", who, a.flags);
    else
      btsbot_set_error("%s: BTSBOT_KNN_EXCLUDE_SAME needs query_group and bank_group, got NULL", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int64_t need = (int64_t)(image_bytes(a.n_query, a.dim) + a.extra_bytes);
  if (a.workspace_bytes < need || ((uintptr_t)a.workspace & 15) != 0 || ((uintptr_t)a.packed & 15) != 0) {
    btsbot_set_error("%s: workspace of %lld bytes (need %lld), or workspace / packed not 16-byte aligned", who,
                     (long long)a.workspace_bytes, (long long)need);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

Margin margin(int dim, int metric) {
  const float u = 5.9604644775390625e-8f;
  return Margin{1.f + 4.f * (float)(dim + 4) * u, 1.f - 4.f * (float)(dim + 4) * u,
                (metric == BTSBOT_KNN_COSINE ? 16.f : 8.f) * (float)(dim + 8) * u};
}

TileGrid tile_grid(int64_t n_query, int64_t n_bank, int splits) {
  const int total_tiles = (int)((n_bank + TB - 1) / TB);
  return TileGrid{(total_tiles + splits - 1) / splits, dim3((unsigned)((n_query + TQ - 1) / TQ), (unsigned)splits)};
}

unsigned verify_waves(int64_t n, int64_t n_query) {
  const int64_t per = (n + n_query - 1) / n_query;
  return (unsigned)(per <= 32 ? 1 : per >= 32 * 64 ? 64 : (per + 31) / 32);
}

int pack_queries(const float* queries, int64_t n_query, int dim, unsigned char* qimg, hipStream_t st) {
  hipLaunchKernelGGL(knn_pack_kernel, dim3((unsigned)((n_query + 3) / 4)), dim3(256), 0, st, queries, (long)n_query, dim,
                     (int)MODE_QUERY, qimg);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

}  // namespace knn

extern "C" int64_t btsbot_knn_bank_bytes(int64_t n_bank, int dim) {
  if (knn::check_shape("btsbot_knn_bank_bytes", 0, n_bank, dim, 1) != BTSBOT_OK) return BTSBOT_ERR_INVALID_ARG;
  return (int64_t)((size_t)n_bank * record_bytes(dim));
}

extern "C" int btsbot_knn_pack_bank(const float* rows, int64_t first_row, int64_t n_rows, int dim, int metric,
                                    void* packed, int64_t n_bank_capacity, void* stream) {
  const int s = knn::check_shape("btsbot_knn_pack_bank", 0, n_bank_capacity, dim, 1);
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
  const int s = knn::check_shape("btsbot_knn_splits", n_query, n_bank, dim, k);
  if (s != BTSBOT_OK) return s;
  return auto_splits(n_query, n_bank);
}

extern "C" int64_t btsbot_knn_workspace_grouped(int64_t n_query, int64_t n_bank, int dim, int k, int splits, int flags) {
  if (knn::check_shape("btsbot_knn_workspace", n_query, n_bank, dim, k) != BTSBOT_OK) return BTSBOT_ERR_INVALID_ARG;
  if (splits < 0 || splits > MAX_SPLITS) {
    btsbot_set_error("btsbot_knn_workspace: splits=%d must be 0 (the library's choice) .. %d", splits, MAX_SPLITS);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (splits == 0) splits = auto_splits(n_query, n_bank);
  return (int64_t)(knn::image_bytes(n_query, dim) + query_extra_bytes(n_query, k, splits, flags));
}

extern "C" int64_t btsbot_knn_workspace(int64_t n_query, int64_t n_bank, int dim, int k, int splits) {
  return btsbot_knn_workspace_grouped(n_query, n_bank, dim, k, splits, 0);
}

namespace {

// The launches of btsbot_knn_query (GM = 0) and btsbot_knn_query_grouped, one instantiation per group mode
template <int GM>
int launch_query(const float* queries, int64_t n_query, const float* bank, const unsigned char* packed, int64_t n_bank,
                 int dim, int k, int metric, int64_t self_offset, int splits, int64_t* idx, float* dist,
                 unsigned char* qimg, Cand* cand, const long long* qgrp, const long long* bgrp, hipStream_t st) {
  // (the candidates end on a multiple of 8 bytes behind the 256-byte aligned query image)
  long long* lgrp = reinterpret_cast<long long*>(cand + (size_t)n_query * splits * k);
  TRY(knn::pack_queries(queries, n_query, dim, qimg, st));
  const knn::TileGrid tg = knn::tile_grid(n_query, n_bank, splits);
  // 64 KB of operands + 1 KB of lists per k: two workgroups per CU up to k = 16, in every group mode
  static DevOnce attr;
  if (attr.need()) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_select_kernel<GM>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS + TQ * MAX_K * (int)sizeof(Cand)));
    attr.done();
  }
  hipLaunchKernelGGL(knn_select_kernel<GM>, tg.grid, dim3(256), GEMM_LDS + TQ * k * (int)sizeof(Cand), st, qimg, packed,
                     (long)n_query, (int)n_bank, dim, k, (long)self_offset, tg.tiles_per_split, splits, cand, qgrp, bgrp,
                     lgrp);
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
  const bool null_arg = queries == nullptr || idx == nullptr || dist == nullptr || workspace == nullptr ||
                        (n_bank > 0 && (bank == nullptr || packed == nullptr));
  const int sp = splits == 0 ? auto_splits(n_query, n_bank) : splits;
  TRY(knn::check_search(who, knn::SearchArgs{n_query, n_bank, dim, k, metric, splits, 0, flags, GM_EXCLUDE | GM_ONE,
                                             nullptr, null_arg, query_group, bank_group, packed, workspace,
                                             workspace_bytes, query_extra_bytes(n_query, k, sp, flags)}));
  if (n_query == 0) return BTSBOT_OK;
  splits = sp;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* qimg = reinterpret_cast<unsigned char*>(workspace);
  Cand* cand = reinterpret_cast<Cand*>(qimg + knn::image_bytes(n_query, dim));
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
