// btsbot_knn_rank_*: where a given bank row stands in a query row's neighbour ordering (gfx950), DESIGN.md section 4r.
//
// rank[q][c] = the number of eligible bank rows b with (direct_distance(q, b), b) before (dist[q][c], targets[q][c]).
// The tile walk of knn_tile.h with a third epilogue, "count if surely before the target, hand to the direct form if
// within the margin": the margin of 4p read from both sides.  With r = dist[q][c] a pair's GEMM-form value g decides
//   g <  lo_c = r^2 * relm - ctau * (|q|^2 + |b|^2)   (cosine: r - ctau)    surely before: the direct form is < r, strictly
//   g <= hi_c = r^2 * rel  + ctau * (|q|^2 + |b|^2)   (cosine: r + ctau)    the band: the direct form decides
// and nothing otherwise (relm = 1 - 4 (D + 4) u; rel and ctau are the radius search's).  The thresholds kernel leaves
// thr[q][c] = (r^2 * relm, r^2 * rel) (cosine: (r - ctau, r + ctau)) and rowlim[q] = the largest second component.
#include "knn_tile.h"

namespace {

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
  int* qn = reinterpret_cast<int*>(smem + GEMM_LDS + RowRegions::BYTES);   // the queue's fill count (16 bytes kept for it)
  int* sure = qn + 4;                                             // [TQ][t] count pass: the surely-before pairs
  long long* tg = reinterpret_cast<long long*>(smem);             // EXCL: [TB] the tile's bank groups (idle operand LDS)
  RankEnt* ent = reinterpret_cast<RankEnt*>(smem + RANK_QOFF);    // [RANK_QCAP] the tile's queue (idle operand LDS)

  const int tid = threadIdx.x;
  const LanePos p;
  const size_t rec = record_bytes(dim);
  const long q0 = (long)blockIdx.x * TQ;
  const SplitRange sr(N, tiles_per_split);
  RowRegions rows;   // a row's band pairs so far; FILL: where they go in cand / cmask
  rows.init<FILL>(smem + GEMM_LDS, Q, q0, splits, sr.split, counts, offsets);
  if (tid == 0) *qn = 0;
  if constexpr (!FILL)
    for (int i = tid; i < TQ * t; i += 256) sure[i] = 0;

  QueryRows<EXCL> qr;
  qr.load(qimg, rec, Q, q0, N, self_offset, qgrp, p);
  float lim[MI];   // the row's widest limit
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const long gq = p.gq(q0, mi);
    // a row past Q, a non-finite query row and a row without a valid target pass nothing
    lim[mi] = gq < Q && qr.sq[mi] != 0.f ? rowlim[gq] : -__builtin_inff();
  }

  // one (score, column) compare, by the same expressions wherever it is made: -1 surely before, 1 in the band, 0 neither
  auto side = [&](float g, float x, float2 lh) {
    return g < fmaf(-ctau, x, lh.x) ? -1 : g <= fmaf(ctau, x, lh.y) ? 1 : 0;
  };
  bool past = false;
  // FILL: band pair (bank row gb, columns band) of query row `row` into the row's region
  auto write_band = [&](int row, int gb, unsigned long long band) {
    const long long at = rows.slot(row, n_band);
    if (at >= 0) {
      cand[at] = gb;
      cmask[at] = band;
    } else {
      past = true;
    }
  };

  int n[MI] = {0, 0, 0, 0};
  TileWalk w;
  w.init(qimg, bimg, smem, Q, q0, N, dim);
  if (sr.t_begin < sr.t_end) w.gload(sr.t_begin, 0);
  __syncthreads();   // the rows' counters and regions
  for (int tile = sr.t_begin; tile < sr.t_end; ++tile) {
    const int b0 = tile * TB;
    long long gt = 0;   // EXCL: bank row b0 + tid's group, in flight under the products
    if constexpr (EXCL) gt = load_tile_group(bgrp, b0, N);
    f32x4 acc[NI][MI];
    w.products(acc, tile, sr.t_end);
    if constexpr (EXCL) {
      if (tid < TB) tg[tid] = gt;
      lds_barrier();
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float nb[4], sb[4];
      frag_bias_scale(bimg, rec, N, p, b0, ni, nb, sb);
      long long bg[4];
      if constexpr (EXCL) frag_groups(tg, p, ni, bg);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gb = p.gb(b0, ni, i);
          const float s = tile_score(acc[ni][mi][i], qr.sq[mi], sb[i], nb[i]);
          float g, x;   // x: what the margin's tau part scales with (cosine: its tau is in the thresholds)
          if (metric == 0) {
            g = s + qr.qq[mi];
            x = qr.qq[mi] + nb[i];
          } else {
            g = fmaf(s, qr.qinv[mi], 1.f);
            x = 0.f;
          }
          const float l = fmaf(ctau, x, lim[mi]);
          if (eligible<EXCL>(g <= l, s, gb, sr.b_end, qr.selfb[mi], bg[i], qr.qg[mi])) {
            const int row = p.qrow(mi);
            const int slot = atomicAdd(qn, 1);
            if (slot < RANK_QCAP) {
              ent[slot] = RankEnt{row * TB + (gb - b0), g, x, 0u, 0u};
              continue;
            }
            const float2* th = thr + (q0 + row) * t;
            unsigned long long band = 0;
#pragma unroll 1
            for (int c = 0; c < t; ++c) {
              const int sd = side(g, x, th[c]);
              if (sd < 0) {
                if constexpr (!FILL) atomicAdd(&sure[row * t + c], 1);
              } else if (sd > 0) {
                band |= 1ull << c;
              }
            }
            if (band != 0) {
              if constexpr (FILL) write_band(row, gb, band);
              else ++n[mi];
            }
          }
        }
    }
    lds_barrier();   // the queue is complete (and the groups are read)
    const int nq = min(*qn, RANK_QCAP);
    for (int w = tid; w < nq * t; w += 256) {   // one (score, column) compare per thread and step
      const int e = w / t, c = w - e * t;
      const int row = ent[e].rowgb / TB;
      const int sd = side(ent[e].g, ent[e].x, thr[(q0 + row) * t + c]);
      if (sd < 0) {
        if constexpr (!FILL) atomicAdd(&sure[row * t + c], 1);
      } else if (sd > 0) {
        atomicOr(c < 32 ? &ent[e].mlo : &ent[e].mhi, 1u << (c & 31));
      }
    }
    lds_barrier();   // the masks are complete
    for (int e = tid; e < nq; e += 256) {
      const unsigned long long band = (unsigned long long)ent[e].mhi << 32 | ent[e].mlo;
      if (band == 0) continue;
      const int row = ent[e].rowgb / TB;
      if constexpr (FILL) write_band(row, b0 + ent[e].rowgb % TB, band);
      else atomicAdd(&rows.cnt[row], 1);
    }
    lds_barrier();   // the queue is read: the next tile's operands may land there
    if (tid == 0) *qn = 0;   // (the next tile's first push is behind the barriers of its products)
  }

  if constexpr (FILL) {
    if (past) *err = 1;
  } else {
    rows.store_counts(n, p, Q, q0, splits, sr.split, counts);
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

// the workspace behind the packed query rows: thr float2 [n_query][n_targets], rowlim float [n_query]
size_t rank_thr_bytes(int64_t n_query, int n_targets) {
  return ((size_t)n_query * n_targets * sizeof(float2) + 255) & ~(size_t)255;
}
float2* rank_thr(const RankArgs& a) {
  return reinterpret_cast<float2*>(reinterpret_cast<unsigned char*>(a.workspace) + knn::image_bytes(a.n_query, a.dim));
}
float* rank_rowlim(const RankArgs& a) {
  return reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(rank_thr(a)) + rank_thr_bytes(a.n_query, a.n_targets));
}

int rank_checked(const char* who, const RankArgs& a) {
  const bool null_arg = a.queries == nullptr || a.targets == nullptr || a.workspace == nullptr ||
                        (a.n_bank > 0 && (a.bank == nullptr || a.packed == nullptr));
  // (1 <= n_targets <= 64 is k's range)
  return knn::check_search(who, knn::SearchArgs{a.n_query, a.n_bank, a.dim, a.n_targets, a.metric, a.splits, 1, a.flags,
                                                GM_EXCLUDE, "rank", null_arg, a.query_group, a.bank_group, a.packed,
                                                a.workspace, a.workspace_bytes,
                                                rank_thr_bytes(a.n_query, a.n_targets) + (size_t)a.n_query * sizeof(float)});
}

template <bool FILL, bool EXCL>
int launch_rank(const RankArgs& a, int* rank, int* counts, const int64_t* offsets, int* cand, uint64_t* cmask,
                int64_t n_band, int* err, hipStream_t st) {
  // operands + the rows' counters and regions; the queue's count; the count pass: + its n_targets sure counts per row
  const int lds = GEMM_LDS + RowRegions::BYTES + 16 + (FILL ? 0 : TQ * a.n_targets * (int)sizeof(int));
  static DevOnce attr;
  if (attr.need()) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_rank_kernel<FILL, EXCL>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                GEMM_LDS + RowRegions::BYTES + 16 + (FILL ? 0 : TQ * MAX_K * (int)sizeof(int))));
    attr.done();
  }
  const knn::Margin m = knn::margin(a.dim, a.metric);
  const knn::TileGrid tg = knn::tile_grid(a.n_query, a.n_bank, a.splits);
  hipLaunchKernelGGL((knn_rank_kernel<FILL, EXCL>), tg.grid, dim3(256), lds, st,
                     reinterpret_cast<const unsigned char*>(a.workspace), reinterpret_cast<const unsigned char*>(a.packed),
                     (long)a.n_query, (int)a.n_bank, a.dim, a.metric, a.n_targets, (const float2*)rank_thr(a),
                     (const float*)rank_rowlim(a), m.ctau, (long)a.self_offset, tg.tiles_per_split, a.splits,
                     reinterpret_cast<const long long*>(a.query_group),
                     reinterpret_cast<const long long*>(a.bank_group), rank, counts,
                     reinterpret_cast<const long long*>(offsets), cand, reinterpret_cast<unsigned long long*>(cmask),
                     (long long)n_band, err);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

}  // namespace

extern "C" int64_t btsbot_knn_rank_workspace(int64_t n_query, int dim, int n_targets) {
  if (knn::check_shape("btsbot_knn_rank_workspace", n_query, 0, dim, n_targets) != BTSBOT_OK) return BTSBOT_ERR_INVALID_ARG;
  return (int64_t)(knn::image_bytes(n_query, dim) + rank_thr_bytes(n_query, n_targets) + (size_t)n_query * sizeof(float));
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
  TRY(knn::pack_queries(queries, n_query, dim, reinterpret_cast<unsigned char*>(workspace), st));
  const knn::Margin m = knn::margin(dim, metric);
  hipLaunchKernelGGL(knn_rank_thresh_kernel, dim3((unsigned)n_query), dim3(64), 0, st, queries, bank,
                     reinterpret_cast<const unsigned char*>(packed), (long)n_bank, dim, metric,
                     reinterpret_cast<const long long*>(targets), n_targets, (long)self_offset,
                     flags != 0 ? reinterpret_cast<const long long*>(query_group) : nullptr,
                     reinterpret_cast<const long long*>(bank_group), m.rel, m.relm, m.ctau, dist, rank, rank_thr(a),
                     rank_rowlim(a));
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
  hipLaunchKernelGGL(knn_rank_verify_kernel, dim3((unsigned)n_query, knn::verify_waves(n_band, n_query)), dim3(64), 0, st,
                     queries, bank, reinterpret_cast<const long long*>(targets), n_targets, dist,
                     reinterpret_cast<const long long*>(offsets), splits, (const int*)cand,
                     reinterpret_cast<const unsigned long long*>(cand_mask), (int)n_bank, dim, metric, rank);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
