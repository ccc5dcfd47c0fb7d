// btsbot_knn_radius_*: every bank row within r of a query row (gfx950), DESIGN.md section 4p.
//
// The selection's grid and tile walk (knn_tile.h) with a second epilogue, "admit if within r" in place of "keep the
// best k".  A pair is a CANDIDATE when its GEMM-form value
//   Euclidean  g = score + |q|^2            <= lim = r^2 * rel + ctau * (|q|^2 + |b|^2)
//   cosine     g = 1 + score / (2 |q|)      <= lim = r + ctau
// (rel = 1 + 4 (D + 4) u, ctau = 8 (D + 8) u; cosine ctau = 16 (D + 8) u: the margin of 4p, which covers the error
// bounds of this form and of the direct form) -- a superset of the members, decided by the same expression in both
// instantiations.  FILL = false counts a (query, split)'s candidates; FILL = true writes their bank rows into the region
// the scan of the counts gave it, slots handed out by an LDS cursor per query row (the order inside a region is no
// one's business: the lists are sorted afterwards), each slot checked against the region's size.  No list of fixed
// size, nothing of size Q x N.  knn_radius_verify_kernel then applies direct_distance(), the one function that computes
// a returned distance, to every candidate.
#include "knn_tile.h"

namespace {

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
  long long* tg = reinterpret_cast<long long*>(smem);   // EXCL: [TB] the tile's bank groups (idle operand LDS)

  const int tid = threadIdx.x;
  const LanePos p;
  const size_t rec = record_bytes(dim);
  const long q0 = (long)blockIdx.x * TQ;
  const SplitRange sr(N, tiles_per_split);
  // (RowRegions::init and ::store_counts in this kernel's own text, here and at the end: called, the count pass is
  //  18 instructions longer and 1 % slower)
  RowRegions rows;
  rows.cnt = reinterpret_cast<int*>(smem + GEMM_LDS);
  rows.cap = rows.cnt + TQ;
  rows.base = reinterpret_cast<long long*>(rows.cap + TQ);
  if (tid < TQ) {
    rows.cnt[tid] = 0;
    if constexpr (FILL) {
      const bool in = q0 + tid < Q;
      rows.cap[tid] = in ? counts[(q0 + tid) * splits + sr.split] : 0;
      rows.base[tid] = in ? offsets[(q0 + tid) * splits + sr.split] : 0;
    }
  }

  QueryRows<EXCL> qr;
  qr.load(qimg, rec, Q, q0, N, self_offset, qgrp, p);
  float lim[MI];   // r^2 * rel (cosine: r + ctau)
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const long gq = p.gq(q0, mi);
    const float r = gq < Q ? radius[gq] : -1.f;
    // a row past Q, a non-finite query row (scale 0) and a negative or NaN radius admit nothing
    lim[mi] = qr.sq[mi] != 0.f && r >= 0.f ? (metric == 0 ? (r * r) * rel : r + ctau) : -__builtin_inff();
  }

  int n[MI] = {0, 0, 0, 0};
  bool past = false;
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
          float g, l;
          if (metric == 0) {
            g = s + qr.qq[mi];
            l = fmaf(ctau, qr.qq[mi] + nb[i], lim[mi]);
          } else {
            g = fmaf(s, qr.qinv[mi], 1.f);
            l = lim[mi];
          }
          if (eligible<EXCL>(g <= l, s, gb, sr.b_end, qr.selfb[mi], bg[i], qr.qg[mi])) {
            if constexpr (FILL) {
              const long long at = rows.slot(p.qrow(mi), n_cand);
              if (at >= 0) cand[at] = gb;
              else past = true;
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
      if (n[mi] != 0) atomicAdd(&rows.cnt[p.qrow(mi)], n[mi]);
    __syncthreads();
    if (tid < TQ && q0 + tid < Q) counts[(q0 + tid) * splits + sr.split] = rows.cnt[tid];
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
  const bool null_arg = a.queries == nullptr || a.radius == nullptr || a.workspace == nullptr ||
                        (a.n_bank > 0 && a.packed == nullptr);
  return knn::check_search(who, knn::SearchArgs{a.n_query, a.n_bank, a.dim, 1, a.metric, a.splits, 1, a.flags,
                                                GM_EXCLUDE, "radius", null_arg, a.query_group, a.bank_group, a.packed,
                                                a.workspace, a.workspace_bytes, 0});
}

// query pack + one tile pass (FILL = false: counts are written; true: counts and offsets are read, cand is written)
template <bool FILL, bool EXCL>
int launch_radius(const RadiusArgs& a, int* counts, const int64_t* offsets, int* cand, int64_t n_cand, int* err,
                  hipStream_t st) {
  unsigned char* qimg = reinterpret_cast<unsigned char*>(a.workspace);
  TRY(knn::pack_queries(a.queries, a.n_query, a.dim, qimg, st));
  constexpr int LDS = GEMM_LDS + RowRegions::BYTES;
  static DevOnce attr;
  if (attr.need()) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(knn_radius_kernel<FILL, EXCL>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    attr.done();
  }
  const knn::Margin m = knn::margin(a.dim, a.metric);
  const knn::TileGrid tg = knn::tile_grid(a.n_query, a.n_bank, a.splits);
  hipLaunchKernelGGL((knn_radius_kernel<FILL, EXCL>), tg.grid, dim3(256), LDS, st, (const unsigned char*)qimg,
                     reinterpret_cast<const unsigned char*>(a.packed), (long)a.n_query, (int)a.n_bank, a.dim, a.metric,
                     a.radius, m.rel, m.ctau, (long)a.self_offset, tg.tiles_per_split, a.splits,
                     reinterpret_cast<const long long*>(a.query_group),
                     reinterpret_cast<const long long*>(a.bank_group), counts,
                     reinterpret_cast<const long long*>(offsets), cand, (long long)n_cand, err);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

}  // namespace

extern "C" int64_t btsbot_knn_radius_workspace(int64_t n_query, int dim) {
  if (knn::check_shape("btsbot_knn_radius_workspace", n_query, 0, dim, 1) != BTSBOT_OK) return BTSBOT_ERR_INVALID_ARG;
  return (int64_t)knn::image_bytes(n_query, dim);
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
  hipLaunchKernelGGL(knn_radius_verify_kernel, dim3((unsigned)n_query, knn::verify_waves(n_cand, n_query)), dim3(64), 0,
                     st, queries, bank, radius, reinterpret_cast<const long long*>(offsets), splits, (const int*)cand,
                     (int)n_bank, dim, metric, dist, keep);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
