// btsbot_grid_*: exact radius and k-nearest search over 2-D fp32 points on a uniform grid (gfx950), DESIGN.md section 4q.
//
// The grid only prunes, it never decides.  Every kernel here computes a pair's distance with grid_distance() -- the value
// direct_distance() of knn_tile.h gives at D = 2: sqrtf(fl(fl(t0 t0) + fl(t1 t1))), t = q - b, nothing contracted -- and
// decides membership and rank by it alone; the cells say which pairs are looked at.  That no member is missed rests on
// three facts (4q holds the proof):
//   * cell_of() is a monotone function of the coordinate: fl(x - x0), fl(. * inv_h) with inv_h >= 0, floor and clamp are
//     each monotone under round-to-nearest (a NaN product, inf * 0, lands in cell 0 like every other product by 0);
//   * a pair whose fp32 distance is <= r has |q_x - b_x| <= R = inflate(r) in the reals, on either axis;
//   * safe_cells() walks c(lo) .. c(hi) with lo <= q_x - R and q_x + R <= hi as fp32 numbers, each stepped outward once
//     after its rounding.
// Hence c(lo) <= c(b_x) <= c(hi) for every member, whatever the cell size: the resolution governs the cost only.
//
// Layout (btsbot_grid_cells + torch's stable sort): cell = cy * G + cx, the non-finite rows in a trailing bucket G * G
// that no walk visits; cell_start int32 [G * G + 1]; the points as float2, their original rows and their groups in cell
// order.  The cells c(lo_x) .. c(hi_x) of one grid row are one contiguous span of the sorted points.
//
// Radius: a group of W lanes per query row (W = 16 unless the caller says otherwise; 4q has the measurements) strides
// over each span.  The count pass adds per lane and reduces within the group; the fill pass numbers the members of a
// step with a ballot, so the slots inside a row's region are a function of the walk alone -- no atomics.  k-nearest: one
// wave per query row, lane j holding the j-th best (distance, row) seen; squares of cells grow around the query's cell
// until k eligible rows were seen, then the safe range of their k-th distance is walked without the square.
#include <float.h>

#include "list_row.h"

namespace {

constexpr int GRID_MAX_CELLS = 4096;   // per axis: cell_start is 64 MiB there
constexpr int GRID_MAX_K = 64;
constexpr int EMPTY = 0x7fffffff;

struct GridView {
  const float* geom;         // {x0, y0, inv_hx, inv_hy}, written by grid_geometry_kernel
  const int* cell_start;     // [G * G + 1]
  const float2* pts;         // [n] in cell order
  const int* row;            // [n] the points' original rows
  const long long* grp;      // [n] their groups, or nullptr
  int G, n;
};

// ---------------------------------------------------------------------------------------------------------------------
// the three rules every kernel of this file shares
__device__ __forceinline__ float grid_distance(float qx, float qy, float bx, float by) {
#pragma clang fp contract(off)
  const float t0 = qx - bx, t1 = qy - by;
  const float s0 = t0 * t0, s1 = t1 * t1;
  const float ss = s0 + s1;
  return sqrtf(ss);
}

// a finite row: both coordinates finite and fl(fl(x x) + fl(y y)) <= FLT_MAX (load_query_row and the packed bank at D = 2)
__device__ __forceinline__ bool grid_finite(float x, float y) {
#pragma clang fp contract(off)
  const float sx = x * x, sy = y * y;
  const float ss = sx + sy;
  return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && ss <= FLT_MAX;
}

__device__ __forceinline__ int cell_of(float x, float x0, float inv_h, int G) {
#pragma clang fp contract(off)
  const float t = x - x0;
  const float v = floorf(t * inv_h);
  return (int)fminf(fmaxf(v, 0.f), (float)(G - 1));   // fmaxf(NaN, 0) = 0
}

// R >= |q_x - b_x| for every pair whose grid_distance is <= r (r >= 0, +inf allowed): max(r, 2^-60) (1 + 16 u), up
__device__ __forceinline__ float inflate(float r) {
#pragma clang fp contract(off)
  const float R = fmaxf(r, 0x1p-60f) * 1.00000095367431640625f;
  return nextafterf(R, __builtin_inff());
}

__device__ __forceinline__ void safe_cells(float x, float R, float x0, float inv_h, int G, int& c0, int& c1) {
#pragma clang fp contract(off)
  const float lo = nextafterf(x - R, -__builtin_inff());
  const float hi = nextafterf(x + R, __builtin_inff());
  c0 = cell_of(lo, x0, inv_h, G);
  c1 = cell_of(hi, x0, inv_h, G);
}

// a span of the sorted points, kept inside [0, n] whatever cell_start holds
__device__ __forceinline__ void span_of(const GridView& g, int row_cell, int cx0, int cx1, int& s0, int& s1) {
  s0 = g.cell_start[row_cell + cx0];
  s1 = g.cell_start[row_cell + cx1 + 1];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > g.n ? g.n : s1;
}

// ---------------------------------------------------------------------------------------------------------------------
// build
__global__ __launch_bounds__(256) void grid_finite_kernel(const float2* __restrict__ pts, long n,
                                                          unsigned char* __restrict__ finite) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float2 p = pts[i];
  finite[i] = grid_finite(p.x, p.y) ? 1 : 0;
}

// bbox = {min x, min y, max x, max y} of the finite rows (+inf / -inf without one).  A zero, negative or NaN extent, or
// one so small that G / extent overflows, gives inv_h = 0: everything lands in cell 0.
__global__ void grid_geometry_kernel(const float* __restrict__ bbox, int G, float* __restrict__ geom) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int a = 0; a < 2; ++a) {
    const float lo = bbox[a], hi = bbox[2 + a];
    const float ext = hi - lo;
    float inv = (float)G / ext;
    if (!(ext > 0.f) || !(inv <= FLT_MAX) || !(fabsf(lo) <= FLT_MAX)) inv = 0.f;
    geom[a] = fabsf(lo) <= FLT_MAX ? lo : 0.f;
    geom[2 + a] = inv;
  }
}

__global__ __launch_bounds__(256) void grid_cell_kernel(const float2* __restrict__ pts, long n,
                                                        const float* __restrict__ geom, int G,
                                                        int* __restrict__ cell) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float2 p = pts[i];
  cell[i] = grid_finite(p.x, p.y) ? cell_of(p.y, geom[1], geom[3], G) * G + cell_of(p.x, geom[0], geom[2], G) : G * G;
}

// ---------------------------------------------------------------------------------------------------------------------
// radius: W lanes per query row.  FILL = false: counts[q] = the members, visited[q] = the pairs looked at.  FILL = true:
// the members' rows and distances at indptr[q] .., in the order of the walk; a slot past indptr[q + 1] is not written
// and raises *err.
template <int W, bool FILL, bool EXCL>
__global__ __launch_bounds__(256) void grid_radius_kernel(const GridView g, const float2* __restrict__ queries, long Q,
                                                          const float* __restrict__ radius, long self_offset,
                                                          const long long* __restrict__ qgrp,
                                                          long long* __restrict__ counts,
                                                          long long* __restrict__ visited,
                                                          const long long* __restrict__ indptr, int* __restrict__ cand,
                                                          float* __restrict__ dist, int* __restrict__ err) {
  const int lane = threadIdx.x & 63, l = lane & (W - 1), sub = lane / W;
  const long q = ((long)blockIdx.x * 256 + threadIdx.x) / W;
  bool live = q < Q;
  float qx = 0.f, qy = 0.f, r = 0.f;
  if (live) {
    const float2 p = queries[q];
    qx = p.x;
    qy = p.y;
    r = radius[q];
    live = grid_finite(qx, qy) && r >= 0.f;   // (a negative or NaN radius admits nothing)
  }
  int cnt = 0;
  long long vis = 0;
  if (live) {
    const float R = inflate(r);
    int cx0, cx1, cy0, cy1;
    safe_cells(qx, R, g.geom[0], g.geom[2], g.G, cx0, cx1);
    safe_cells(qy, R, g.geom[1], g.geom[3], g.G, cy0, cy1);
    const long self = self_offset >= 0 ? q + self_offset : -1;
    const long long qg = EXCL ? qgrp[q] : 0;
    const long long base = FILL ? indptr[q] : 0, end = FILL ? indptr[q + 1] : 0;
    for (int cy = cy0; cy <= cy1; ++cy) {
      int s0, s1;
      span_of(g, cy * g.G, cx0, cx1, s0, s1);
      vis += s1 > s0 ? s1 - s0 : 0;
      for (int b = s0; b < s1; b += W) {   // (the same trips in every lane of the group)
        const int s = b + l;
        bool member = false;
        float d = 0.f;
        int bi = 0;
        if (s < s1) {
          const float2 p = g.pts[s];
          bi = g.row[s];
          d = grid_distance(qx, qy, p.x, p.y);
          member = d <= r && (long)bi != self;
          if (EXCL) member = member && g.grp[s] != qg;
        }
        if (FILL) {
          const unsigned long long m = __ballot(member);
          const unsigned long long gm = W == 64 ? m : (m >> (sub * W)) & ((1ull << (W & 63)) - 1ull);
          if (member) {
            const long long slot = base + cnt + __popcll(gm & ((1ull << l) - 1ull));
            if (slot < end) {
              cand[slot] = bi;
              dist[slot] = d;
            } else {
              *err = 1;
            }
          }
          cnt += __popcll(gm);
        } else {
          cnt += member ? 1 : 0;
        }
      }
    }
  }
  if (!FILL) {
#pragma unroll
    for (int o = W / 2; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (l == 0 && q < Q) {
      counts[q] = cnt;
      if (visited != nullptr) visited[q] = vis;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// k-nearest: one wave per query row
__device__ __forceinline__ bool before(float ad, int ai, float bd, int bi) { return ad < bd || (ad == bd && ai < bi); }

struct KnnState {
  float ld;   // lane j: the j-th best distance seen (+inf: none)
  int li;     //         its row (EMPTY: none)
  int have;   // eligible rows seen
};

template <bool EXCL>
__device__ __forceinline__ void knn_span(const GridView& g, int s0, int s1, float qx, float qy, long self, long long qg,
                                         int k, int lane, KnnState& st) {
  for (int b = s0; b < s1; b += 64) {
    const int s = b + lane;
    bool ok = false;
    float d = __builtin_inff();
    int bi = EMPTY;
    if (s < s1) {
      const float2 p = g.pts[s];
      bi = g.row[s];
      d = grid_distance(qx, qy, p.x, p.y);
      ok = (long)bi != self;
      if (EXCL) ok = ok && g.grp[s] != qg;
    }
    const float wd = __shfl(st.ld, k - 1);
    const int wi = __shfl(st.li, k - 1);
    st.have += __popcll(__ballot(ok));
    unsigned long long m = __ballot(ok && before(d, bi, wd, wi));
    while (m != 0) {   // (wave-uniform) insert the survivors one by one: the list stays sorted by (distance, row)
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      const float cd = __shfl(d, src);
      const int ci = __shfl(bi, src);
      const int pos = __popcll(__ballot(lane < k && before(st.ld, st.li, cd, ci)));   // the entries ahead: a prefix
      const float ud = __shfl_up(st.ld, 1);
      const int ui = __shfl_up(st.li, 1);
      if (lane < k) {
        if (lane == pos) {
          st.ld = cd;
          st.li = ci;
        } else if (lane > pos) {
          st.ld = ud;
          st.li = ui;
        }
      }
    }
  }
}

// every cell of the rectangle o that is not in the rectangle v (v empty: vy0 > vy1)
template <bool EXCL>
__device__ __forceinline__ void knn_walk(const GridView& g, int ox0, int ox1, int oy0, int oy1, int vx0, int vx1, int vy0,
                                         int vy1, float qx, float qy, long self, long long qg, int k, int lane,
                                         KnnState& st) {
  for (int cy = oy0; cy <= oy1; ++cy) {
    const int rc = cy * g.G;
    int s0, s1;
    if (cy >= vy0 && cy <= vy1 && vx0 <= vx1) {
      const int b = ox1 < vx0 - 1 ? ox1 : vx0 - 1;
      if (ox0 <= b) {
        span_of(g, rc, ox0, b, s0, s1);
        knn_span<EXCL>(g, s0, s1, qx, qy, self, qg, k, lane, st);
      }
      const int a = ox0 > vx1 + 1 ? ox0 : vx1 + 1;
      if (a <= ox1) {
        span_of(g, rc, a, ox1, s0, s1);
        knn_span<EXCL>(g, s0, s1, qx, qy, self, qg, k, lane, st);
      }
    } else {
      span_of(g, rc, ox0, ox1, s0, s1);
      knn_span<EXCL>(g, s0, s1, qx, qy, self, qg, k, lane, st);
    }
  }
}

template <bool EXCL>
__global__ __launch_bounds__(256) void grid_knn_kernel(const GridView g, const float2* __restrict__ queries, long Q,
                                                       int k, long self_offset, const long long* __restrict__ qgrp,
                                                       long long* __restrict__ oidx, float* __restrict__ odist) {
  const int lane = threadIdx.x & 63;
  const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= Q) return;
  const float2 p = queries[q];
  const float qx = p.x, qy = p.y;
  if (!grid_finite(qx, qy)) {
    if (lane < k) {
      oidx[q * k + lane] = -1;
      odist[q * k + lane] = __builtin_nanf("");
    }
    return;
  }
  const int G = g.G;
  const float x0 = g.geom[0], y0 = g.geom[1], ihx = g.geom[2], ihy = g.geom[3];
  const int cx = cell_of(qx, x0, ihx, G), cy = cell_of(qy, y0, ihy, G);
  const long self = self_offset >= 0 ? q + self_offset : -1;
  const long long qg = EXCL ? qgrp[q] : 0;
  KnnState st{__builtin_inff(), EMPTY, 0};
  int vx0 = 1, vx1 = 0, vy0 = 1, vy1 = 0;
  bool all = false;
  for (int rho = 0;;) {
    const int nx0 = cx - rho > 0 ? cx - rho : 0, nx1 = cx + rho < G - 1 ? cx + rho : G - 1;
    const int ny0 = cy - rho > 0 ? cy - rho : 0, ny1 = cy + rho < G - 1 ? cy + rho : G - 1;
    knn_walk<EXCL>(g, nx0, nx1, ny0, ny1, vx0, vx1, vy0, vy1, qx, qy, self, qg, k, lane, st);
    vx0 = nx0, vx1 = nx1, vy0 = ny0, vy1 = ny1;
    all = nx0 == 0 && ny0 == 0 && nx1 == G - 1 && ny1 == G - 1;
    if (st.have >= k || all) break;
    rho = rho < 4 ? rho + 1 : 2 * rho;
  }
  if (!all) {   // k rows were seen: the answer lies within their k-th distance
    const float R = inflate(__shfl(st.ld, k - 1));
    int sx0, sx1, sy0, sy1;
    safe_cells(qx, R, x0, ihx, G, sx0, sx1);
    safe_cells(qy, R, y0, ihy, G, sy0, sy1);
    knn_walk<EXCL>(g, sx0, sx1, sy0, sy1, vx0, vx1, vy0, vy1, qx, qy, self, qg, k, lane, st);
  }
  if (lane < k) {
    oidx[q * k + lane] = st.li == EMPTY ? -1 : st.li;
    odist[q * k + lane] = st.li == EMPTY ? __builtin_inff() : st.ld;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
int check_grid(const char* who, int64_t n_query, int64_t n_bank, int cells, int flags, const void* geom,
               const void* cell_start, const void* pts, const void* rows, const void* sorted_group,
               const void* query_group) {
  if (n_query < 0 || n_query > 0x7fffffffLL || n_bank < 0 || n_bank > 0x7fffffffLL || cells < 1 ||
      cells > GRID_MAX_CELLS) {
    btsbot_set_error("%s: need 0 <= n_query, n_bank < 2^31 and 1 <= cells <= %d (n_query=%lld n_bank=%lld cells=%d)", who,
                     GRID_MAX_CELLS, (long long)n_query, (long long)n_bank, cells);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (flags != 0 && flags != BTSBOT_KNN_EXCLUDE_SAME) {
    btsbot_set_error("%s: flags must be 0 or BTSBOT_KNN_EXCLUDE_SAME, got %d", who, flags);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (flags != 0 && (query_group == nullptr || sorted_group == nullptr)) {
    btsbot_set_error("%s: BTSBOT_KNN_EXCLUDE_SAME needs query_group and sorted_group", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (geom == nullptr || cell_start == nullptr || (n_bank > 0 && (pts == nullptr || rows == nullptr))) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

GridView view_of(const float* geom, int cells, const int32_t* cell_start, const float* pts, const int32_t* rows,
                 const int64_t* sorted_group, int64_t n_bank) {
  return GridView{geom, cell_start, reinterpret_cast<const float2*>(pts), rows,
                  reinterpret_cast<const long long*>(sorted_group), cells, (int)n_bank};
}

template <int W, bool FILL>
int launch_radius(const GridView& g, const float* queries, int64_t nq, const float* radius, int64_t self_offset,
                  const int64_t* qgrp, bool excl, int64_t* counts, int64_t* visited, const int64_t* indptr, int32_t* cand,
                  float* dist, int32_t* err, hipStream_t st) {
  const unsigned blocks = (unsigned)((nq * W + 255) / 256);
  const auto* q2 = reinterpret_cast<const float2*>(queries);
  const auto* qg = reinterpret_cast<const long long*>(qgrp);
  auto* cn = reinterpret_cast<long long*>(counts);
  auto* vi = reinterpret_cast<long long*>(visited);
  const auto* ip = reinterpret_cast<const long long*>(indptr);
  if (excl)
    hipLaunchKernelGGL((grid_radius_kernel<W, FILL, true>), dim3(blocks), dim3(256), 0, st, g, q2, (long)nq, radius,
                       (long)self_offset, qg, cn, vi, ip, cand, dist, err);
  else
    hipLaunchKernelGGL((grid_radius_kernel<W, FILL, false>), dim3(blocks), dim3(256), 0, st, g, q2, (long)nq, radius,
                       (long)self_offset, qg, cn, vi, ip, cand, dist, err);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

template <bool FILL>
int launch_radius_lanes(int lanes, const char* who, const GridView& g, const float* queries, int64_t nq,
                        const float* radius, int64_t self_offset, const int64_t* qgrp, bool excl, int64_t* counts,
                        int64_t* visited, const int64_t* indptr, int32_t* cand, float* dist, int32_t* err,
                        hipStream_t st) {
  switch (lanes) {
    case 0:
    case 16:
      return launch_radius<16, FILL>(g, queries, nq, radius, self_offset, qgrp, excl, counts, visited, indptr, cand, dist,
                                     err, st);
    case 1:
      return launch_radius<1, FILL>(g, queries, nq, radius, self_offset, qgrp, excl, counts, visited, indptr, cand, dist,
                                    err, st);
    case 4:
      return launch_radius<4, FILL>(g, queries, nq, radius, self_offset, qgrp, excl, counts, visited, indptr, cand, dist,
                                    err, st);
    case 8:
      return launch_radius<8, FILL>(g, queries, nq, radius, self_offset, qgrp, excl, counts, visited, indptr, cand, dist,
                                    err, st);
    case 32:
      return launch_radius<32, FILL>(g, queries, nq, radius, self_offset, qgrp, excl, counts, visited, indptr, cand, dist,
                                     err, st);
    case 64:
      return launch_radius<64, FILL>(g, queries, nq, radius, self_offset, qgrp, excl, counts, visited, indptr, cand, dist,
                                     err, st);
  }
  btsbot_set_error("%s: lanes per query row must be 0 (the library's choice), 1, 4, 8, 16, 32 or 64, got %d", who, lanes);
  return BTSBOT_ERR_INVALID_ARG;
}

}  // namespace

extern "C" int btsbot_grid_finite(const float* points, int64_t n, uint8_t* finite, void* stream) {
  TRY(list_row::check_count("btsbot_grid_finite", "n", n));
  if (n == 0) return BTSBOT_OK;
  if (points == nullptr || finite == nullptr) {
    btsbot_set_error("btsbot_grid_finite: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(grid_finite_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float2*>(points), (long)n, finite);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_grid_cells(const float* points, int64_t n, const float* bbox, int cells, float* geom,
                                 int32_t* cell, void* stream) {
  if (n < 0 || n > 0x7fffffffLL || cells < 1 || cells > GRID_MAX_CELLS) {
    btsbot_set_error("btsbot_grid_cells: need 0 <= n < 2^31 and 1 <= cells <= %d (n=%lld cells=%d)", GRID_MAX_CELLS,
                     (long long)n, cells);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (bbox == nullptr || geom == nullptr || (n > 0 && (points == nullptr || cell == nullptr))) {
    btsbot_set_error("btsbot_grid_cells: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grid_geometry_kernel, dim3(1), dim3(64), 0, st, bbox, cells, geom);
  LAUNCH_CHECK();
  if (n == 0) return BTSBOT_OK;
  hipLaunchKernelGGL(grid_cell_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const float2*>(points), (long)n, (const float*)geom, cells, cell);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_grid_radius_count(const float* queries, int64_t n_query, const float* radius, const float* geom,
                                        int cells, const int32_t* cell_start, const float* sorted_points,
                                        const int32_t* sorted_rows, const int64_t* sorted_group, int64_t n_bank,
                                        int64_t self_offset, const int64_t* query_group, int flags, int lanes,
                                        int64_t* counts, int64_t* visited, void* stream) {
  const char* who = "btsbot_grid_radius_count";
  TRY(check_grid(who, n_query, n_bank, cells, flags, geom, cell_start, sorted_points, sorted_rows, sorted_group,
                 query_group));
  if (n_query == 0) return BTSBOT_OK;
  if (queries == nullptr || radius == nullptr || counts == nullptr) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const GridView g = view_of(geom, cells, cell_start, sorted_points, sorted_rows, sorted_group, n_bank);
  return launch_radius_lanes<false>(lanes, who, g, queries, n_query, radius, self_offset, query_group, flags != 0, counts,
                                    visited, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int btsbot_grid_radius_fill(const float* queries, int64_t n_query, const float* radius, const float* geom,
                                       int cells, const int32_t* cell_start, const float* sorted_points,
                                       const int32_t* sorted_rows, const int64_t* sorted_group, int64_t n_bank,
                                       int64_t self_offset, const int64_t* query_group, int flags, int lanes,
                                       const int64_t* indptr, int64_t total, int32_t* cand, float* dist,
                                       int32_t* error_flag, void* stream) {
  const char* who = "btsbot_grid_radius_fill";
  TRY(check_grid(who, n_query, n_bank, cells, flags, geom, cell_start, sorted_points, sorted_rows, sorted_group,
                 query_group));
  if (total < 0) {
    btsbot_set_error("%s: total=%lld must be >= 0", who, (long long)total);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query == 0 || total == 0) return BTSBOT_OK;
  if (queries == nullptr || radius == nullptr || indptr == nullptr || cand == nullptr || dist == nullptr ||
      error_flag == nullptr) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const GridView g = view_of(geom, cells, cell_start, sorted_points, sorted_rows, sorted_group, n_bank);
  return launch_radius_lanes<true>(lanes, who, g, queries, n_query, radius, self_offset, query_group, flags != 0, nullptr,
                                   nullptr, indptr, cand, dist, error_flag, (hipStream_t)stream);
}

extern "C" int btsbot_grid_knn(const float* queries, int64_t n_query, int k, const float* geom, int cells,
                               const int32_t* cell_start, const float* sorted_points, const int32_t* sorted_rows,
                               const int64_t* sorted_group, int64_t n_bank, int64_t self_offset,
                               const int64_t* query_group, int flags, int64_t* idx, float* dist, void* stream) {
  const char* who = "btsbot_grid_knn";
  TRY(check_grid(who, n_query, n_bank, cells, flags, geom, cell_start, sorted_points, sorted_rows, sorted_group,
                 query_group));
  if (k < 1 || k > GRID_MAX_K) {
    btsbot_set_error("%s: k=%d must be in 1..%d", who, k, GRID_MAX_K);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query == 0) return BTSBOT_OK;
  if (queries == nullptr || idx == nullptr || dist == nullptr) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const GridView g = view_of(geom, cells, cell_start, sorted_points, sorted_rows, sorted_group, n_bank);
  const unsigned blocks = (unsigned)((n_query + 3) / 4);
  const auto* q2 = reinterpret_cast<const float2*>(queries);
  const auto* qg = reinterpret_cast<const long long*>(query_group);
  auto* oi = reinterpret_cast<long long*>(idx);
  if (flags != 0)
    hipLaunchKernelGGL(grid_knn_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, q2, (long)n_query, k,
                       (long)self_offset, qg, oi, dist);
  else
    hipLaunchKernelGGL(grid_knn_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, q2, (long)n_query, k,
                       (long)self_offset, qg, oi, dist);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
