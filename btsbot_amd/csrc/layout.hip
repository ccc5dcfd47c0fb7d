// btsbot_layout_*: a deterministic UMAP layout of embedding rows (gfx950), DESIGN.md section 4n.
//
//   kNN graph (btsbot_knn_query, self first) -> smooth_knn: rho, sigma, memberships a_ij
//                                            -> symmetrize: CSR graph, w = (a_ij + a_ji) - a_ij a_ji, columns ascending
//                                            -> epochs: Y [n][2], one launch per epoch
//
// smooth_knn   one wave per row, one lane per neighbour (k <= 64).  umap-learn's smooth_knn_dist with local_connectivity
//              = 1 and bandwidth = 1; the bisection runs in float64 and sigma is rounded to fp32 once, so that a float64
//              restatement takes the same branches (the rule of alert_features.hip).
// symmetrize   every directed pair (i, j) gives two sort keys, i n + j ("forward") and j n + i ("reverse"); after one
//              radix sort (hipcub; stable, no atomics) the entries of an undirected edge's two CSR slots stand together.
//              The merge kernel marks the first entry of each key, an inclusive scan ranks the marks, and the fill kernel
//              writes column and weight of slot `rank` and finds indptr by binary search.  The structure depends on
//              the keys alone.  The one atomic is the maximum weight, whose result does not depend on order.
// epochs       a Jacobi form of umap-learn's optimize_layout_euclidean: epoch n reads Y_old and writes Y_new, a vertex is
//              written by its own group of 8 lanes only (a row of more than 128 slots by its workgroup's 256 threads).
//              Lane l of the group takes the row's CSR slots p0 + l, p0 + l + 8, ... in order, adds for each slot that
//              fires the attractive term and then the negative samples s = 0, 1, ... to its partial sum, and the
//              partial sums meet in a fixed butterfly: the summation order of a vertex depends on its row alone, never
//              on the grid or the run.
//              Negative samples come from a counter hash of (seed, epoch, slot, s); there is no RNG state.
//
//   kNN of new rows in a bank (btsbot_knn_query, no self) -> smooth_knn_query: sigma, memberships w_j (rho = 0)
//                                                         -> transform: positions of the new rows on the FIXED map of
//                                                            the bank, every epoch of the schedule in one launch (4o)
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace {

constexpr int MAX_K = 64, MAX_NSR = 64;
constexpr int G = 8;                 // lanes per vertex in the epoch kernel
constexpr int LONG_ROW = 128;        // a row of more slots than this is walked by the whole workgroup
constexpr int EPOCH_MAX_BLOCKS = 16384;
constexpr int TRANSFORM_MAX_BLOCKS = 65536;   // of one wave (8 queries) each

__host__ __device__ inline uint64_t mix64(uint64_t x) {   // splitmix64: the state step and the finaliser
  x += 0x9e3779b97f4a7c15ULL;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
  return x ^ (x >> 31);
}
// the hash of (seed, epoch, slot, sample) is mix64(hash_base(seed, epoch) + 64 slot + sample)
__host__ __device__ inline uint64_t hash_base(uint64_t seed, uint64_t epoch) { return mix64(seed ^ mix64(epoch)); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

// umap's bisection for sigma over one wave's row (lane = column): sum over the neighbours of exp(-max(x, 0) / sigma) =
// target.  The trips and branches are the same in every lane (psum is a wave sum).
__device__ __forceinline__ double bisect_sigma(bool nb, double x, double target) {
  double lo = 0.0, hi = __builtin_inf(), mid = 1.0;
  for (int trip = 0; trip < 64; ++trip) {
    const double psum = wave_sum_f64(nb ? (x > 0.0 ? exp(-(x / mid)) : 1.0) : 0.0);
    if (fabs(psum - target) < 1e-5) break;
    if (psum > target) {
      hi = mid;
      mid = (lo + hi) / 2.0;
    } else {
      lo = mid;
      if (hi == __builtin_inf()) mid *= 2.0;
      else mid = (lo + hi) / 2.0;
    }
  }
  return mid;
}

// ---------------------------------------------------------------------------------------------------------------------
// smooth_knn: one wave per row
__global__ __launch_bounds__(256) void layout_smooth_knn_kernel(const int64_t* __restrict__ idx, const float* __restrict__ dist,
                                                                long n, int k, double target,
                                                                const double* __restrict__ mean_all,
                                                                float* __restrict__ sigma, float* __restrict__ rho,
                                                                float* __restrict__ memb) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const bool in_row = lane < k;
  const int64_t j = in_row ? idx[row * k + lane] : -1;
  const float d32 = in_row ? dist[row * k + lane] : 0.f;
  const bool present = in_row && j >= 0;            // a -1 tail (fewer than k rows eligible) is no entry at all
  const bool nb = present && lane >= 1;             // column 0 is the row itself
  const double d = d32;
  const float r32 = wave_min_f32(nb && d32 > 0.f ? d32 : __builtin_inff());
  const double rh = r32 == __builtin_inff() ? 0.0 : (double)r32;
  const double x = d - rh;
  double mid = bisect_sigma(nb, x, target);
  const double cnt = wave_sum_f64(present ? 1.0 : 0.0);
  const double mean_row = cnt > 0.0 ? wave_sum_f64(present ? d : 0.0) / cnt : 0.0;
  const double floor_s = 1e-3 * (rh > 0.0 ? mean_row : *mean_all);
  if (mid < floor_s) mid = floor_s;
  const float s32 = (float)mid;
  if (lane == 0) {
    sigma[row] = s32;
    rho[row] = (float)rh;
  }
  if (in_row) {
    float a = 0.f;
    if (nb && j < n && j != row) a = x > 0.0 ? (float)exp(-(x / (double)s32)) : 1.f;
    memb[row * k + lane] = a;
  }
}

// The query side (umap-learn's transform: rows that are NOT in the bank): no self column, rho = 0, and the floor of sigma
// is 1e-3 x the mean of the row's OWN present distances -- nothing here depends on the other rows of the call.
__global__ __launch_bounds__(256) void layout_smooth_knn_query_kernel(const int64_t* __restrict__ idx,
                                                                      const float* __restrict__ dist, long n, int k,
                                                                      double target, float* __restrict__ sigma,
                                                                      float* __restrict__ memb) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const bool in_row = lane < k;
  const bool nb = in_row && idx[row * k + lane] >= 0;
  const double x = nb ? (double)dist[row * k + lane] : 0.0;
  double mid = bisect_sigma(nb, x, target);
  const double cnt = wave_sum_f64(nb ? 1.0 : 0.0);
  const double floor_s = cnt > 0.0 ? 1e-3 * (wave_sum_f64(x) / cnt) : 0.0;
  if (mid < floor_s) mid = floor_s;
  const float s32 = (float)mid;
  if (lane == 0) sigma[row] = s32;
  if (in_row) memb[row * k + lane] = nb ? (x > 0.0 ? (float)exp(-(x / (double)s32)) : 1.f) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
// symmetrize
__global__ __launch_bounds__(256) void layout_edge_keys_kernel(const int64_t* __restrict__ idx, long n, int k,
                                                               uint64_t* __restrict__ keys, uint32_t* __restrict__ slots,
                                                               float* __restrict__ w_max) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p == 0) *w_max = 0.f;
  if (p >= n * k) return;
  const long i = p / k;
  const int c = (int)(p - i * k);
  const int64_t j = idx[p];
  const bool valid = c >= 1 && j >= 0 && j < n && j != i;
  const uint64_t none = (uint64_t)n * (uint64_t)n;
  keys[2 * p] = valid ? (uint64_t)i * n + (uint64_t)j : none;
  keys[2 * p + 1] = valid ? (uint64_t)j * n + (uint64_t)i : none;
  slots[2 * p] = (uint32_t)(2 * p);
  slots[2 * p + 1] = (uint32_t)(2 * p + 1);
}

__global__ __launch_bounds__(256) void layout_merge_kernel(const uint64_t* __restrict__ skeys, long m, uint64_t none,
                                                           uint32_t* __restrict__ head) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= m) return;
  const uint64_t key = skeys[q];
  head[q] = (key != none && (q == 0 || skeys[q - 1] != key)) ? 1u : 0u;
}

// threads [0, m): the first entry of a key writes the slot; threads [m, m + n]: indptr of row (thread - m)
__global__ __launch_bounds__(256) void layout_csr_fill_kernel(const uint64_t* __restrict__ skeys,
                                                              const uint32_t* __restrict__ sslots,
                                                              const uint32_t* __restrict__ head,
                                                              const uint32_t* __restrict__ rank,
                                                              const float* __restrict__ memb, long m, long n,
                                                              int64_t* __restrict__ indptr, int32_t* __restrict__ indices,
                                                              float* __restrict__ weights, float* __restrict__ w_max) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q < m) {
    if (head[q] == 0u) return;
    const uint64_t key = skeys[q];
    float fwd = 0.f, rev = 0.f;
    for (long t = q; t < m && skeys[t] == key; ++t) {
      const uint32_t s = sslots[t];
      const float a = memb[s >> 1];
      if (s & 1u) rev = fmaxf(rev, a);
      else fwd = fmaxf(fwd, a);
    }
    // umap-learn's probabilistic union in exactly this form (no contraction): bitwise symmetric in fwd, rev
    const float w = __fsub_rn(__fadd_rn(fwd, rev), __fmul_rn(fwd, rev));
    const long e = (long)rank[q] - 1;
    indices[e] = (int32_t)(key % (uint64_t)n);
    weights[e] = w;
    if (w > 0.f) atomicMax(reinterpret_cast<unsigned*>(w_max), __float_as_uint(w));   // w >= 0: the bits order as the values
    return;
  }
  const long r = q - m;
  if (r > n) return;
  const uint64_t want = (uint64_t)r * (uint64_t)n;
  long lo = 0, hi = m;   // the first entry whose key is >= want
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (skeys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  indptr[r] = lo == m ? (int64_t)rank[m - 1] : (int64_t)rank[lo] - (int64_t)head[lo];
}

// ---------------------------------------------------------------------------------------------------------------------
// initial positions: mode 0 uniform in [-10, 10), mode 1 adds a jitter in +-1e-4 (epoch 0 of the hash, slot = vertex)
__global__ __launch_bounds__(256) void layout_init_kernel(float* __restrict__ y, long n, uint64_t base, int mode) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * n) return;
  const uint64_t h = mix64(base + 64ULL * (uint64_t)(t >> 1) + (uint64_t)(t & 1));
  const double u = (double)(h >> 40) * (1.0 / 16777216.0);
  y[t] = mode == 0 ? (float)(20.0 * u - 10.0) : (float)((double)y[t] + (2.0 * u - 1.0) * 1e-4);
}

// ---------------------------------------------------------------------------------------------------------------------
// one epoch
struct EpochArgs {
  const int64_t* indptr;
  const int32_t* indices;
  const float* weights;
  const float* w_max;
  const float2* yin;
  float2* yout;
  long n;
  int epoch, nsr;
  float a, b, alpha;
  uint64_t base;
};

__device__ __forceinline__ float clip4(float v) { return fminf(fmaxf(v, -4.f), 4.f); }

// what CSR slot p adds to vertex v in this epoch: nothing unless it fires; then the attractive term, then the negative
// samples s = 0, 1, ... in order
__device__ __forceinline__ void slot_terms(const EpochArgs& A, long v, float2 yv, long p, float wmax, float& sx, float& sy) {
  const float a = A.a, b = A.b;
  // r_e = fp32(w / w_max); the slot fires when floor(n r) > floor((n - 1) r), both products exact in float64
  const double r = (double)__fdiv_rn(A.weights[p], wmax);
  if (!(floor((double)A.epoch * r) > floor((double)(A.epoch - 1) * r))) return;
  const float2 yu = A.yin[A.indices[p]];
  const uint64_t h0 = A.base + 64ULL * (uint64_t)p;
  {
    const float dx = yv.x - yu.x, dy = yv.y - yu.y;
    const float d2 = dx * dx + dy * dy;
    if (d2 > 0.f) {
      const float L = log2f(d2);   // d2^b and d2^(b-1) share it
      const float c = -2.f * a * b * exp2f((b - 1.f) * L) / (1.f + a * exp2f(b * L));
      // the factor 2: the reverse slot (u, v) has the same weight and schedule, and umap moves both ends
      sx += 2.f * clip4(c * dx);
      sy += 2.f * clip4(c * dy);
    }
  }
  const uint32_t un = (uint32_t)A.n;
  for (int s0 = 0; s0 < A.nsr; s0 += 4) {
    uint32_t t[4];
    float2 yt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      t[i] = __umulhi((uint32_t)(mix64(h0 + (uint64_t)(s0 + i)) >> 32), un);   // < n
      if (s0 + i < A.nsr) yt[i] = A.yin[t[i]];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (s0 + i >= A.nsr || (long)t[i] == v || !(isfinite(yt[i].x) && isfinite(yt[i].y))) continue;
      const float dx = yv.x - yt[i].x, dy = yv.y - yt[i].y;
      const float d2 = dx * dx + dy * dy;
      if (d2 > 0.f) {
        const float c = 2.f * b / ((0.001f + d2) * (1.f + a * exp2f(b * log2f(d2))));
        sx += clip4(c * dx);
        sy += clip4(c * dy);
      } else {
        sx += 4.f;
        sy += 4.f;
      }
    }
  }
}

// A workgroup takes GPB = 32 consecutive vertices per round.  A row of at most LONG_ROW slots belongs to its group of 8
// lanes (slots p0 + l, p0 + l + 8, ...).  A longer one -- the hubs of a kNN graph in many dimensions reach thousands of
// slots, and eight lanes walking one of them alone held up the whole epoch: 0.25 ms of 0.25 at N = 100,000 -- is then
// taken by all 256 threads (slots p0 + t, p0 + t + 256, ...), whose partial sums meet in a 64-lane butterfly and, wave
// 0 to 3 in order, through LDS.  Either way the order is a function of the row alone.
__global__ __launch_bounds__(256) void layout_epoch_kernel(const EpochArgs A) {
  constexpr int GPB = 256 / G;
  __shared__ int is_long[GPB];
  __shared__ float2 wave_part[4];
  const int tid = threadIdx.x, lane = tid % G, grp = tid / G;
  const long stride = (long)gridDim.x * GPB;
  const float wmax = *A.w_max;
  for (long v0 = (long)blockIdx.x * GPB; v0 < A.n; v0 += stride) {   // the same trips for every thread of the workgroup
    const long v = v0 + grp;
    if (v < A.n) {
      const long p0 = A.indptr[v], p1 = A.indptr[v + 1];
      const bool longer = p1 - p0 > LONG_ROW;
      if (lane == 0) is_long[grp] = longer;
      if (!longer) {
        const float2 yv = A.yin[v];
        float sx = 0.f, sy = 0.f;
        for (long p = p0 + lane; p < p1; p += G) slot_terms(A, v, yv, p, wmax, sx, sy);
#pragma unroll
        for (int o = G / 2; o >= 1; o >>= 1) {
          sx += __shfl_xor(sx, o);
          sy += __shfl_xor(sy, o);
        }
        if (lane == 0) A.yout[v] = make_float2(__fmaf_rn(A.alpha, sx, yv.x), __fmaf_rn(A.alpha, sy, yv.y));
      }
    } else if (lane == 0) {
      is_long[grp] = 0;
    }
    __syncthreads();
    for (int j = 0; j < GPB; ++j) {
      if (!is_long[j]) continue;   // uniform over the workgroup
      const long vl = v0 + j;
      const float2 yv = A.yin[vl];
      const long p1 = A.indptr[vl + 1];
      float sx = 0.f, sy = 0.f;
      for (long p = A.indptr[vl] + tid; p < p1; p += 256) slot_terms(A, vl, yv, p, wmax, sx, sy);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        sx += __shfl_xor(sx, o);
        sy += __shfl_xor(sy, o);
      }
      if ((tid & 63) == 0) wave_part[tid >> 6] = make_float2(sx, sy);
      __syncthreads();
      if (tid == 0) {
        sx = ((wave_part[0].x + wave_part[1].x) + wave_part[2].x) + wave_part[3].x;
        sy = ((wave_part[0].y + wave_part[1].y) + wave_part[2].y) + wave_part[3].y;
        A.yout[vl] = make_float2(__fmaf_rn(A.alpha, sx, yv.x), __fmaf_rn(A.alpha, sy, yv.y));
      }
      __syncthreads();
    }
    __syncthreads();   // is_long is rewritten in the next round
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// transform: new rows placed on the fixed map of a bank
struct TransformArgs {
  const int64_t* idx;   // [q][k] rows of the bank, -1 = absent
  const float* w;       // [q][k] memberships
  const float2* bank;   // [n_bank] map positions, fixed
  const float2* yin;    // [q]; may be yout
  float2* yout;         // [q]
  long q;
  uint32_t n_bank;
  int k, n_epochs, first, last, nsr;
  float a, b, lr;
  uint64_t seed;
};

// the start: the mean of the neighbours' positions weighted by the memberships, float64 in slot order, rounded once
__global__ __launch_bounds__(256) void layout_transform_init_kernel(const TransformArgs A) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= A.q) return;
  double sw = 0.0, sx = 0.0, sy = 0.0;
  for (int j = 0; j < A.k; ++j) {
    const int64_t u = A.idx[q * A.k + j];
    if (u < 0 || u >= (int64_t)A.n_bank) continue;
    const double wj = A.w[q * A.k + j];
    const float2 yu = A.bank[u];
    sw = __dadd_rn(sw, wj);
    sx = __dadd_rn(sx, __dmul_rn(wj, (double)yu.x));
    sy = __dadd_rn(sy, __dmul_rn(wj, (double)yu.y));
  }
  A.yout[q] = make_float2((float)(sx / sw), (float)(sy / sw));   // no slot present: 0 / 0 = NaN
}

// A group of G = 8 lanes owns one query for the whole schedule.  Lane l holds the slots l, l + 8, ... (S of them at
// most) in registers: the neighbour's fixed position and r = fp32(w / w_rowmax).  With the bank fixed a query depends on
// nothing but its own row, so the epochs first..last run here back to back: the position stays in registers, only the
// negative samples are gathered, and the one store is lane 0's after the last epoch.  No LDS, no barrier, no atomic.
// The sum order of an epoch (lane: slots in order, per firing slot the attractive term then the samples in order; then a
// 3-step xor butterfly, which leaves the same bits in all eight lanes) is a function of the row alone.
template <int S>
__global__ __launch_bounds__(64) void layout_transform_kernel(const TransformArgs A) {
  constexpr int GPB = 64 / G;
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  const float a = A.a, b = A.b;
  const int k = A.k;
  for (long q0 = (long)blockIdx.x * GPB; q0 < A.q; q0 += (long)gridDim.x * GPB) {
    const long q = q0 + grp;
    if (q >= A.q) continue;   // a whole group leaves together; the butterfly never crosses groups
    const int64_t* ri = A.idx + q * k;
    const float* rw = A.w + q * k;
    // rowkey: what makes the samples of a row a function of the row alone
    uint64_t key = 0;
    float wmax = 0.f;
    for (int j = 0; j < k; ++j) {
      const float wj = rw[j];
      key = mix64(key + (((uint64_t)(uint32_t)ri[j] << 32) | (uint64_t)__float_as_uint(wj)));
      wmax = fmaxf(wmax, wj);
    }
    float2 yn[S];
    float r[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const int j = lane + G * i;
      const int64_t u = j < k ? ri[j] : -1;
      const bool present = u >= 0 && u < (int64_t)A.n_bank;
      yn[i] = present ? A.bank[u] : make_float2(0.f, 0.f);
      r[i] = present ? __fdiv_rn(rw[j], wmax) : 0.f;   // w_rowmax = 0: NaN, which never fires
    }
    float2 y = A.yin[q];
    for (int n = A.first; n <= A.last; ++n) {
      const uint64_t base = hash_base(A.seed, (uint64_t)n) + key + 64ULL * (uint64_t)lane;
      float sx = 0.f, sy = 0.f;
#pragma unroll
      for (int i = 0; i < S; ++i) {
        const double rd = (double)r[i];
        if (!(floor((double)n * rd) > floor((double)(n - 1) * rd))) continue;
        {
          // one end moves only: no factor 2
          const float dx = y.x - yn[i].x, dy = y.y - yn[i].y;
          const float d2 = dx * dx + dy * dy;
          if (d2 > 0.f) {
            const float L = log2f(d2);
            const float c = -2.f * a * b * exp2f((b - 1.f) * L) / (1.f + a * exp2f(b * L));
            sx += clip4(c * dx);
            sy += clip4(c * dy);
          }
        }
        const uint64_t h0 = base + 64ULL * (uint64_t)(G * i);
        for (int s0 = 0; s0 < A.nsr; s0 += 8) {
          float2 yt[8];
#pragma unroll
          for (int s = 0; s < 8; ++s) {   // the gathers of up to eight samples are in flight together
            yt[s] = make_float2(__builtin_nanf(""), 0.f);
            if (s0 + s < A.nsr) yt[s] = A.bank[__umulhi((uint32_t)(mix64(h0 + (uint64_t)(s0 + s)) >> 32), A.n_bank)];
          }
#pragma unroll
          for (int s = 0; s < 8; ++s) {
            if (!(isfinite(yt[s].x) && isfinite(yt[s].y))) continue;
            const float dx = y.x - yt[s].x, dy = y.y - yt[s].y;
            const float d2 = dx * dx + dy * dy;
            if (d2 > 0.f) {
              const float c = 2.f * b / ((0.001f + d2) * (1.f + a * exp2f(b * log2f(d2))));
              sx += clip4(c * dx);
              sy += clip4(c * dy);
            } else {
              sx += 4.f;
              sy += 4.f;
            }
          }
        }
      }
#pragma unroll
      for (int o = G / 2; o >= 1; o >>= 1) {
        sx += __shfl_xor(sx, o);
        sy += __shfl_xor(sy, o);
      }
      // umap-learn's transform starts at initial_alpha / 4
      const float alpha = (float)((double)A.lr / 4.0 * (1.0 - (double)(n - 1) / (double)A.n_epochs));
      y = make_float2(__fmaf_rn(alpha, sx, y.x), __fmaf_rn(alpha, sy, y.y));
    }
    if (lane == 0) A.yout[q] = y;
  }
}

int check_graph_shape(const char* who, int64_t n, int k) {
  if (n < 0 || k < 2 || k > MAX_K || 2 * n * (int64_t)k >= 0x7fffffffLL) {
    btsbot_set_error("%s: need n >= 0, 2 <= k <= %d and 2 n k < 2^31 (n=%lld k=%d)", who, MAX_K, (long long)n, k);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

int key_bits(int64_t n) {   // bits that hold every key, n * n included
  const uint64_t top = (uint64_t)n * (uint64_t)n;
  int bits = 1;
  while (bits < 64 && (top >> bits) != 0) ++bits;
  return bits;
}

struct SymLayout {
  size_t keys, skeys, slots, sslots, head, rank, tmp, tmp_bytes, total;
};
int sym_layout(int64_t n, int k, SymLayout& L) {
  const size_t m = 2 * (size_t)n * k;
  size_t sort_b = 0, scan_b = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                             (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)m, 0, key_bits(n),
                                             (hipStream_t) nullptr));
  HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)m,
                                           (hipStream_t) nullptr));
  size_t cur = 0;
  L.keys = bump(cur, m * 8);
  L.skeys = bump(cur, m * 8);
  L.slots = bump(cur, m * 4);
  L.sslots = bump(cur, m * 4);
  L.head = bump(cur, m * 4);
  L.rank = bump(cur, m * 4);
  L.tmp_bytes = sort_b > scan_b ? sort_b : scan_b;
  L.tmp = bump(cur, L.tmp_bytes);
  L.total = cur;
  return BTSBOT_OK;
}

}  // namespace

extern "C" int btsbot_layout_smooth_knn(const int64_t* idx, const float* dist, int64_t n, int k, const double* mean_all,
                                        float* sigma, float* rho, float* memb, void* stream) {
  TRY(check_graph_shape("btsbot_layout_smooth_knn", n, k));
  if (n == 0) return BTSBOT_OK;
  if (idx == nullptr || dist == nullptr || mean_all == nullptr || sigma == nullptr || rho == nullptr || memb == nullptr) {
    btsbot_set_error("btsbot_layout_smooth_knn: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(layout_smooth_knn_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, idx, dist,
                     (long)n, k, log2((double)k), mean_all, sigma, rho, memb);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_layout_smooth_knn_query(const int64_t* idx, const float* dist, int64_t q, int k, float* sigma,
                                              float* w, void* stream) {
  TRY(check_graph_shape("btsbot_layout_smooth_knn_query", q, k));
  if (q == 0) return BTSBOT_OK;
  if (idx == nullptr || dist == nullptr || sigma == nullptr || w == nullptr) {
    btsbot_set_error("btsbot_layout_smooth_knn_query: NULL argument");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(layout_smooth_knn_query_kernel, dim3((unsigned)((q + 3) / 4)), dim3(256), 0, (hipStream_t)stream, idx,
                     dist, (long)q, k, log2((double)k), sigma, w);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_layout_transform(const int64_t* idx, const float* w, const float* bank_y, int64_t n_bank, int64_t q,
                                       int k, const float* y0, float* yout, int n_epochs, int first_epoch, int last_epoch,
                                       float a, float b, uint64_t seed, int negative_sample_rate, float learning_rate,
                                       int blocks, void* stream) {
  TRY(check_graph_shape("btsbot_layout_transform", q, k));
  const bool start_only = first_epoch == 1 && last_epoch == 0 && y0 == nullptr;   // the weighted-mean start, no epoch
  if (n_bank < 0 || n_bank > 0x7fffffffLL || n_epochs < 1 || first_epoch < 1 || last_epoch > n_epochs ||
      (first_epoch > last_epoch && !start_only) || negative_sample_rate < 0 || negative_sample_rate > MAX_NSR ||
      blocks < 0) {
    btsbot_set_error("btsbot_layout_transform: need 0 <= n_bank < 2^31, 1 <= first_epoch <= last_epoch <= n_epochs (or "
                     "epochs 1..0 without y0: the start alone), 0 <= negative_sample_rate <= %d, blocks >= 0 (n_bank=%lld "
                     "epochs %d..%d of %d, rate %d, blocks %d)", MAX_NSR, (long long)n_bank, first_epoch, last_epoch,
                     n_epochs, negative_sample_rate, blocks);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (first_epoch > 1 && y0 == nullptr) {
    btsbot_set_error("btsbot_layout_transform: first_epoch = %d needs y0, the positions after epoch %d", first_epoch,
                     first_epoch - 1);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (q == 0) return BTSBOT_OK;
  if (n_bank == 0) {
    btsbot_set_error("btsbot_layout_transform: the bank is empty (q=%lld)", (long long)q);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (idx == nullptr || w == nullptr || bank_y == nullptr || yout == nullptr || ((uintptr_t)bank_y & 7) != 0 ||
      ((uintptr_t)yout & 7) != 0 || ((uintptr_t)y0 & 7) != 0) {
    btsbot_set_error("btsbot_layout_transform: NULL argument, or positions not 8-byte aligned");
    return BTSBOT_ERR_INVALID_ARG;
  }
  TransformArgs A;
  A.idx = idx;
  A.w = w;
  A.bank = reinterpret_cast<const float2*>(bank_y);
  A.yin = reinterpret_cast<const float2*>(y0 != nullptr ? y0 : yout);
  A.yout = reinterpret_cast<float2*>(yout);
  A.q = (long)q;
  A.n_bank = (uint32_t)n_bank;
  A.k = k;
  A.n_epochs = n_epochs;
  A.first = first_epoch;
  A.last = last_epoch;
  A.nsr = negative_sample_rate;
  A.a = a;
  A.b = b;
  A.lr = learning_rate;
  A.seed = seed;
  hipStream_t st = (hipStream_t)stream;
  if (y0 == nullptr) {
    hipLaunchKernelGGL(layout_transform_init_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, st, A);
    LAUNCH_CHECK();
  }
  if (start_only) return BTSBOT_OK;
  constexpr int GPB = 64 / G;
  long grid = (q + GPB - 1) / GPB;
  if (blocks > 0) grid = grid < blocks ? grid : blocks;
  else if (grid > TRANSFORM_MAX_BLOCKS) grid = TRANSFORM_MAX_BLOCKS;
  const dim3 g((unsigned)grid), t(64);
  if (k <= 2 * G) hipLaunchKernelGGL(layout_transform_kernel<2>, g, t, 0, st, A);
  else if (k <= 4 * G) hipLaunchKernelGGL(layout_transform_kernel<4>, g, t, 0, st, A);
  else hipLaunchKernelGGL(layout_transform_kernel<8>, g, t, 0, st, A);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int64_t btsbot_layout_symmetrize_workspace(int64_t n, int k) {
  if (check_graph_shape("btsbot_layout_symmetrize_workspace", n, k) != BTSBOT_OK) return BTSBOT_ERR_INVALID_ARG;
  if (n == 0) return 0;
  SymLayout L;
  const int s = sym_layout(n, k, L);
  return s != BTSBOT_OK ? (int64_t)s : (int64_t)L.total;
}

extern "C" int btsbot_layout_symmetrize(const int64_t* idx, const float* memb, int64_t n, int k, int64_t* indptr,
                                        int32_t* indices, float* weights, float* w_max, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  TRY(check_graph_shape("btsbot_layout_symmetrize", n, k));
  if (indptr == nullptr || w_max == nullptr) {
    btsbot_set_error("btsbot_layout_symmetrize: NULL indptr / w_max");
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    TRY(launch_fill0(reinterpret_cast<float*>(indptr), 2, st));
    return launch_fill0(w_max, 1, st);
  }
  SymLayout L;
  TRY(sym_layout(n, k, L));
  if (idx == nullptr || memb == nullptr || indices == nullptr || weights == nullptr || workspace == nullptr ||
      ((uintptr_t)workspace & 255) != 0 || workspace_bytes < (int64_t)L.total) {
    btsbot_set_error("btsbot_layout_symmetrize: NULL argument, workspace of %lld bytes (need %zu) or not 256-byte aligned",
                     (long long)workspace_bytes, L.total);
    return BTSBOT_ERR_INVALID_ARG;
  }
  unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
  uint64_t* keys = reinterpret_cast<uint64_t*>(ws + L.keys);
  uint64_t* skeys = reinterpret_cast<uint64_t*>(ws + L.skeys);
  uint32_t* slots = reinterpret_cast<uint32_t*>(ws + L.slots);
  uint32_t* sslots = reinterpret_cast<uint32_t*>(ws + L.sslots);
  uint32_t* head = reinterpret_cast<uint32_t*>(ws + L.head);
  uint32_t* rank = reinterpret_cast<uint32_t*>(ws + L.rank);
  const long m = 2 * (long)n * k;
  hipLaunchKernelGGL(layout_edge_keys_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, st, idx, (long)n, k, keys,
                     slots, w_max);
  LAUNCH_CHECK();
  size_t tmp_bytes = L.tmp_bytes;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(ws + L.tmp, tmp_bytes, (const uint64_t*)keys, skeys, (const uint32_t*)slots,
                                             sslots, (int)m, 0, key_bits(n), st));
  hipLaunchKernelGGL(layout_merge_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, skeys, m,
                     (uint64_t)n * (uint64_t)n, head);
  LAUNCH_CHECK();
  tmp_bytes = L.tmp_bytes;
  HIP_TRY(hipcub::DeviceScan::InclusiveSum(ws + L.tmp, tmp_bytes, (const uint32_t*)head, rank, (int)m, st));
  hipLaunchKernelGGL(layout_csr_fill_kernel, dim3((unsigned)((m + n + 1 + 255) / 256)), dim3(256), 0, st, skeys, sslots, head,
                     rank, memb, m, (long)n, indptr, indices, weights, w_max);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_layout_init(float* y, int64_t n, uint64_t seed, int mode, void* stream) {
  if (n < 0 || n > 0x7fffffffLL || (mode != 0 && mode != 1) || (n > 0 && y == nullptr)) {
    btsbot_set_error("btsbot_layout_init: need 0 <= n < 2^31, mode 0 (uniform) or 1 (jitter) and y (n=%lld mode=%d)",
                     (long long)n, mode);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n == 0) return BTSBOT_OK;
  hipLaunchKernelGGL(layout_init_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, (long)n,
                     hash_base(seed, 0), mode);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_layout_epochs(const int64_t* indptr, const int32_t* indices, const float* weights, const float* w_max,
                                    int64_t n, float* y_a, float* y_b, int n_epochs, int first_epoch, int last_epoch, float a,
                                    float b, uint64_t seed, int negative_sample_rate, float learning_rate, int blocks,
                                    void* stream) {
  if (n < 0 || n > 0x7fffffffLL || n_epochs < 1 || first_epoch < 1 || last_epoch > n_epochs || first_epoch > last_epoch ||
      negative_sample_rate < 0 || negative_sample_rate > MAX_NSR || blocks < 0) {
    btsbot_set_error("btsbot_layout_epochs: need 0 <= n < 2^31, 1 <= first_epoch <= last_epoch <= n_epochs, 0 <= "
                     "negative_sample_rate <= %d, blocks >= 0 (n=%lld epochs %d..%d of %d, rate %d, blocks %d)", MAX_NSR,
                     (long long)n, first_epoch, last_epoch, n_epochs, negative_sample_rate, blocks);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n == 0) return BTSBOT_OK;
  if (indptr == nullptr || indices == nullptr || weights == nullptr || w_max == nullptr || y_a == nullptr || y_b == nullptr ||
      ((uintptr_t)y_a & 7) != 0 || ((uintptr_t)y_b & 7) != 0 || y_a == y_b) {
    btsbot_set_error("btsbot_layout_epochs: NULL argument, y_a == y_b, or positions not 8-byte aligned");
    return BTSBOT_ERR_INVALID_ARG;
  }
  constexpr int GPB = 256 / G;
  long grid = (n + GPB - 1) / GPB;
  if (blocks > 0) grid = grid < blocks ? grid : blocks;
  else if (grid > EPOCH_MAX_BLOCKS) grid = EPOCH_MAX_BLOCKS;
  EpochArgs A;
  A.indptr = indptr;
  A.indices = indices;
  A.weights = weights;
  A.w_max = w_max;
  A.n = (long)n;
  A.nsr = negative_sample_rate;
  A.a = a;
  A.b = b;
  float* src = y_a;
  float* dst = y_b;
  for (int e = first_epoch; e <= last_epoch; ++e) {
    A.yin = reinterpret_cast<const float2*>(src);
    A.yout = reinterpret_cast<float2*>(dst);
    A.epoch = e;
    A.alpha = (float)((double)learning_rate * (1.0 - (double)(e - 1) / (double)n_epochs));
    A.base = hash_base(seed, (uint64_t)e);
    hipLaunchKernelGGL(layout_epoch_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, A);
    LAUNCH_CHECK();
    float* t = src;
    src = dst;
    dst = t;
  }
  return BTSBOT_OK;
}
