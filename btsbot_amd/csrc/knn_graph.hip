// btsbot_knn_graph_merge: offers of new rows merged into the neighbour lists of old rows, in place (gfx950), DESIGN.md
// section 4x.  btsbot_knn_graph_compact, the lists after rows were removed, is at the end of the file (section 4y).
//
// A list is what btsbot_knn_query writes: k slots, the present entries (idx >= 0) first, ordered by (dist, idx), then a
// -1 / +inf tail.  A row's offers are a slice of a CSR, ordered by (dist, idx) too, and every offer index is larger than
// every list index (the offers are NEW rows), so in the merged (dist, idx) order an old entry goes before an offer of the
// same dist.  The list becomes the first k of the merge; under DISTINCT an entry is emitted only if its group differs
// from every entry emitted before it.
//
// One wave per row, lane c the list's column c (k <= 64).  The row is read whole into registers before anything is
// written, the wave is the only writer of the row, and nothing is written unless an offer enters: the result is a
// function of the row's own list and offers, no atomic touches a list.  A row without offers ends after its two indptr
// reads.
//
//   plain     only the first min(k, offers) offers can matter: one per lane.  No sort: for every offer j, in order, one
//             ballot gives the present old entries at or before it -- its place is j + that count --, and every old
//             entry counts the offers strictly before it -- its place is its column + that count.  The loop ends at the
//             first offer whose place is >= k (every later one lies behind it).  Work: k + the offers that enter.
//   DISTINCT  a two-pointer walk over (list, offers) in merged order, the offers fetched 64 at a time; lane e keeps the
//             e-th emitted entry and one ballot answers "group seen before".  It ends at k emitted groups.
#include "list_row.h"

namespace {

constexpr int GM_MAX_K = 64;
constexpr int GM_MAX_K_DISTINCT = 32;
constexpr int WG = 256;
constexpr int WAVE = 64;

__device__ __forceinline__ void mark_changed(long row, int lane, uint8_t* __restrict__ changed_rows,
                                             int32_t* __restrict__ changed_count) {
  if (lane != 0) return;
  if (changed_rows != nullptr) changed_rows[row] = 1;
  if (changed_count != nullptr) atomicAdd(changed_count, 1);
}

template <bool DISTINCT>
__global__ __launch_bounds__(WG) void knn_graph_merge_kernel(int64_t* __restrict__ idx, float* __restrict__ dist, long stride,
                                                            int k, long n_old, const int64_t* __restrict__ indptr,
                                                            const int64_t* __restrict__ offer_idx,
                                                            const float* __restrict__ offer_dist, long n_offers,
                                                            const int64_t* __restrict__ groups, long n_groups,
                                                            const int64_t* __restrict__ rows, long n_rows,
                                                            uint8_t* __restrict__ changed_rows,
                                                            int32_t* __restrict__ changed_count) {
  const int lane = threadIdx.x % WAVE;
  const long w = (long)blockIdx.x * (WG / WAVE) + threadIdx.x / WAVE;   // (a whole wave leaves together throughout)
  long row = w;
  if (rows != nullptr) {
    if (w >= n_rows) return;
    row = (long)rows[w];
  }
  if (row < 0 || row >= n_old) return;
  const long beg = (long)indptr[row], end = (long)indptr[row + 1];
  if (end <= beg || beg < 0 || end > n_offers) return;
  const long n_off = end - beg;

  int64_t* const li = idx + row * stride;
  float* const ld = dist + row * stride;
  const float inf = __builtin_inff();
  const bool in_row = lane < k;
  const int64_t oi = in_row ? li[lane] : -1;
  const float od = in_row ? ld[lane] : inf;
  const float d0 = __shfl(od, 0, WAVE);
  if (d0 != d0) return;   // a non-finite row: -1 / NaN throughout, and it stays so
  const bool present = oi >= 0;

  if (!DISTINCT) {
    const int n_take = (int)(n_off < (long)k ? n_off : (long)k);
    const bool has = lane < n_take;
    const int64_t fi = has ? offer_idx[beg + lane] : -1;
    const float fd = has ? offer_dist[beg + lane] : inf;
    int before = 0;      // an old entry: the offers strictly before it
    int place = k;       // an offer: where it goes
    int entered = 0;
    for (int j = 0; j < n_take; ++j) {
      const float d = __shfl(fd, j, WAVE);
      const int p = j + __popcll(__ballot(present && od <= d));
      if (p >= k) break;
      if (lane == j) place = p;
      before += (present && d < od) ? 1 : 0;
      entered = j + 1;
    }
    if (entered == 0) return;
    // an old entry behind an offer the loop did not reach has before == entered and column + entered >= k: it leaves
    if (present && before > 0 && lane + before < k) {
      li[lane + before] = oi;
      ld[lane + before] = od;
    }
    if (lane < entered) {
      li[place] = fi;
      ld[place] = fd;
    }
    mark_changed(row, lane, changed_rows, changed_count);
  } else {
    const int m = __popcll(__ballot(present));   // the present entries are columns 0 .. m - 1
    const int64_t og = (present && oi < n_groups) ? groups[oi] : 0;
    int64_t ei = -1, eg = 0;   // lane e: the e-th emitted entry
    float ed = inf;
    int64_t fi = -1, fg = 0;   // lane t: offer chunk + t
    float fd = inf;
    long chunk = -WAVE;
    int i = 0, emitted = 0;
    long j = 0;
    bool offer_entered = false;
    while (emitted < k && (i < m || j < n_off)) {
      if (j < n_off && j >= chunk + WAVE) {
        chunk = j;
        const long t = chunk + lane;
        const bool has = t < n_off;
        fi = has ? offer_idx[beg + t] : -1;
        fd = has ? offer_dist[beg + t] : inf;
        fg = (has && fi >= 0 && fi < n_groups) ? groups[fi] : 0;
      }
      const int a = i < m ? i : 0;
      const int b = j < n_off ? (int)(j - chunk) : 0;
      const float ad = __shfl(od, a, WAVE), bd = __shfl(fd, b, WAVE);
      const bool take_offer = i >= m || (j < n_off && bd < ad);   // (an old entry wins a tie in dist)
      const int64_t ci = take_offer ? __shfl(fi, b, WAVE) : __shfl(oi, a, WAVE);
      const int64_t cg = take_offer ? __shfl(fg, b, WAVE) : __shfl(og, a, WAVE);
      const float cd = take_offer ? bd : ad;
      if (__ballot(lane < emitted && eg == cg) == 0) {
        if (lane == emitted) {
          ei = ci;
          eg = cg;
          ed = cd;
        }
        ++emitted;
        offer_entered |= take_offer;
      }
      if (take_offer) ++j; else ++i;
    }
    if (!offer_entered) return;   // no offer emitted: every old entry was, in its own place
    if (in_row) {
      li[lane] = lane < emitted ? ei : -1;
      ld[lane] = lane < emitted ? ed : inf;
    }
    mark_changed(row, lane, changed_rows, changed_count);
  }
}

using list_row::misaligned;

// ---- btsbot_knn_graph_compact: the lists of the surviving rows, renumbered, out of place.
//
// W lanes hold old row a, lane c its column c (list_row.h).  A streaming pass, 12 k bytes per row in and out, with one
// 8-byte gather per entry into new_of_old, which stays in L2 at a million rows.  The lanes of a removed row leave after
// their one (broadcast) read of new_of_old[a]; the others read the row whole, map every present entry through new_of_old,
// and one ballot over the row's lanes gives a surviving entry its new column: the survivors before it.  Input and output
// do not overlap (the entry refuses it), so a row is its group's to write in any order; lane c also writes the tail slot
// c where c is past the survivors.  The two counters take at most two atomics per wave, from its first active lane.
template <int W>
__global__ __launch_bounds__(list_row::WG) void knn_graph_compact_kernel(
    const int64_t* __restrict__ idx, const float* __restrict__ dist, long stride, int k, long n_old,
    const int64_t* __restrict__ new_of_old, int64_t* __restrict__ out_idx, float* __restrict__ out_dist, long out_stride,
    long n_new, bool distinct, uint8_t* __restrict__ damaged, int32_t* __restrict__ counts) {
  const int c = list_row::lane_col<W>();
  const long a = list_row::lane_row<W>();
  if (a >= n_old) return;   // (a whole group leaves together throughout)
  const long j = (long)new_of_old[a];
  if (j < 0 || j >= n_new) return;
  const bool in_row = c < k;
  const float inf = __builtin_inff();
  const int64_t e = in_row ? idx[a * stride + c] : -1;
  const float d = in_row ? dist[a * stride + c] : inf;
  int64_t* const oi = out_idx + j * out_stride;
  float* const od = out_dist + j * out_stride;
  const float d0 = __shfl(d, 0, W);
  if (d0 != d0) {   // a non-finite row: copied as it stands
    if (in_row) {
      oi[c] = e;
      od[c] = d;
    }
    if (c == 0) damaged[j] = 0;
    return;
  }
  const bool present = e >= 0;
  const int64_t m = (present && e < n_old) ? new_of_old[e] : -1;   // (an entry out of range is never a subscript)
  const bool survives = m >= 0;
  const int base = (threadIdx.x % WAVE) & ~(W - 1);   // where the group's lanes stand in the wave's ballot
  const unsigned long long ones = W == 64 ? ~0ull : ((1ull << (W % 64)) - 1);
  const unsigned long long dropped_wave = __ballot(present && !survives);
  const unsigned long long kept_mask = (__ballot(survives) >> base) & ones;
  const unsigned long long present_mask = (__ballot(present) >> base) & ones;
  const bool any_dropped = ((dropped_wave >> base) & ones) != 0;
  const int kept = __popcll(kept_mask);
  const bool full = ((present_mask >> (k - 1)) & 1ull) != 0;
  const bool dam = any_dropped && (full || distinct);
  if (survives) {
    const int at = __popcll(kept_mask & ((1ull << c) - 1));
    oi[at] = m;
    od[at] = d;
  }
  if (in_row && c >= kept) {
    oi[c] = -1;
    od[c] = inf;
  }
  if (c == 0) damaged[j] = dam ? 1 : 0;
  if (counts != nullptr) {
    const unsigned long long active = __ballot(true);
    const unsigned long long dam_wave = __ballot(c == 0 && dam);
    if ((int)(threadIdx.x % WAVE) == __ffsll((long long)active) - 1) {
      if (dam_wave != 0) atomicAdd(counts, __popcll(dam_wave));
      if (dropped_wave != 0) atomicAdd(counts + 1, __popcll(dropped_wave));
    }
  }
}

// [p, p + bytes) and [q, q + bytes_q) share a byte
inline bool overlap(const void* p, int64_t bytes, const void* q, int64_t bytes_q) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)bytes_q && b < a + (uintptr_t)bytes;
}

}  // namespace

extern "C" int btsbot_knn_graph_merge(int64_t* idx, float* dist, int64_t stride, int k, int64_t n_old, const int64_t* indptr,
                                      const int64_t* offer_idx, const float* offer_dist, int64_t n_offers,
                                      const int64_t* groups, int64_t n_groups, int flags, const int64_t* rows, int64_t n_rows,
                                      uint8_t* changed_rows, int32_t* changed_count, void* stream) {
  const char* who = "btsbot_knn_graph_merge";
  const bool distinct = (flags & BTSBOT_KNN_GRAPH_DISTINCT) != 0;
  if ((flags & ~BTSBOT_KNN_GRAPH_DISTINCT) != 0) {
    btsbot_set_error("%s: unknown flags %d", who, flags);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int max_k = distinct ? GM_MAX_K_DISTINCT : GM_MAX_K;
  if (k < 1 || k > max_k || stride < k) {
    btsbot_set_error("%s: need 1 <= k <= %d%s and stride >= k (k=%d stride=%lld)", who, max_k,
                     distinct ? " (the distinct mode)" : "", k, (long long)stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int64_t lim = 0x7fffffffLL;
  if (n_old < 0 || n_old > lim || n_offers < 0 || n_offers > lim || n_groups < 0 || n_groups > lim ||
      (rows != nullptr && (n_rows < 0 || n_rows > lim))) {
    btsbot_set_error("%s: need 0 <= n_old, n_offers, n_groups, n_rows < 2^31 (n_old=%lld n_offers=%lld n_groups=%lld "
                     "n_rows=%lld)", who, (long long)n_old, (long long)n_offers, (long long)n_groups, (long long)n_rows);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (distinct && groups == nullptr) {
    btsbot_set_error("%s: BTSBOT_KNN_GRAPH_DISTINCT needs groups", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int64_t visits = rows != nullptr ? n_rows : n_old;
  if (n_old == 0 || n_offers == 0 || visits == 0) return BTSBOT_OK;
  if (idx == nullptr || dist == nullptr || indptr == nullptr || offer_idx == nullptr || offer_dist == nullptr) {
    btsbot_set_error("%s: NULL argument (only groups, rows, changed_rows and changed_count may be NULL)", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (misaligned(idx, 8) || misaligned(dist, 4) || misaligned(indptr, 8) || misaligned(offer_idx, 8) ||
      misaligned(offer_dist, 4) || misaligned(groups, 8) || misaligned(rows, 8) || misaligned(changed_count, 4)) {
    btsbot_set_error("%s: misaligned argument (int64 arrays: 8 bytes; dist, offer_dist, changed_count: 4)", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const dim3 grid((unsigned)((visits + WG / WAVE - 1) / (WG / WAVE)));
  const hipStream_t s = (hipStream_t)stream;
  if (distinct)
    hipLaunchKernelGGL(knn_graph_merge_kernel<true>, grid, dim3(WG), 0, s, idx, dist, (long)stride, k, (long)n_old, indptr,
                       offer_idx, offer_dist, (long)n_offers, groups, (long)n_groups, rows, (long)n_rows, changed_rows,
                       changed_count);
  else
    hipLaunchKernelGGL(knn_graph_merge_kernel<false>, grid, dim3(WG), 0, s, idx, dist, (long)stride, k, (long)n_old, indptr,
                       offer_idx, offer_dist, (long)n_offers, groups, (long)n_groups, rows, (long)n_rows, changed_rows,
                       changed_count);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_knn_graph_compact(const int64_t* idx, const float* dist, int64_t stride, int k, int64_t n_old,
                                        const int64_t* new_of_old, int64_t* out_idx, float* out_dist, int64_t out_stride,
                                        int64_t n_new, int flags, uint8_t* damaged, int32_t* counts, void* stream) {
  const char* who = "btsbot_knn_graph_compact";
  const bool distinct = (flags & BTSBOT_KNN_GRAPH_DISTINCT) != 0;
  if ((flags & ~BTSBOT_KNN_GRAPH_DISTINCT) != 0) {
    btsbot_set_error("%s: unknown flags %d", who, flags);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int max_k = distinct ? GM_MAX_K_DISTINCT : GM_MAX_K;
  if (k < 1 || k > max_k || stride < k || out_stride < k) {
    btsbot_set_error("%s: need 1 <= k <= %d%s, stride >= k and out_stride >= k (k=%d stride=%lld out_stride=%lld)", who, max_k,
                     distinct ? " (the distinct mode)" : "", k, (long long)stride, (long long)out_stride);
    return BTSBOT_ERR_INVALID_ARG;
  }
  TRY(list_row::check_count(who, "n_old", n_old));
  TRY(list_row::check_count(who, "n_new", n_new));
  if (n_new > n_old) {
    btsbot_set_error("%s: n_new=%lld survivors of n_old=%lld rows", who, (long long)n_new, (long long)n_old);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_old == 0 || n_new == 0) return BTSBOT_OK;
  if (idx == nullptr || dist == nullptr || new_of_old == nullptr || out_idx == nullptr || out_dist == nullptr ||
      damaged == nullptr) {
    btsbot_set_error("%s: NULL argument (only counts may be NULL)", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (misaligned(idx, 8) || misaligned(dist, 4) || misaligned(new_of_old, 8) || misaligned(out_idx, 8) ||
      misaligned(out_dist, 4) || misaligned(counts, 4)) {
    btsbot_set_error("%s: misaligned argument (int64 arrays: 8 bytes; dist, out_dist, counts: 4)", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const int64_t in_slots = (n_old - 1) * stride + k, out_slots = (n_new - 1) * out_stride + k;
  const void* const in_p[3] = {idx, dist, new_of_old};
  const int64_t in_b[3] = {in_slots * 8, in_slots * 4, n_old * 8};
  const void* const out_p[3] = {out_idx, out_dist, damaged};
  const int64_t out_b[3] = {out_slots * 8, out_slots * 4, n_new};
  for (int i = 0; i < 3; ++i)
    for (int o = 0; o < 3; ++o)
      if (overlap(in_p[i], in_b[i], out_p[o], out_b[o])) {
        btsbot_set_error("%s: an output array overlaps an input array (the lists are compacted out of place)", who);
        return BTSBOT_ERR_INVALID_ARG;
      }
  const hipStream_t s = (hipStream_t)stream;
  list_row::for_lanes(list_row::lanes_for(k), [&](auto w) {
    constexpr int W = decltype(w)::value;
    hipLaunchKernelGGL(knn_graph_compact_kernel<W>, list_row::row_grid((long)n_old, W), dim3(list_row::WG), 0, s, idx, dist,
                       (long)stride, k, (long)n_old, new_of_old, out_idx, out_dist, (long)out_stride, (long)n_new, distinct,
                       damaged, counts);
  });
  LAUNCH_CHECK();
  return BTSBOT_OK;
}
