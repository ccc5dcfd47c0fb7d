// btsbot_kmeans_* / btsbot_ivf_*: the partitioned form of the embedding index (gfx950), DESIGN.md section 4ab.
//
// The rows are cut into lists around k-means centroids; a query searches only the lists of its nprobe nearest centroids.
// The answer is EXACTLY the k-nearest answer over the rows of the probed lists -- the selection scores, the merge and the
// returned distances are those of btsbot_knn_query (knn.hip), on the shared pieces of knn_tile.h --; which lists are
// looked at is the only approximation, and it is made by the caller (the probes are an input here).
//
//   btsbot_kmeans_update   centroids from rows and labels, deterministic, no atomic on a sum.  The rows of a cluster, in
//                          ascending row order, are cut into chunks of KM_CHUNK rows counted from the CLUSTER's first row;
//                          pass 1 sums a chunk's rows one after the other per column (one read of the fp32 rows, coalesced
//                          over the columns), pass 2 adds a cluster's partial sums in chunk order and divides by the count.
//                          A centroid's bits depend on its cluster's rows and on KM_CHUNK only.
//   btsbot_ivf_layout      the list-ordered operand image: the packed records (knn.hip) in list order, every list starting
//                          on a 128-row tile boundary and padded with the record the packer writes for a non-finite row
//                          (bias +inf: its score is +inf and is never kept), so no epilogue learns about padding.
//   btsbot_ivf_query       the listed tile pass and its merge.  A work item is one list and at most 128 of the queries that
//                          probe it; the items come from a histogram of the (query, probe) pairs over the lists, its scan
//                          and a fill, all on the device.  The grid is the upper bound ceil(Q * nprobe / 128) + n_lists;
//                          surplus workgroups leave at once.  The query records are read through the item's row map.
//
// Both item tables (chunks of clusters, query tiles of lists) are made the same way: hist_kernel counts, scan_kernel gives
// every bin its first entry and its first item, and a workgroup finds its bin by a binary search over the item starts.
// The only atomics are integer counters: the histogram, and the slot a pair takes inside its list's run of pairs.  Which
// slot -- hence which item and which tile row -- a pair gets differs from run to run; its partial list does not, because a
// score depends on its two records alone and a list is the k best of what it was offered whatever the order (knn.hip).
//
// Groups (btsbot_ivf_query_grouped).  A row may carry a group, any int64 (an alert's object), and the probed search takes
// the two switches of btsbot_knn_query_grouped with the same contract over the rows of the probed lists.  Both kernels
// are templates on the group mode GM, as knn.hip's are; GM = 0 is the text above, unchanged, and is what btsbot_ivf_query
// launches.  The selection's indices are positions of the list image, so the groups are banked in list order:
// btsbot_ivf_layout_groups gathers list_group[position] = bank_group[row_of[position]] (0 at a padding position, whose
// score is +inf and which is therefore never offered: its group is never read as a candidate's), 8 bytes per row next to
// a record of 2.1 KB.  A tile's 128 groups are requested under the products, one per thread, and parked in the idle
// operand LDS at TG_OFF (load_tile_group, knn_tile.h), exactly as knn.hip does it.
//   GM & 1, exclude   the query groups of a lane's four tile rows sit in registers, taken from query_group[pair /
//                     nprobe] through the item's row map; one more term in the mask of what may be offered.  self_rows
//                     stays the position compare it is and combines with every mode.
//   GM & 2, one per group   offer_one (knn_tile.h).  The groups of the list entries live in the workspace, not in LDS
//                     (knn.hip says why), as lg[j * pairs + slot], an int64 [k][n_query * nprobe] array, 8 k bytes per
//                     (query, probe) pair -- 7.9 MB at Q = 8,192, nprobe = 8, k = 15 --: slot = first + tile row is the
//                     pair's place in its list's run of pairs, unique and below n_query * nprobe, so an entry is only
//                     ever touched by the slot's owner thread and the owners of an item read and write neighbouring
//                     words.  No host read and no n_lists term: a block per work item would be [items][k][128] over the
//                     grid's upper bound, about 1 GiB at 65,536 lists and k = 15.  k <= 32 in this mode (MAX_K_ONE).
// Order-independence in the listed pass.  Inside one list the positions ascend with the original row number, so "a
// group's best by (score, position)" is its best by (score, row), and knn.hip's argument -- the list is the k best of
// B(S), the best row of every group offered so far, whatever the order of the offers -- holds per work item as written.
// Which slot a pair takes still differs from run to run; its list does not.
// The merge.  A group's rows may lie in several probed lists, so this is where they meet.  After the pool's positions
// are mapped to original rows, GM & 2 drops every pool entry that has an entry of its own group before it by (score,
// row) and ranks among the rest (keep_group_bests, knn_tile.h, shared with knn_merge_kernel).  This is knn.hip's split
// argument with "list" for "split": a group's best over the probed lists is the best of its list-bests; it is in its
// list's k unless k other groups' bests of that list are before it, and then it is not among the k best groups overall
// either.  A row that is not its group's best over the probed lists either loses to its group's entry in the pool, or
// its group's best was pushed out of a list by k groups' bests, each represented in the pool by a kept entry no worse
// -- rank >= k.  The pool is nprobe * k <= 32 * 32 entries and their 8 KB of groups, on chip.
// New code here has no inline assembly; the only atomics are the integer LDS and global counters named above.
#include "knn_tile.h"

namespace {

constexpr int BCAP = 8;          // candidates a query row's bucket holds per round (as knn.hip)
constexpr int KM_CHUNK = 64;     // rows per partial sum
constexpr int KM_COLS = 256;     // columns per workgroup
constexpr int MAX_LISTS = 65536;
constexpr int SCAN_T = 1024;

// ---------------------------------------------------------------------------------------------------------------------
// the item tables
// cnt[key] += 1 for 0 <= key < n_bins, cnt[n_bins] += 1 for a negative key; a key >= n_bins is not counted
__global__ __launch_bounds__(256) void hist_kernel(const long long* __restrict__ keys, long n, int n_bins,
                                                   int* __restrict__ cnt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long key = keys[i];
  if (key < 0) atomicAdd(&cnt[n_bins], 1);
  else if (key < n_bins) atomicAdd(&cnt[(int)key], 1);
}

// One workgroup.  start[b] = the entries of the bins before b, istart[b] = their items, an item being `unit` entries of
// one bin (the last one of a bin may be short); both [n_bins + 1].  sizes: NULL, or int64 [n_bins] that receives cnt.
__global__ __launch_bounds__(SCAN_T) void scan_kernel(const int* __restrict__ cnt, int n_bins, int unit,
                                                      int* __restrict__ start, int* __restrict__ istart,
                                                      long long* __restrict__ sizes) {
  __shared__ int sa[SCAN_T], sb[SCAN_T];
  const int t = threadIdx.x;
  const int per = (n_bins + SCAN_T - 1) / SCAN_T;
  const int b0 = min(t * per, n_bins), b1 = min(b0 + per, n_bins);
  int ta = 0, tb = 0;
  for (int b = b0; b < b1; ++b) {
    const int c = cnt[b];
    ta += c;
    tb += (c + unit - 1) / unit;
  }
  sa[t] = ta;
  sb[t] = tb;
  __syncthreads();
  for (int o = 1; o < SCAN_T; o <<= 1) {
    const int xa = t >= o ? sa[t - o] : 0, xb = t >= o ? sb[t - o] : 0;
    __syncthreads();
    sa[t] += xa;
    sb[t] += xb;
    __syncthreads();
  }
  int a = sa[t] - ta, i = sb[t] - tb;
  for (int b = b0; b < b1; ++b) {
    const int c = cnt[b];
    start[b] = a;
    istart[b] = i;
    if (sizes != nullptr) sizes[b] = c;
    a += c;
    i += (c + unit - 1) / unit;
  }
  if (t == SCAN_T - 1) {
    start[n_bins] = sa[t];
    istart[n_bins] = sb[t];
  }
}

// the bin of item w: istart[b] <= w < istart[b + 1] (w < istart[n_bins])
__device__ __forceinline__ int bin_of_item(const int* __restrict__ istart, int n_bins, int w) {
  int lo = 0, hi = n_bins - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (istart[mid + 1] <= w) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------------------
// k-means update
// pass 1: item = (cluster, chunk of KM_CHUNK of its rows), grid.y = blocks of KM_COLS columns, a thread per column
__global__ __launch_bounds__(KM_COLS) void kmeans_partial_kernel(const float* __restrict__ rows, long n_rows, int dim,
                                                                 const long long* __restrict__ order, int n_clusters,
                                                                 const int* __restrict__ cnt,
                                                                 const int* __restrict__ start,
                                                                 const int* __restrict__ istart,
                                                                 float* __restrict__ part) {
  __shared__ long at[KM_CHUNK];
  const int w = blockIdx.x;
  if (w >= istart[n_clusters]) return;
  const int c = bin_of_item(istart, n_clusters, w);
  const int j = w - istart[c];
  // the sorted order holds the rows of negative label first
  const long first = (long)cnt[n_clusters] + start[c] + (long)j * KM_CHUNK;
  const int n = min(KM_CHUNK, cnt[c] - j * KM_CHUNK);
  const int tid = threadIdx.x;
  if (tid < KM_CHUNK) {
    long r = -1;
    if (tid < n && first + tid < n_rows) {
      r = order[first + tid];
      if (r < 0 || r >= n_rows) r = -1;
    }
    at[tid] = r;
  }
  __syncthreads();
  const int col = blockIdx.y * KM_COLS + tid;
  if (col >= dim) return;
  float s = 0.f;
#pragma unroll 8
  for (int e = 0; e < n; ++e) {
    const long r = at[e];
    const float v = r >= 0 ? rows[r * dim + col] : 0.f;
    s = e == 0 ? v : s + v;
  }
  part[(size_t)w * dim + col] = s;
}

// pass 2: a cluster's partial sums in chunk order, then the mean.  An empty cluster's centroid is left as it is.
__global__ __launch_bounds__(KM_COLS) void kmeans_final_kernel(const float* __restrict__ part, int dim, int n_clusters,
                                                               const int* __restrict__ cnt,
                                                               const int* __restrict__ istart,
                                                               float* __restrict__ centroids,
                                                               long long* __restrict__ counts) {
  const int c = blockIdx.x;
  const int n = cnt[c];
  if (blockIdx.y == 0 && threadIdx.x == 0) counts[c] = n;
  const int col = blockIdx.y * KM_COLS + threadIdx.x;
  if (n == 0 || col >= dim) return;
  const int i0 = istart[c], i1 = istart[c + 1];
  float s = part[(size_t)i0 * dim + col];
#pragma unroll 8
  for (int i = i0 + 1; i < i1; ++i) s += part[(size_t)i * dim + col];
  centroids[(size_t)c * dim + col] = s / (float)n;
}

struct KmeansWs {
  size_t cnt, start, istart, part, total;
  KmeansWs(int64_t n_rows, int dim, int n_clusters) {
    const size_t bins = align256(((size_t)n_clusters + 1) * sizeof(int));
    cnt = 0;
    start = bins;
    istart = 2 * bins;
    part = 3 * bins;
    total = part + align256(((size_t)n_rows / KM_CHUNK + (size_t)n_clusters) * (size_t)dim * sizeof(float));
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// layout
// the sorted row at `i` (behind the rows of negative label) goes to its list's next position
__global__ __launch_bounds__(256) void ivf_place_kernel(const long long* __restrict__ labels,
                                                        const long long* __restrict__ order, long n_bank, int n_lists,
                                                        const int* __restrict__ cnt, const int* __restrict__ start,
                                                        const int* __restrict__ tstart, long n_list_rows,
                                                        int* __restrict__ row_of, int* __restrict__ pos_of) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_bank) return;
  const long long r = order[i];
  if (r < 0 || r >= n_bank) return;
  const long long l = labels[r];
  long pos = -1;
  if (l >= 0 && l < n_lists) {
    const long in_list = i - cnt[n_lists] - start[l];
    if (in_list >= 0 && in_list < cnt[l]) pos = (long)tstart[l] * TB + in_list;
    if (pos >= n_list_rows) pos = -1;
  }
  pos_of[r] = (int)pos;
  if (pos >= 0) row_of[pos] = (int)r;
}

// the list image: position p holds the record of bank row row_of[p], or the padding record.  16 bytes per thread.
__global__ __launch_bounds__(256) void ivf_gather_kernel(const unsigned char* __restrict__ packed,
                                                         const int* __restrict__ row_of, long n_list_rows, int rec16,
                                                         unsigned char* __restrict__ out) {
  const long p = blockIdx.x;
  const int r = row_of[p];
  uint4* o = reinterpret_cast<uint4*>(out + (size_t)p * rec16 * 16);
  if (r >= 0) {
    const uint4* s = reinterpret_cast<const uint4*>(packed + (size_t)r * rec16 * 16);
    for (int c = threadIdx.x; c < rec16; c += 256) o[c] = s[c];
  } else {
    for (int c = threadIdx.x; c < rec16; c += 256) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (c == 0) v.x = __float_as_uint(__builtin_inff());   // bias +inf, scale 0, a zero image
      o[c] = v;
    }
  }
}

// the groups in list order: position p holds the group of bank row row_of[p], 0 at a padding position
__global__ __launch_bounds__(256) void ivf_gather_groups_kernel(const long long* __restrict__ bank_group,
                                                                const int* __restrict__ row_of, long n_list_rows,
                                                                long n_bank, long long* __restrict__ list_group) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_list_rows) return;
  const int r = row_of[p];
  list_group[p] = r >= 0 && r < n_bank ? bank_group[r] : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// query: the (query, probe) pairs into their lists' runs
__global__ __launch_bounds__(256) void ivf_fill_kernel(const long long* __restrict__ probes, long n_pairs, int n_lists,
                                                       const int* __restrict__ pstart, int* __restrict__ cursor,
                                                       int* __restrict__ pair_at) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pairs) return;
  const long long l = probes[i];
  if (l < 0 || l >= n_lists) return;
  const int slot = atomicAdd(&cursor[(int)l], 1);
  const long at = (long)pstart[l] + slot;
  if (at < n_pairs) pair_at[at] = (int)i;
}

// The listed selection.  Item blockIdx.x = list l and the pairs pair_at[first .. first + nq) that probe it; tile row r is
// query pair_at[first + r] / nprobe.  The list's tiles [tstart[l], tstart[l + 1]) of the list image are walked as
// knn_select_kernel walks a split; an index is a POSITION of the list image (ascending in the row number inside a list).
// cand[pair][k] receives the row's list.  GM != 0: qgrp = the query rows' groups, lgrp = the groups in list order; GM & 2:
// lg = the groups of the list entries, entry j of the pair at slot s at lg[j * lg_stride + s], lg_stride = Q * nprobe.
template <int GM>
__global__ __launch_bounds__(256, 2) void ivf_select_kernel(const unsigned char* __restrict__ qimg,
                                                            const unsigned char* __restrict__ limg, long n_list_rows,
                                                            int dim, int k, int nprobe, int n_lists, long n_bank,
                                                            const int* __restrict__ pstart,
                                                            const int* __restrict__ istart,
                                                            const int* __restrict__ pair_at,
                                                            const int* __restrict__ tstart,
                                                            const long long* __restrict__ self_rows,
                                                            const int* __restrict__ pos_of, Cand* __restrict__ cand,
                                                            const long long* __restrict__ qgrp,
                                                            const long long* __restrict__ lgrp,
                                                            long long* __restrict__ lg, long lg_stride) {
  constexpr int MI = TileWalk::MI, NI = TileWalk::NI;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int w = blockIdx.x;
  if (w >= istart[n_lists]) return;
  unsigned char* Qh = smem;
  unsigned char* Ql = Qh + TQ * ROWB;
  unsigned char* Bh = Ql + TQ * ROWB;
  unsigned char* Bl = Bh + TB * ROWB;
  Cand* L = reinterpret_cast<Cand*>(smem + GEMM_LDS);   // [TQ][k] lists
  int* qpair = reinterpret_cast<int*>(L + TQ * k);      // [TQ] the tile rows' pairs, -1 past the item's end
  Cand* bucket = reinterpret_cast<Cand*>(smem);         // behind a tile's products, as knn.hip
  int* bcnt = reinterpret_cast<int*>(bucket + TQ * BCAP);
  float* thr = reinterpret_cast<float*>(bcnt + TQ);
  int* flag = reinterpret_cast<int*>(thr + TQ);
  long long* tg = reinterpret_cast<long long*>(smem + TG_OFF);   // GM != 0: [TB] the tile's groups

  const int tid = threadIdx.x;
  const LanePos p;
  const int dp = padded_dim(dim);
  const size_t rec = record_bytes(dim);
  const int nk = (dp + BK - 1) / BK;

  const int l = bin_of_item(istart, n_lists, w);
  const int first = pstart[l] + (w - istart[l]) * TQ;
  const int nq = min(TQ, pstart[l + 1] - first);
  const int total_tiles = (int)(n_list_rows / TB);
  const int t_begin = min(tstart[l], total_tiles), t_end = min(tstart[l + 1], total_tiles);

  float ts = __builtin_inff();
  int ti = EMPTY, tp = 0;
  if (tid < TQ) {
    for (int j = 0; j < k; ++j) L[tid * k + j] = Cand{__builtin_inff(), EMPTY};
    qpair[tid] = tid < nq ? pair_at[first + tid] : -1;
  }
  __syncthreads();
  const bool owner = tid < TQ && qpair[tid] >= 0;

  float sq[MI];
  int selfb[MI];   // the position of the list image that IS the query row, -1: none
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int pr = qpair[p.qrow(mi)];
    sq[mi] = 0.f;
    selfb[mi] = -1;
    if (pr >= 0) {
      const long q = pr / nprobe;
      sq[mi] = reinterpret_cast<const float*>(qimg + q * rec)[1];
      if (self_rows != nullptr) {
        const long long s = self_rows[q];
        if (s >= 0 && s < n_bank) selfb[mi] = pos_of[s];
      }
    }
  }
  long long qg[MI];   // GM & GM_EXCLUDE: the groups of the lane's four tile rows
  if constexpr ((GM & GM_EXCLUDE) != 0) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int pr = qpair[p.qrow(mi)];
      qg[mi] = pr >= 0 ? qgrp[pr / nprobe] : 0;   // (a row past the item's end never has a candidate)
    }
  }
  // GM & GM_ONE: the groups of this thread's list entries (an owner's slot first + tid is below lg_stride)
  long long* LG = lg + ((long)first + tid);
  long qoff[CH];   // the records of the rows this thread loads chunks of, -1: none
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int pr = qpair[(tid + i * 256) >> 3];
    qoff[i] = pr >= 0 ? (long)(pr / nprobe) * (long)rec : -1;
  }

  uint4 qh[CH], ql[CH], bh[CH], bl[CH];
  auto gload = [&](int tile, int kt) {
    const int k0 = kt * BK;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + i * 256, row = c >> 3, gk = k0 + (c & 7) * 8;
      const bool kin = gk < dp;
      const unsigned char* pq = qimg + (qoff[i] >= 0 ? qoff[i] : 0) + HDR + gk * 2;
      const unsigned char* pb = limg + ((long)tile * TB + row) * rec + HDR + gk * 2;   // (tile < total_tiles)
      const bool okq = kin && qoff[i] >= 0;
      qh[i] = okq ? *reinterpret_cast<const uint4*>(pq) : make_uint4(0, 0, 0, 0);
      ql[i] = okq ? *reinterpret_cast<const uint4*>(pq + 2 * dp) : make_uint4(0, 0, 0, 0);
      bh[i] = kin ? *reinterpret_cast<const uint4*>(pb) : make_uint4(0, 0, 0, 0);
      bl[i] = kin ? *reinterpret_cast<const uint4*>(pb + 2 * dp) : make_uint4(0, 0, 0, 0);
    }
  };
  auto sstore = [&]() { tile_sstore(smem, qh, ql, bh, bl, tid); };

  if (t_begin < t_end) gload(t_begin, 0);
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int b0 = tile * TB;
    long long gt = 0;   // GM != 0: the group at position b0 + tid, in flight under the products
    if constexpr (GM != 0) gt = load_tile_group(lgrp, b0, (int)n_list_rows);
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
#pragma unroll 1
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

    // ---- the tile's candidates (knn.hip): the owners publish their worst kept scores in the idle operand planes
    if (tid < TQ) {
      thr[tid] = owner ? ts : -__builtin_inff();   // (a row past the item's end never has a candidate)
      bcnt[tid] = 0;
      if constexpr (GM != 0) tg[tid] = gt;
    }
    if (tid < 2) flag[tid] = 0;
    lds_barrier();
    float t[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) t[mi] = thr[p.qrow(mi)];
    unsigned long long mask = 0;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float nb[4], sb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float2 h = *reinterpret_cast<const float2*>(limg + (size_t)p.gb(b0, ni, i) * rec);
        nb[i] = h.x;
        sb[i] = h.y;
      }
      long long bg[4];   // GM & GM_EXCLUDE: the fragment's groups
      if constexpr ((GM & GM_EXCLUDE) != 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bg[i] = tg[p.wn * 64 + ni * 16 + p.lq * 4 + i];   // (p.brow(ni, i), as knn.hip)
      }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int gb = p.gb(b0, ni, i);
          const float s = tile_score(acc[ni][mi][i], sq[mi], sb[i], nb[i]);
          acc[ni][mi][i] = s;
          bool in = s <= t[mi] && s < __builtin_inff() && gb != selfb[mi];
          if constexpr ((GM & GM_EXCLUDE) != 0) in = in && bg[i] != qg[mi];
          if (in) mask |= 1ull << ((ni * MI + mi) * 4 + i);
        }
    }
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
      if (tid == 0) flag[(rc + 1) & 1] = 0;
      lds_barrier();
      if (owner) {
        const int n = min(bcnt[tid], BCAP);
        for (int e = 0; e < n; ++e) {
          const Cand c = bucket[tid * BCAP + e];
          if constexpr ((GM & GM_ONE) != 0) offer_one(L + tid * k, LG, lg_stride, k, c.s, b0 + c.i, tg[c.i], ts, ti, tp);
          else offer(L + tid * k, k, c.s, b0 + c.i, ts, ti, tp);
        }
        thr[tid] = ts;
      }
      if (tid < TQ) bcnt[tid] = 0;
      const int more = flag[rc & 1];
      lds_barrier();
      if (more == 0) break;
    }
  }

  if (owner) {
    Cand* o = cand + (size_t)qpair[tid] * k;
    for (int j = 0; j < k; ++j) o[j] = L[tid * k + j];
  }
}

// merge, one wave per query (knn_merge_kernel): the pool is the query's nprobe * k candidates, their positions mapped to
// original row numbers before any comparison; the k best by (score, row), each one's distance in the direct form from
// the fp32 rows by direct_distance() -- the function btsbot_knn_query applies --, ordered by (dist, row).  A probe outside
// 0 .. n_lists - 1 has no item and contributes nothing.  GM & GM_ONE (the header's argument): the entries' groups are read
// at their positions, lgrp, and only a group's best entry by (score, row) is ranked.
template <int GM>
__global__ __launch_bounds__(64) void ivf_merge_kernel(const float* __restrict__ queries, const float* __restrict__ bank,
                                                       long n_bank, const Cand* __restrict__ cand,
                                                       const long long* __restrict__ probes, int n_lists,
                                                       const int* __restrict__ row_of, long n_list_rows, int dim, int k,
                                                       int nprobe, int64_t* __restrict__ idx, float* __restrict__ dist,
                                                       const long long* __restrict__ lgrp) {
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
  if (!load_query_row(x, dim, lane, xv, qq)) {
    if (lane < k) {
      oi[lane] = -1;
      od[lane] = __builtin_nanf("");
    }
    return;
  }

  const int P = nprobe * k;
  for (int c = lane; c < P; c += 64) {
    const long long l = probes[q * nprobe + c / k];
    Cand e = Cand{__builtin_inff(), EMPTY};
    if (l >= 0 && l < n_lists) {
      const Cand got = cand[q * P + c];
      if (got.i != EMPTY && got.i >= 0 && got.i < n_list_rows) {
        const int r = row_of[got.i];
        if (r >= 0 && r < n_bank) e = Cand{got.s, r};
      }
    }
    pool[c] = e;
  }
  if (lane < MAX_K) win[lane] = EMPTY;
  __syncthreads();
  if constexpr ((GM & GM_ONE) != 0) {
    // one per group: the groups of the entries that stand (their positions are in range), then only the groups' bests
    __shared__ long long pgrp[MAX_SPLITS * MAX_K_ONE];
    for (int c = lane; c < P; c += 64) pgrp[c] = pool[c].i != EMPTY ? lgrp[cand[q * P + c].i] : 0;
    __syncthreads();
    keep_group_bests(pool, pgrp, P, lane);
  }
  // a row lies in one list: the entries are distinct, so the ranks are too
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

  int nwin = 0;
  for (int j = 0; j < k; ++j) {
    const int b = win[j];
    if (b == EMPTY) break;
    nwin = j + 1;
    const float dj = direct_distance(xv, qq, bank + (long)b * dim, dim, BTSBOT_KNN_EUCLIDEAN, lane);
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

struct IvfWs {
  size_t qimg, cand, pair_at, cnt, pstart, istart, lg, total;
  IvfWs(int64_t n_query, int dim, int k, int nprobe, int n_lists, int flags = 0) {
    const size_t pairs = (size_t)n_query * nprobe;
    const size_t bins = align256(((size_t)n_lists + 1) * sizeof(int));
    qimg = 0;
    cand = knn::image_bytes(n_query, dim);
    pair_at = cand + align256(pairs * k * sizeof(Cand));
    cnt = pair_at + align256(pairs * sizeof(int));
    pstart = cnt + bins;
    istart = pstart + bins;
    lg = istart + bins;   // GM_ONE: the groups of the list entries, int64 [k][pairs]
    total = lg + ((flags & GM_ONE) != 0 ? align256(pairs * k * sizeof(long long)) : 0);
  }
};

int check_lists(const char* who, int n_lists) {
  if (n_lists < 1 || n_lists > MAX_LISTS) {
    btsbot_set_error("%s: n_lists / n_clusters = %d must be in 1 .. %d", who, n_lists, MAX_LISTS);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

int check_probe_shape(const char* who, int64_t n_query, int dim, int k, int nprobe, int n_lists) {
  TRY(knn::check_shape(who, n_query, 0, dim, k));
  TRY(check_lists(who, n_lists));
  if (nprobe < 1 || nprobe > MAX_SPLITS || nprobe > n_lists) {
    btsbot_set_error("%s: nprobe=%d must be in 1 .. min(n_lists, %d) (n_lists=%d)", who, nprobe, MAX_SPLITS, n_lists);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query * nprobe > 0x7fffffffLL) {
    btsbot_set_error("%s: n_query * nprobe = %lld must be below 2^31", who, (long long)(n_query * nprobe));
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

// the group switches of the probed query, as knn::check_search holds them for the exact one
int check_group_flags(const char* who, int flags, int k) {
  if ((flags & ~(GM_EXCLUDE | GM_ONE)) != 0) {
    btsbot_set_error("%s: flags=%d holds bits other than BTSBOT_KNN_EXCLUDE_SAME | BTSBOT_KNN_ONE_PER_GROUP", who, flags);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if ((flags & GM_ONE) != 0 && k > MAX_K_ONE) {
    btsbot_set_error("%s: k=%d, but BTSBOT_KNN_ONE_PER_GROUP holds k <= %d (the merge keeps its pool's groups on chip)", who,
                     k, MAX_K_ONE);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return BTSBOT_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int64_t btsbot_kmeans_workspace(int64_t n_rows, int dim, int n_clusters) {
  if (knn::check_shape("btsbot_kmeans_workspace", 0, n_rows, dim, 1) != BTSBOT_OK ||
      check_lists("btsbot_kmeans_workspace", n_clusters) != BTSBOT_OK)
    return BTSBOT_ERR_INVALID_ARG;
  return (int64_t)KmeansWs(n_rows, dim, n_clusters).total;
}

extern "C" int btsbot_kmeans_update(const float* rows, int64_t n_rows, int dim, const int64_t* labels,
                                    const int64_t* order, int n_clusters, float* centroids, int64_t* counts,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "btsbot_kmeans_update";
  TRY(knn::check_shape(who, 0, n_rows, dim, 1));
  TRY(check_lists(who, n_clusters));
  const KmeansWs ws(n_rows, dim, n_clusters);
  if (centroids == nullptr || counts == nullptr || workspace == nullptr ||
      (n_rows > 0 && (rows == nullptr || labels == nullptr || order == nullptr))) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (workspace_bytes < (int64_t)ws.total || ((uintptr_t)workspace & 15) != 0) {
    btsbot_set_error("%s: workspace of %lld bytes (need %lld), or workspace not 16-byte aligned", who,
                     (long long)workspace_bytes, (long long)ws.total);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
  int* cnt = reinterpret_cast<int*>(base + ws.cnt);
  int* start = reinterpret_cast<int*>(base + ws.start);
  int* istart = reinterpret_cast<int*>(base + ws.istart);
  float* part = reinterpret_cast<float*>(base + ws.part);
  HIP_TRY(hipMemsetAsync(cnt, 0, ((size_t)n_clusters + 1) * sizeof(int), st));
  if (n_rows > 0) {
    hipLaunchKernelGGL(hist_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const long long*>(labels), (long)n_rows, n_clusters, cnt);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_T), 0, st, (const int*)cnt, n_clusters, KM_CHUNK, start, istart,
                     (long long*)nullptr);
  LAUNCH_CHECK();
  const unsigned colb = (unsigned)((dim + KM_COLS - 1) / KM_COLS);
  const unsigned items = (unsigned)(n_rows / KM_CHUNK + n_clusters);
  if (n_rows > 0) {
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3(items, colb), dim3(KM_COLS), 0, st, rows, (long)n_rows, dim,
                       reinterpret_cast<const long long*>(order), n_clusters, (const int*)cnt, (const int*)start,
                       (const int*)istart, part);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(kmeans_final_kernel, dim3((unsigned)n_clusters, colb), dim3(KM_COLS), 0, st, (const float*)part, dim,
                     n_clusters, (const int*)cnt, (const int*)istart, centroids, reinterpret_cast<long long*>(counts));
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int64_t btsbot_ivf_list_rows(int64_t n_bank, int n_lists) {
  if (knn::check_shape("btsbot_ivf_list_rows", 0, n_bank, 1, 1) != BTSBOT_OK ||
      check_lists("btsbot_ivf_list_rows", n_lists) != BTSBOT_OK)
    return BTSBOT_ERR_INVALID_ARG;
  const int64_t rows = (n_bank / TB + n_lists) * TB;
  if (rows > 0x7fffffffLL) {
    btsbot_set_error("btsbot_ivf_list_rows: the list image would hold %lld rows, at most 2^31 - 1", (long long)rows);
    return BTSBOT_ERR_INVALID_ARG;
  }
  return rows;
}

extern "C" int btsbot_ivf_layout(const void* packed, int64_t n_bank, int dim, const int64_t* labels,
                                 const int64_t* order, int n_lists, void* list_packed, int64_t n_list_rows,
                                 int32_t* row_of, int32_t* pos_of, int64_t* list_sizes, int32_t* list_tile,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "btsbot_ivf_layout";
  TRY(knn::check_shape(who, 0, n_bank, dim, 1));
  TRY(check_lists(who, n_lists));
  const int64_t need_rows = btsbot_ivf_list_rows(n_bank, n_lists);
  if (need_rows < 0) return BTSBOT_ERR_INVALID_ARG;
  if (n_list_rows != need_rows) {
    btsbot_set_error("%s: n_list_rows=%lld, btsbot_ivf_list_rows() gives %lld", who, (long long)n_list_rows,
                     (long long)need_rows);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const size_t bins = align256(((size_t)n_lists + 1) * sizeof(int));
  if (list_packed == nullptr || row_of == nullptr || list_sizes == nullptr || list_tile == nullptr ||
      workspace == nullptr || (n_bank > 0 && (packed == nullptr || labels == nullptr || order == nullptr ||
                                              pos_of == nullptr))) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (workspace_bytes < (int64_t)(2 * bins) || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)packed & 15) != 0 ||
      ((uintptr_t)list_packed & 15) != 0) {
    btsbot_set_error("%s: workspace of %lld bytes (need %lld), or workspace / packed / list_packed not 16-byte aligned",
                     who, (long long)workspace_bytes, (long long)(2 * bins));
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  int* cnt = reinterpret_cast<int*>(workspace);
  int* start = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(workspace) + bins);
  HIP_TRY(hipMemsetAsync(cnt, 0, ((size_t)n_lists + 1) * sizeof(int), st));
  HIP_TRY(hipMemsetAsync(row_of, 0xff, (size_t)n_list_rows * sizeof(int), st));   // -1: padding
  if (n_bank > 0) {
    hipLaunchKernelGGL(hist_kernel, dim3((unsigned)((n_bank + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const long long*>(labels), (long)n_bank, n_lists, cnt);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_T), 0, st, (const int*)cnt, n_lists, TB, start, list_tile,
                     reinterpret_cast<long long*>(list_sizes));
  LAUNCH_CHECK();
  if (n_bank > 0) {
    hipLaunchKernelGGL(ivf_place_kernel, dim3((unsigned)((n_bank + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const long long*>(labels), reinterpret_cast<const long long*>(order),
                       (long)n_bank, n_lists, (const int*)cnt, (const int*)start, (const int*)list_tile,
                       (long)n_list_rows, row_of, pos_of);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ivf_gather_kernel, dim3((unsigned)n_list_rows), dim3(256), 0, st,
                     reinterpret_cast<const unsigned char*>(packed), (const int*)row_of, (long)n_list_rows,
                     (int)(record_bytes(dim) / 16), reinterpret_cast<unsigned char*>(list_packed));
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int btsbot_ivf_layout_groups(const int64_t* bank_group, int64_t n_bank, int n_lists, const int32_t* row_of,
                                        int64_t n_list_rows, int64_t* list_group, void* stream) {
  const char* who = "btsbot_ivf_layout_groups";
  TRY(knn::check_shape(who, 0, n_bank, 1, 1));
  TRY(check_lists(who, n_lists));
  if (n_list_rows != btsbot_ivf_list_rows(n_bank, n_lists)) {
    btsbot_set_error("%s: n_list_rows=%lld is not btsbot_ivf_list_rows(n_bank, n_lists)", who, (long long)n_list_rows);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (row_of == nullptr || list_group == nullptr || (n_bank > 0 && bank_group == nullptr)) {
    btsbot_set_error("%s: NULL bank_group, row_of or list_group", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(ivf_gather_groups_kernel, dim3((unsigned)((n_list_rows + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, reinterpret_cast<const long long*>(bank_group), (const int*)row_of,
                     (long)n_list_rows, (long)n_bank, reinterpret_cast<long long*>(list_group));
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

extern "C" int64_t btsbot_ivf_workspace_grouped(int64_t n_query, int dim, int k, int nprobe, int n_lists, int flags) {
  const char* who = flags == 0 ? "btsbot_ivf_workspace" : "btsbot_ivf_workspace_grouped";
  if (check_probe_shape(who, n_query, dim, k, nprobe, n_lists) != BTSBOT_OK ||
      check_group_flags(who, flags, k) != BTSBOT_OK)
    return BTSBOT_ERR_INVALID_ARG;
  return (int64_t)IvfWs(n_query, dim, k, nprobe, n_lists, flags).total;
}

extern "C" int64_t btsbot_ivf_workspace(int64_t n_query, int dim, int k, int nprobe, int n_lists) {
  return btsbot_ivf_workspace_grouped(n_query, dim, k, nprobe, n_lists, 0);
}

namespace {

// what btsbot_ivf_query and btsbot_ivf_query_grouped were given, behind their checks
struct IvfQuery {
  const float* queries;
  int64_t n_query;
  const float* bank;
  int64_t n_bank;
  int dim, k;
  const long long* probes;
  int nprobe;
  const long long* self_rows;
  const unsigned char* list_packed;
  int64_t n_list_rows;
  const int *row_of, *pos_of, *list_tile;
  int n_lists;
  int64_t* idx;
  float* dist;
  unsigned char* base;
  const long long *qgrp, *lgrp;
  hipStream_t st;
};

// The launches of btsbot_ivf_query (GM = 0) and btsbot_ivf_query_grouped, one instantiation per group mode
template <int GM>
int launch_query(const IvfQuery& a) {
  const IvfWs ws(a.n_query, a.dim, a.k, a.nprobe, a.n_lists, GM);
  hipStream_t st = a.st;
  unsigned char* qimg = a.base + ws.qimg;
  Cand* cand = reinterpret_cast<Cand*>(a.base + ws.cand);
  int* pair_at = reinterpret_cast<int*>(a.base + ws.pair_at);
  int* cnt = reinterpret_cast<int*>(a.base + ws.cnt);
  int* pstart = reinterpret_cast<int*>(a.base + ws.pstart);
  int* istart = reinterpret_cast<int*>(a.base + ws.istart);
  long long* lg = reinterpret_cast<long long*>(a.base + ws.lg);
  const int k = a.k, n_lists = a.n_lists;
  const long n_pairs = (long)(a.n_query * a.nprobe);
  const long long* pr = a.probes;
  const unsigned pair_blocks = (unsigned)((n_pairs + 255) / 256);

  TRY(knn::pack_queries(a.queries, a.n_query, a.dim, qimg, st));
  HIP_TRY(hipMemsetAsync(cnt, 0, ((size_t)n_lists + 1) * sizeof(int), st));
  hipLaunchKernelGGL(hist_kernel, dim3(pair_blocks), dim3(256), 0, st, pr, n_pairs, n_lists, cnt);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_T), 0, st, (const int*)cnt, n_lists, TQ, pstart, istart,
                     (long long*)nullptr);
  LAUNCH_CHECK();
  HIP_TRY(hipMemsetAsync(cnt, 0, ((size_t)n_lists + 1) * sizeof(int), st));   // now the lists' fill cursors
  hipLaunchKernelGGL(ivf_fill_kernel, dim3(pair_blocks), dim3(256), 0, st, pr, n_pairs, n_lists, (const int*)pstart, cnt,
                     pair_at);
  LAUNCH_CHECK();
  // 64 KB of operands + 1 KB of lists per k + the tile's row map: two workgroups per CU up to k = 15, in every group mode
  const int lds_max = GEMM_LDS + TQ * MAX_K * (int)sizeof(Cand) + TQ * (int)sizeof(int);
  static DevOnce attr;
  if (attr.need()) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(ivf_select_kernel<GM>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    attr.done();
  }
  const unsigned items = (unsigned)((n_pairs + TQ - 1) / TQ + n_lists);
  hipLaunchKernelGGL(ivf_select_kernel<GM>, dim3(items), dim3(256),
                     GEMM_LDS + TQ * k * (int)sizeof(Cand) + TQ * (int)sizeof(int), st, (const unsigned char*)qimg,
                     a.list_packed, (long)a.n_list_rows, a.dim, k, a.nprobe, n_lists, (long)a.n_bank, (const int*)pstart,
                     (const int*)istart, (const int*)pair_at, a.list_tile, a.self_rows, a.pos_of, cand, a.qgrp, a.lgrp, lg,
                     n_pairs);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(ivf_merge_kernel<(GM & GM_ONE)>, dim3((unsigned)a.n_query), dim3(64), 0, st, a.queries, a.bank,
                     (long)a.n_bank, (const Cand*)cand, pr, n_lists, a.row_of, (long)a.n_list_rows, a.dim, k, a.nprobe,
                     a.idx, a.dist, a.lgrp);
  LAUNCH_CHECK();
  return BTSBOT_OK;
}

int query_checked(const char* who, const float* queries, int64_t n_query, const float* bank, int64_t n_bank, int dim, int k,
                  const int64_t* probes, int nprobe, const int64_t* self_rows, const void* list_packed,
                  int64_t n_list_rows, const int32_t* row_of, const int32_t* pos_of, const int32_t* list_tile, int n_lists,
                  int64_t* idx, float* dist, void* workspace, int64_t workspace_bytes, void* stream,
                  const int64_t* query_group, const int64_t* list_group, int flags) {
  TRY(check_probe_shape(who, n_query, dim, k, nprobe, n_lists));
  TRY(check_group_flags(who, flags, k));
  TRY(knn::check_shape(who, 0, n_bank, dim, 1));
  if (n_list_rows != btsbot_ivf_list_rows(n_bank, n_lists)) {
    btsbot_set_error("%s: n_list_rows=%lld is not btsbot_ivf_list_rows(n_bank, n_lists)", who, (long long)n_list_rows);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (n_query == 0) return BTSBOT_OK;
  if (queries == nullptr || probes == nullptr || list_packed == nullptr || row_of == nullptr || list_tile == nullptr ||
      idx == nullptr || dist == nullptr || workspace == nullptr ||
      (n_bank > 0 && (bank == nullptr || pos_of == nullptr))) {
    btsbot_set_error("%s: NULL argument", who);
    return BTSBOT_ERR_INVALID_ARG;
  }
  if (((flags & GM_EXCLUDE) != 0 && query_group == nullptr) || (flags != 0 && list_group == nullptr)) {
    btsbot_set_error("%s: flags=%d need list_group (and BTSBOT_KNN_EXCLUDE_SAME query_group), got NULL", who, flags);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const IvfWs ws(n_query, dim, k, nprobe, n_lists, flags);
  if (workspace_bytes < (int64_t)ws.total || ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)list_packed & 15) != 0) {
    btsbot_set_error("%s: workspace of %lld bytes (need %lld), or workspace / list_packed not 16-byte aligned", who,
                     (long long)workspace_bytes, (long long)ws.total);
    return BTSBOT_ERR_INVALID_ARG;
  }
  const IvfQuery a{queries, n_query, bank, n_bank, dim, k, reinterpret_cast<const long long*>(probes), nprobe,
                   reinterpret_cast<const long long*>(self_rows), reinterpret_cast<const unsigned char*>(list_packed),
                   n_list_rows, row_of, pos_of, list_tile, n_lists, idx, dist, reinterpret_cast<unsigned char*>(workspace),
                   reinterpret_cast<const long long*>(query_group), reinterpret_cast<const long long*>(list_group),
                   (hipStream_t)stream};
  switch (flags) {
    case 0: return launch_query<0>(a);
    case GM_EXCLUDE: return launch_query<GM_EXCLUDE>(a);
    case GM_ONE: return launch_query<GM_ONE>(a);
    default: return launch_query<(GM_EXCLUDE | GM_ONE)>(a);
  }
}

}  // namespace

extern "C" int btsbot_ivf_query(const float* queries, int64_t n_query, const float* bank, int64_t n_bank, int dim, int k,
                                const int64_t* probes, int nprobe, const int64_t* self_rows, const void* list_packed,
                                int64_t n_list_rows, const int32_t* row_of, const int32_t* pos_of,
                                const int32_t* list_tile, int n_lists, int64_t* idx, float* dist, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  return query_checked("btsbot_ivf_query", queries, n_query, bank, n_bank, dim, k, probes, nprobe, self_rows, list_packed,
                       n_list_rows, row_of, pos_of, list_tile, n_lists, idx, dist, workspace, workspace_bytes, stream,
                       nullptr, nullptr, 0);
}

extern "C" int btsbot_ivf_query_grouped(const float* queries, int64_t n_query, const float* bank, int64_t n_bank, int dim,
                                        int k, const int64_t* probes, int nprobe, const int64_t* self_rows,
                                        const void* list_packed, int64_t n_list_rows, const int32_t* row_of,
                                        const int32_t* pos_of, const int32_t* list_tile, int n_lists, int64_t* idx,
                                        float* dist, void* workspace, int64_t workspace_bytes, void* stream,
                                        const int64_t* query_group, const int64_t* list_group, int flags) {
  return query_checked("btsbot_ivf_query_grouped", queries, n_query, bank, n_bank, dim, k, probes, nprobe, self_rows,
                       list_packed, n_list_rows, row_of, pos_of, list_tile, n_lists, idx, dist, workspace, workspace_bytes,
                       stream, query_group, list_group, flags);
}
