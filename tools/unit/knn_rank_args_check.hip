// The host-side argument checks of btsbot_knn_rank_workspace / _count / _fill (btsbot_amd/csrc/knn_rank.hip, with the
// shared checker of knn.hip) as a stand-alone program for a run under the host sanitizers, on a machine without a GPU:
// every call below is refused, or has nothing to do, before the first HIP call.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined
//       -Xarch_host -fno-sanitize-recover=all -o tools/unit/knn_rank_args_check tools/unit/knn_rank_args_check.hip
//   tools/unit/knn_rank_args_check
//
// Prints one line per group of checks and exits 0, or names the first expectation that failed and exits 1.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../btsbot_amd/csrc/knn.hip"
#include "../../btsbot_amd/csrc/knn_rank.hip"

static char g_err[512];
void btsbot_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

static int g_failed = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, g_err); \
      g_failed = 1;                                                          \
    }                                                                        \
  } while (0)

int main() {
  const int bad = BTSBOT_ERR_INVALID_ARG;
  // an address that is never dereferenced: a call that got past its checks would be a sanitizer report
  alignas(16) static unsigned char arena[16];
  float* f = reinterpret_cast<float*>(arena);
  int64_t* i64 = reinterpret_cast<int64_t*>(arena);
  int32_t* i32 = reinterpret_cast<int32_t*>(arena);
  uint64_t* u64 = reinterpret_cast<uint64_t*>(arena);
  void* v = arena;

  EXPECT(btsbot_knn_rank_workspace(0, 5, 3) == 0);
  EXPECT(btsbot_knn_rank_workspace(3, 5, 2) == 512 + 256 + 12);
  EXPECT(btsbot_knn_rank_workspace(3, 0, 2) == bad && btsbot_knn_rank_workspace(3, 1025, 2) == bad);
  EXPECT(btsbot_knn_rank_workspace(3, 5, 0) == bad && btsbot_knn_rank_workspace(3, 5, 65) == bad);
  EXPECT(btsbot_knn_rank_workspace(-1, 5, 2) == bad && btsbot_knn_rank_workspace(int64_t(1) << 31, 5, 2) == bad);
  printf("workspace: sizes and refusals as documented\n");

  const int64_t need = btsbot_knn_rank_workspace(4, 3, 2);
  auto count = [&](const float* q, int64_t nq, const float* b, const void* pk, int64_t nb, int dim, int metric,
                   const int64_t* tg, int t, int splits, const int64_t* qg, const int64_t* bg, int flags, float* dist,
                   int32_t* rank, int32_t* counts, void* ws, int64_t wsb) {
    g_err[0] = 0;
    return btsbot_knn_rank_count(q, nq, b, pk, nb, dim, metric, tg, t, -1, splits, qg, bg, flags, dist, rank, counts, ws,
                                 wsb, nullptr);
  };
  // bad shapes
  EXPECT(count(f, 4, f, v, 9, 0, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 1025, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 0, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 65, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, -1, f, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, int64_t(1) << 31, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 3, 2, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad && strstr(g_err, "metric"));
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 0, nullptr, nullptr, 0, f, i32, i32, v, need) == bad && strstr(g_err, "splits"));
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 33, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 2, f, i32, i32, v, need) == bad && strstr(g_err, "rank modes"));
  printf("count: bad shapes, metric, splits and flags refused\n");
  // NULL arguments
  EXPECT(count(nullptr, 4, f, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad && strstr(g_err, "NULL"));
  EXPECT(count(f, 4, nullptr, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, nullptr, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 3, 0, nullptr, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, nullptr, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 1, nullptr, i64, 1, f, i32, i32, v, need) == bad && strstr(g_err, "query_group"));
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 1, i64, nullptr, 1, f, i32, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, nullptr, i32, i32, v, need) == bad && strstr(g_err, "NULL"));
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, nullptr, i32, v, need) == bad);
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, nullptr, v, need) == bad);
  // a short or misaligned workspace, a misaligned packed bank
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need - 1) == bad && strstr(g_err, "workspace"));
  EXPECT(count(f, 4, f, v, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, arena + 4, need) == bad);
  EXPECT(count(f, 4, f, arena + 8, 9, 3, 0, i64, 2, 1, nullptr, nullptr, 0, f, i32, i32, v, need) == bad);
  // nothing to do: no pointer is looked at
  EXPECT(count(nullptr, 0, nullptr, nullptr, 9, 3, 0, nullptr, 2, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0) == BTSBOT_OK);
  printf("count: NULL pointers and workspaces refused, n_query = 0 accepted\n");

  auto fill = [&](int64_t nq, int64_t nb, int t, int splits, int flags, int64_t n_band, int32_t* cand, uint64_t* mask,
                  int32_t* err, const int64_t* offsets, void* ws, int64_t wsb) {
    g_err[0] = 0;
    return btsbot_knn_rank_fill(f, nq, f, v, nb, 3, 0, i64, t, -1, splits, nullptr, nullptr, flags, f, i32, i32, offsets,
                                n_band, cand, mask, err, ws, wsb, nullptr);
  };
  EXPECT(fill(4, 9, 2, 1, 0, -1, i32, u64, i32, i64, v, need) == bad && strstr(g_err, "n_band"));
  EXPECT(fill(4, 9, 2, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, v, need) == BTSBOT_OK);    // no band pairs
  EXPECT(fill(0, 9, 2, 1, 0, 5, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == BTSBOT_OK);  // no queries
  EXPECT(fill(4, 0, 2, 1, 0, 5, nullptr, nullptr, nullptr, nullptr, v, need) == BTSBOT_OK);     // an empty bank
  EXPECT(fill(4, 9, 2, 1, 0, 5, nullptr, u64, i32, i64, v, need) == bad && strstr(g_err, "NULL"));
  EXPECT(fill(4, 9, 2, 1, 0, 5, i32, nullptr, i32, i64, v, need) == bad);
  EXPECT(fill(4, 9, 2, 1, 0, 5, i32, u64, nullptr, i64, v, need) == bad);
  EXPECT(fill(4, 9, 2, 1, 0, 5, i32, u64, i32, nullptr, v, need) == bad);
  EXPECT(fill(4, 9, 2, 1, 0, 5, i32, u64, i32, i64, v, need - 1) == bad && strstr(g_err, "workspace"));
  EXPECT(fill(4, 9, 65, 1, 0, 5, i32, u64, i32, i64, v, need) == bad);
  EXPECT(fill(4, 9, 2, 0, 0, 5, i32, u64, i32, i64, v, need) == bad);
  EXPECT(fill(4, 9, 2, 1, 2, 5, i32, u64, i32, i64, v, need) == bad);
  EXPECT(fill(4, 9, 2, 1, 1, 5, i32, u64, i32, i64, v, need) == bad && strstr(g_err, "query_group"));
  printf("fill: n_band, NULL pointers and workspaces refused, empty work accepted\n");
  printf(g_failed ? "knn_rank_args_check: FAILED\n" : "knn_rank_args_check: ok\n");
  return g_failed;
}
