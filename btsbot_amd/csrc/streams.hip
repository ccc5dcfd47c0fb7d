// Streams the library creates itself: the placement probe (pick_apart_stream) and the training step's side stream with
// its fork / join (ctx.h).
#include <chrono>

#include "ctx.h"

// The backward's second stream must be served by a DIFFERENT hardware pipe than the caller's stream.  A compute pipe
// works on one of its hardware queues at a time and changes queue when that one runs dry or after a time quantum; which
// pipe a new stream's queue gets depends on how many queues the process already has.  When both streams of the backward
// land on one pipe their kernels are dispatched in turns of ~50 us instead of side by side: measured 4.9-7.0 ms per
// 1024-alert step against 2.75 ms, in every process that had used exactly THREE other streams before the first
// btsbot_backward() (bench.py's scoring loop; tools/host_streams_probe2.py: two or four are fine; stream priorities and
// GPU_MAX_HW_QUEUES do not move it).  The placement cannot be asked, so it is measured, RELATIVE to a baseline taken in
// the same call: the host times an empty kernel on the candidate (launch -> event synchronise) first with the busy
// streams idle, then while a train of short spinning kernels keeps each of them busy; the minimum over the trials of
// each (host noise and a profiler's per-launch cost only ever add, and they add to both) differs by a few microseconds
// when the candidate runs beside the trains and by a quantum (30-40 us) when it shares a pipe with one of them.
// Up to eight candidates.  The choice is kept per caller stream (ctx.h: side_cache); when no candidate runs apart the
// last one is kept anyway and the handle says so: once on stderr, in btsbot_last_error() and through
// btsbot_set_option(h, "query_side_apart", 0) (returns 1 / 0 as BTSBOT_OK / BTSBOT_ERR_STATE).
__global__ void spin_kernel(unsigned long long ticks) {   // s_memrealtime counts at 100 MHz
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
__global__ void empty_kernel() {}

namespace {
constexpr double SAME_PIPE_EXTRA_US = 20.0;   // beside: +0 .. 9 us over the idle baseline; same pipe: +30 .. 40
constexpr int PLACEMENT_TRIALS = 4;

struct StreamPile {   // candidates that were not taken (and the event) are released on every path out
  hipStream_t s[8];
  int n = 0;
  hipEvent_t ev = nullptr;
  ~StreamPile() {
    for (int i = 0; i < n; ++i) (void)hipStreamDestroy(s[i]);
    if (ev != nullptr) (void)hipEventDestroy(ev);
  }
};

// microseconds from the launch of an empty kernel on `cand` to the host seeing it done (minimum of the trials), with a
// train of spinning kernels on each of busy[0..nbusy) when `loaded`
int time_candidate(hipStream_t cand, hipEvent_t ev, const hipStream_t* busy, int nbusy, bool loaded, double* best_us) {
  double best = 1e30;
  for (int trial = 0; trial < PLACEMENT_TRIALS; ++trial) {
    for (int b = 0; b < nbusy; ++b) HIP_TRY(hipStreamSynchronize(busy[b]));
    if (loaded)
      for (int i = 0; i < 24; ++i)          // 24 x 25 us per busy stream, interleaved so that every train has started
        for (int b = 0; b < nbusy; ++b) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, busy[b], 2500ULL);
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, cand);
    HIP_TRY(hipEventRecord(ev, cand));
    HIP_TRY(hipEventSynchronize(ev));
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    best = us < best ? us : best;
  }
  for (int b = 0; b < nbusy; ++b) HIP_TRY(hipStreamSynchronize(busy[b]));
  *best_us = best;
  return BTSBOT_OK;
}
}  // namespace

// a new non-blocking stream whose hardware queue is served by another pipe than every stream in busy[]
int pick_apart_stream(btsbot_ctx* h, const hipStream_t* busy, int nbusy, const char* role, hipStream_t* out, bool* apart_out) {
  StreamPile pile;
  HIP_TRY(hipEventCreateWithFlags(&pile.ev, hipEventDisableTiming));
  const bool debug = switch_set(SW_DEBUG_SIDE);
  hipStream_t chosen = nullptr;
  bool apart = false;
  for (int attempt = 0; attempt < 8 && chosen == nullptr; ++attempt) {
    hipStream_t cand = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&cand, hipStreamNonBlocking));
    pile.s[pile.n++] = cand;
    hipLaunchKernelGGL(empty_kernel, dim3(1), dim3(64), 0, cand);   // (first use of the stream: its queue exists now)
    HIP_TRY(hipStreamSynchronize(cand));
    double idle = 0.0, loaded = 0.0;
    TRY(time_candidate(cand, pile.ev, busy, nbusy, false, &idle));
    TRY(time_candidate(cand, pile.ev, busy, nbusy, true, &loaded));
    apart = loaded - idle < SAME_PIPE_EXTRA_US;
    if (debug)
      fprintf(stderr, "btsbot: %s-stream candidate %d: its kernel returns in %.1f us with the %d busy stream(s) idle, %.1f us "
                      "beside their spinning kernels -> %s\n", role, attempt, idle, nbusy, loaded,
              apart ? "taken" : "shares a pipe, rejected");
    if (apart) {
      chosen = cand;
      --pile.n;   // (the newest entry: leaves the pile)
    }
  }
  if (chosen == nullptr) {   // no candidate ran beside the busy streams: keep the last one, and say so
    chosen = pile.s[--pile.n];
    btsbot_set_error("warning: no %s stream on a hardware pipe of its own was found in 8 candidates; its kernels will take turns "
                     "with the caller's (expect slower training steps)", role);
    static bool told = false;
    if (!told) {
      told = true;
      fprintf(stderr, "btsbot_amd: %s\n", btsbot_last_error());
    }
  }
  *out = chosen;
  *apart_out = apart;
  (void)h;
  return BTSBOT_OK;
}

int create_side_stream(btsbot_ctx* h, hipStream_t caller) {
  // one choice per caller stream: a caller that alternates streams gets the stream picked for each back, no new probe
  for (const SidePick& p : h->side_cache)
    if (p.caller == caller) {
      h->side = p.side;
      h->side_for = caller;
      h->side_apart = p.apart;
      return BTSBOT_OK;
    }
  hipStream_t chosen = nullptr;
  bool apart = false;
  TRY(pick_apart_stream(h, &caller, 1, "side", &chosen, &apart));
  h->side_cache.push_back(SidePick{caller, chosen, apart});
  h->side = chosen;
  h->side_for = caller;
  h->side_apart = apart;
  return BTSBOT_OK;
}

static int side_event(btsbot_ctx* h, hipEvent_t* e) {
  if (h->side_used == h->side_ev.size()) {
    hipEvent_t fresh;
    HIP_TRY(hipEventCreateWithFlags(&fresh, hipEventDisableTiming));
    h->side_ev.push_back(fresh);
  }
  *e = h->side_ev[h->side_used++];
  return BTSBOT_OK;
}

int side_fork(btsbot_ctx* h, hipStream_t st, hipStream_t* sd) {
  *sd = st;
  if (!h->sched.side_stream || h->side == nullptr) return BTSBOT_OK;
  hipEvent_t e;
  TRY(side_event(h, &e));
  HIP_TRY(hipEventRecord(e, st));
  HIP_TRY(hipStreamWaitEvent(h->side, e, 0));
  *sd = h->side;
  return BTSBOT_OK;
}

int side_join(btsbot_ctx* h, hipStream_t st) {
  if (!h->sched.side_stream || h->side == nullptr) return BTSBOT_OK;
  hipEvent_t e;
  TRY(side_event(h, &e));
  HIP_TRY(hipEventRecord(e, h->side));
  HIP_TRY(hipStreamWaitEvent(st, e, 0));
  h->meta_join_pending = false;
  return BTSBOT_OK;
}
