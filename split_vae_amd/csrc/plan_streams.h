// The step plan's side streams and every event that orders them against the caller's stream (lgvae_plan.hip holds one SideStreams by value).
//
// Weight gradients on a second stream (they feed only Adam / the all-reduce; the input-gradient chain is the critical path): fork = the side stream waits
// for the event recorded on the main stream when dY is ready, join before Adam and at the end of every sv_lgvae_step call.
// The struct does not know the plan: begin_call() takes what a call's launches depend on, once per call.
// ONE includer (lgvae_plan.hip): the test hook's kernel and the struct live in an anonymous namespace, a second translation unit would get its own copies.
#pragma once
#include <string.h>
#include "common.hip.h"
#include "kernels.h"

namespace {

// test hook only (sv_lgvae_plan_debug "side_delay_us"): holds a stream back for a while
__global__ void sv_plan_spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
static void sv_plan_spin(hipStream_t st, int us) { hipLaunchKernelGGL(sv_plan_spin_kernel, dim3(1), dim3(64), 0, st, (long long)us * 100); }   // wall_clock64: 100 MHz

struct SideStreams {
  enum { SIDE_MAX = 4 };
  hipStream_t side[SIDE_MAX] = {nullptr, nullptr, nullptr, nullptr};   // SV_SIDE_STREAMS of them, taken round-robin: the weight
  hipEvent_t ev_fork = nullptr, ev_join[SIDE_MAX] = {nullptr, nullptr, nullptr, nullptr};   // gradients of different layers are independent
  int use = 1;             // streams the current call hands layers to (begin_call)
  int count = 0;           // layers forked since the last join
  int nside = 0, next = 0, slot = 0;   // slot: which stream (and which slab workspace) the last wgrad_stream() gave out
  bool pending = false;
  bool serial = false, capture = false;   // this call's launches must be serial / are captured or replayable (begin_call)
  // EARLY SIDE WORK (round 6): what the step's first launches do not need runs on side stream 0 beside them -- the decoders' weight images (the encoders' forward
  // reads only its own) and the zero fill of the gradient buffer (first written by the backward).  Both are HBM-bound, the encoder convs beside them matrix-bound;
  // batch-independent time off the critical path of every shard size.  ev_early is waited for before the decoders' forward / the backward / the end of the call.
  hipEvent_t ev_early = nullptr, ev_early_now = nullptr;
  bool early_pending = false;
  // fork / join events: one per use while graph replay is on (a captured event node per dependency), the two fixed ones otherwise
  enum { CAP_EV = 96 };
  hipEvent_t ev_cap[CAP_EV] = {};
  int n_cap = 0;
  bool side_used[SIDE_MAX] = {false, false, false, false};
  // per-plan test hooks (sv_lgvae_plan_debug): never read from the environment, so nothing a job inherits can switch them on
  int dbg_side_delay_us = 0;
  bool dbg_bucket_skip_side = false;
  // gradient-bucket events (SV_PHASE_BUCKET_EVENTS): [bucket][0 = compute stream, 1 + i = side stream i]
  hipEvent_t ev_bucket[3][1 + SIDE_MAX] = {};
  bool bucket_rec[3][1 + SIDE_MAX] = {};

  // One sv_lgvae_step call begins: its fork / join events and the side streams it uses.  serial: the full per-kernel profile table wants serial launches;
  // capture: the call is being captured into a graph, or may be (graph replay is on); whole_step: every phase in one call; images: images per twin launch.
  void begin_call(bool serial_, bool capture_, bool whole_step, int images) {
    serial = serial_;
    capture = capture_;
    n_cap = 0;
    for (auto& u : side_used) u = false;
    // Two weight-gradient side streams for a whole step at >= 768 images per launch, one otherwise.  Re-measured in round 3 (round 2: +-0):
    // B = 512 2.056 -> 2.005 ms (three launches in flight fill the CUs the rolling-window d4 kernel and the row-ring input gradients leave);
    // B = 256 +1.8 %, 128 +6 %, 64 +3 % (launches too small to share the chip three ways); a data-parallel step (phase-split calls: the
    // communication stream is a further active queue) 2.14 -> 2.15 ms over torch's nccl, 2.12 -> 3.31 ms over sv_comm (four active streams
    // on GPU_MAX_HW_QUEUES = 3): one.  SV_SIDE_STREAMS forces a count.
    const int forced = sv_knob_side_streams(0);
    // fp32 (round 5, polyphase decoder layers + 52-KB weight-gradient tiles): two side streams 9.60-9.62 -> 9.37-9.39 ms at B = 512 (profiles/r05_f32_streams.txt)
    // (fp32, 256 images per network: 5.14 -> 5.09 ms; 128: 2.84 -> 2.87: from 256)
    // (round 6, with the process's fixed side streams: bf16 256 images per network 1.068-1.080 -> 1.054-1.056 ms with two: the bf16 threshold moved from 768 to 512 too;
    //  profiles/r06_sweep_bf16.txt)
    use = forced > 0 ? forced : (whole_step && images >= 512) ? 2 : 1;
  }
  // captured steps: SV_GRAPH_SIDE=1 lets the capture fork to the side streams too (every fork / join on its OWN event and only the streams a call really used are
  // joined: round 3's capture, which re-recorded one fork event and joined every stream, replayed wrongly on ROCm 7.2).  Off by default: see DESIGN.md section 7.
  static bool graph_side() { return sv_knob_graph_side(); }
  bool side_allowed() const {
    static const bool off = SV_TUNE_FLAG("SV_NO_SIDE");
    return !(off || serial || (capture && !graph_side()));
  }
  hipEvent_t* fresh_event(hipEvent_t* fixed) { return capture && n_cap < CAP_EV ? &ev_cap[n_cap++] : fixed; }   // (created where it is first recorded)
  hipStream_t early_stream(hipStream_t st) {          // side stream 0, ordered behind everything `st` holds now; nullptr: no side streams (serial modes)
    // OPT-IN (SV_EARLY_SIDE=1).  Measured (profiles/r06_ab.txt): the step is no shorter for it at any shard size -- fp32 512 images 9.152 against 9.138 ms without,
    // 64 images 1.690 / 1.689, bf16 512 images 1.661 / 1.646: the encoders' first layers are HBM-bound themselves (e1 reads the whole batch), the weight images' 165 MB
    // beside them slow them by what the overlap saves (fwd.e1 25 -> 52 us at 64 images).  Same finding as round 3's early optimizer tail: no idle resource to hide it in.
    const bool on = sv_knob_early_side();
    if (!on || !side_allowed() || !ensure_side()) return nullptr;
    if (!sv_event_handoff(fresh_event(&ev_fork), st, side[0])) return nullptr;
    side_used[0] = true;
    return side[0];
  }
  int early_done(hipStream_t side0) {                 // the early work is enqueued: mark it
    hipEvent_t* e = fresh_event(&ev_early);
    if (!sv_event_record(e, side0)) return (int)hipGetLastError();
    ev_early_now = *e;
    early_pending = true;
    return SV_OK;
  }
  int early_wait(hipStream_t st) {
    if (!early_pending) return SV_OK;
    early_pending = false;
    return hipStreamWaitEvent(st, ev_early_now, 0) == hipSuccess ? SV_OK : (int)hipGetLastError();
  }
  bool ensure_side() {
    if (nside) return true;
    // (priority: streams.hip creates the shared streams at the lowest priority; SV_SIDE_PRIO_NORMAL is read there)
    const int want = sv_knob_side_streams(2);      // taken; `use` of them are used per call
    const int k = want < 1 ? 1 : want > SIDE_MAX - 1 ? SIDE_MAX - 1 : want;   // the last workspace slot belongs to the main stream
    for (int i = 0; i < k && i < SV_SHARED_STREAMS; ++i) {
      side[i] = sv_shared_stream(i);               // the process's shared side streams (streams.hip): never a stream per plan
      if (!side[i]) break;
      ++nside;
    }
    return nside > 0;
  }
  hipStream_t wgrad_stream(hipStream_t st) {
    slot = 0;
    if (!side_allowed()) return st;     // the full per-kernel table wants serial launches; a captured fork/join replayed wrongly on ROCm 7.2 (corrupt gradients, then a crash): captures stay single-stream
    if (!ensure_side()) return st;
    const int n = use < nside ? use : nside;
    static const char* order = SV_TUNE_STR("SV_SIDE_ORDER", nullptr);        // experiment: stream per forked layer in launch order, e.g. "0110" (repeats)
    int s = next % n;
    if (order && order[0]) { const int c = order[count % (int)strlen(order)] - '0'; if (c >= 0 && c < n) s = c; }
    ++count;
    if (!sv_event_handoff(fresh_event(&ev_fork), st, side[s])) return st;
    side_used[s] = true;
    // test hook (sv_lgvae_plan_debug "side_delay_us", tests/test_gpu_dist.py): hold the side stream back at its first use of a step, so that a consumer
    // of the gradients that does not wait for the side stream's part (a missing bucket dependency) reads them before they exist
    if (dbg_side_delay_us > 0 && count == 1) sv_plan_spin(side[s], dbg_side_delay_us);
    next = s + 1;
    slot = s;
    pending = true;
    return side[s];
  }
  int join_side(hipStream_t st) {
    if (!pending && !(capture && side_used[0])) return SV_OK;         // (a captured call joins the early work's stream too: every forked stream must rejoin the capture)
    pending = false;
    next = 0;                          // every step hands the layers to the same streams
    count = 0;
    for (int i = 0; i < nside; ++i) {
      if (capture && !side_used[i]) continue;                          // (an event of a stream outside the capture must not be waited for inside it)
      if (!sv_event_handoff(fresh_event(&ev_join[i]), side[i], st)) return (int)hipGetLastError();
    }
    return SV_OK;
  }
  void clear_buckets() {
    for (auto& row : bucket_rec)
      for (auto& b : row) b = false;
  }
  int record_bucket(int k, hipStream_t st) {
    for (int i = 0; i <= SIDE_MAX; ++i) bucket_rec[k][i] = false;
    for (int i = 0; i <= nside; ++i) {                    // every stream that may hold work of this bucket, in its own order
      hipStream_t s = i == 0 ? st : side[i - 1];
      if (i > 0 && !s) continue;
      if (!sv_event_record(&ev_bucket[k][i], s)) return (int)hipGetLastError();
      bucket_rec[k][i] = true;
    }
    return SV_OK;
  }
  // sv_lgvae_bucket_wait: `st` waits for bucket 0 .. 2, or 3 = 1 and 2; SV_E_STATE: no such events were recorded
  int bucket_wait(int bucket, hipStream_t st) const {
    int n = 0;
    for (int k = (bucket == 3 ? 1 : bucket); k <= (bucket == 3 ? 2 : bucket); ++k)
      for (int i = 0; i <= SIDE_MAX; ++i)
        if (bucket_rec[k][i]) {
          // test hook (negative control of tests/test_gpu_dist.py::test_buckets_wait_for_the_side_stream): drop the side streams' events
          if (dbg_bucket_skip_side && i > 0) continue;
          if (hipStreamWaitEvent(st, ev_bucket[k][i], 0) != hipSuccess) return (int)hipGetLastError();
          ++n;
        }
    return n ? SV_OK : SV_E_STATE;
  }
  // per-plan test hooks: "side_delay_us" (hold the first side-stream launch of every step back by that long), "bucket_skip_side" (sv_lgvae_bucket_wait
  // drops the side streams' events: the negative control of the bucket-dependency test).  Deliberately an explicit call on one plan, not an environment
  // variable: nothing a training job inherits can switch them on.
  int debug(const char* key, int64_t value) {
    if (!strcmp(key, "side_delay_us")) { if (value < 0 || value > 1000000) return SV_E_BADARG; dbg_side_delay_us = (int)value; return SV_OK; }
    if (!strcmp(key, "bucket_skip_side")) { dbg_bucket_skip_side = value != 0; return SV_OK; }
    return SV_E_BADARG;
  }
  void destroy() {                     // the events are this object's; the streams are shared with every other plan / tape of the process: not destroyed
    for (int i = 0; i < nside; ++i) (void)hipStreamSynchronize(side[i]);
    auto drop = [](hipEvent_t e) { if (e) (void)hipEventDestroy(e); };
    drop(ev_fork); drop(ev_early);
    for (auto e : ev_join) drop(e);
    for (auto e : ev_cap) drop(e);
    for (auto& row : ev_bucket)
      for (auto e : row) drop(e);
  }
};

}  // namespace
