// icp_ctx_internal.h — layout of the C-ABI context (private to libicp_hip.so).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/icp_hip.h"
#include "call_io.h"
#include "ctx_util.h"
#include "kernels.h"

// The prewalk (launch_prewalk): a second stream refreshes, during an iterate's statistics kernels,
// the records the next search would otherwise re-walk. Only ctx_prewalk.cpp touches these fields.
struct Prewalk {
  hipStream_t stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_done = nullptr;
  bool pending = false;    // work of the last iterate may still run on `stream` (drain_prewalk)
  double look = 0.0;       // look-ahead in iterates of the current motion (0: off)
  bool explicit_ = false;  // set by icp_hip_set_prewalk (the built-in default: large sources only)
  int4* req = nullptr;     // per-wave request records (NNLaunch::wc_req)
  double* list = nullptr;
  unsigned int* count = nullptr;
  unsigned int cap = 0;
  uint32_t stamp = 0;
};

// The search's follow-up lists as the context holds them (follow_lists.h): the counters for the
// context's lifetime, the lists for the resident source's, and what the last search published.
struct FollowBuffers {
  icp::FollowCounts* counts = nullptr;
  int32_t* ints = nullptr;    // follow_list_ints(n_src) ints: the four lists (carve_follow_lists)
  double* guesses = nullptr;  // n_src: the ball list's distance guesses
  // The counters are zero at every search's launch. An iterate's publish clears them on the device
  // once it has read them (published()), so the next search needs no memset; after anything else
  // that ran a search (nn), begin_search clears them itself.
  bool counts_zero = false;
  icp::PublishedLists last{0, 0, 0};  // of the last search (icp_iter_stats' three counts)
  double last_wide = 0.0;             // waves whose candidate set overflowed in the last published iterate

  // The counters at the first call (zeroed), and the lists of a source of n points (n < 0: none).
  hipError_t alloc(int64_t n) {
    release(false);
    hipError_t e = hipSuccess;
    if (!counts) {
      e = dalloc(&counts, 1);
      if (e == hipSuccess) e = hipMemset(counts, 0, sizeof(icp::FollowCounts));
      counts_zero = e == hipSuccess;
    }
    if (e == hipSuccess && n >= 0) e = dalloc(&ints, (size_t)icp::follow_list_ints(n));
    if (e == hipSuccess && n >= 0) e = dalloc(&guesses, (size_t)n);
    return e;
  }
  void release(bool with_counts) {
    dfree(ints);
    dfree(guesses);
    if (with_counts) dfree(counts);
  }
  hipError_t begin_search(hipStream_t s) {
    const hipError_t e = counts_zero ? hipSuccess : hipMemsetAsync(counts, 0, sizeof(icp::FollowCounts), s);
    counts_zero = false;
    return e;
  }
  void published(const icp::PublishedLists& lists, double wide) {
    counts_zero = true;
    last = lists;
    last_wide = wide;
  }
};

struct icp_hip_ctx {
  // --- configuration and lifetime (icp_ctx.hip)
  int device = 0;
  icp_hip_config cfg{};  // explicit configuration (icp_hip_create_ex); nothing from the environment
  hipStream_t stream = nullptr;

  // --- transport (ctx_comm.cpp); comm or xfn set: iterates run the all-gather + rank-order merge
  int nranks = 1, rank = 0;
  ncclComm_t comm = nullptr;
  icp_hip_exchange_fn xfn = nullptr;  // host exchange instead of RCCL (icp_hip_comm_init_host)
  void* xuser = nullptr;
  struct ExchangeWorker* xworker = nullptr;  // runs xfn when config.peer_timeout_ms > 0 (ctx_comm.cpp)
  icp::Moments* gm = nullptr;
  icp::CovMoments* gc = nullptr;
  // a member of a multi-device context: set when a peer member failed (the waits give up)
  const std::atomic<int>* abort = nullptr;
  bool comm_aborted = false;  // icp_hip_comm_abort: iterates fail until the next comm_init
  int inject_failure = 0;     // icp_hip_debug_inject_failure: 1 = fail before the first exchange

  // --- clouds (ctx_clouds.cpp): the target (replicated on every rank)
  hipEvent_t ev_it0 = nullptr, ev_it1 = nullptr;  // set_target timing
  icp::NodeRec* nodes = nullptr;
  icp::TBox* tbox = nullptr;  // tight boxes of the nodes (k_tight_boxes)
  icp::TgtPt* pts = nullptr;
  int64_t n_nodes = 0, n_leaves = 0, n_tgt = 0;
  int32_t pos0 = 0, max_depth = -1, levels = 1;
  int32_t max_inner_depth = -1;  // depth of the deepest inner node (-1: the root is a leaf)
  double init_best = 1.7976931348623157e308;
  int32_t* cells = nullptr;     // per-level cell tables of the octree (octree_gpu.h)
  int cell_lmax = -1;
  double root_box[6] = {0, 0, 0, 0, 0, 0};
  int target_on_device = 0;      // octree built on the device (octree_gpu.hip) or on the host
  double target_build_ms = 0.0;  // set_target wall time on the stream (upload + build)
  unsigned long long* counters = nullptr;  // icp_hip_traversal_counts

  // this rank's source shard, Morton order (perm[k] = caller index of slot k)
  int64_t n_src = 0;
  double *x = nullptr, *y = nullptr, *z = nullptr;
  int32_t* perm = nullptr;
  int32_t* pos = nullptr;  // leaf-order position of the match
  double* dist = nullptr;  // residual
  FollowBuffers follow;                  // the search's follow-up lists and counters
  icp::WaveBox* wc_box = nullptr;        // the wave search's candidate cache (one per wave)
  float4* wc_ents = nullptr;
  uint32_t wc_gen = 1;                   // bumped by set_target / set_source (records of older
                                         // generations are never reused)
  icp::Moments* mparts = nullptr;
  icp::CovMoments* cparts = nullptr;
  icp::WaveStat* wstat = nullptr;  // the search's per-wave covariance records (wave_stats.h)
  int64_t nb_mom = 0, nb_cull = 0;     // residual-moment parts, cull blocks
  bool have_results = false;
  bool have_prev = false;  // dist[] holds residuals of the resident queries (search guess)

  // --- iterate (ctx_iterate.cpp)
  // per-iterate timing events, a ring over the last kTimingRing iterates:
  // [0] search start (the iterate's first launch), [1] search kernel done, [2] iterate end
  static constexpr int kTimingRing = 256;
  hipEvent_t ring[kTimingRing][3] = {};
  bool timed[kTimingRing] = {};  // the slot's search carries events (config.timing_stride)
  // the record exchange of a timed multi-rank iterate: events before / after each of the two
  // all-gathers (RCCL; created at first use), or the host clock around them (host exchange)
  hipEvent_t xring[kTimingRing][4] = {};
  int8_t xtimed[kTimingRing] = {};  // 0 not timed, 1 events (RCCL), 2 host clock
  double xhost_ms[kTimingRing] = {};
  int64_t n_iterates = 0;
  unsigned int* tickets = nullptr;  // "last block done" counters of the moments and cull launches
                                    // (zero between launches: the last block resets its own)
  unsigned long long* dbg = nullptr;
  int last_cull_path = -1;         // IterDev::cull_mode of the last host-published iterate
  // per-iteration record
  icp::IterDev* it = nullptr;
  icp::IterDev* h_it = nullptr;      // pinned, coherent: the publishing kernel stores into it
  icp::IterDev* h_it_dev = nullptr;  // its device address
  uint64_t publish_seq = 0;          // h_it->seq = this once the record is complete
  // the device-resident loop (icp_hip_loop_run): the session state on the device, its pinned
  // staging copy, and one LoopRec per iteration of a batch (pinned, written by the last kernel)
  static constexpr int kLoopRing = kTimingRing;
  icp::LoopDev* loopd = nullptr;
  icp::LoopDev* h_loop = nullptr;
  icp::LoopRec* h_ring = nullptr;
  icp::LoopRec* h_ring_dev = nullptr;
  hipEvent_t ev_batch = nullptr;  // a batch's start (its first iteration's step time)

  // --- prewalk (ctx_prewalk.cpp)
  Prewalk pw;

  // --- LAS records decoded / encoded on the device (ctx_las.cpp): staging buffers, made at first use
  struct LasIo* las = nullptr;
  int las_device_path = -1;      // icp_hip_last_las_path: 1 kernels, 0 host reader / writer, -1 none yet
  size_t las_chunk_bytes = 8u << 20;  // icp_hip_set_las_chunk_bytes

  // --- point-to-plane (ctx_plane.cpp): the target's normals (leaf order, 3 x fp64; null: none) and
  // the part sums of icp_hip_plane_sums (made at first use, released with the target)
  double* normals = nullptr;
  double* plane_parts = nullptr;  // plane_cap parts + the merged sums (kPlaneSums doubles each)
  int64_t plane_cap = 0;

  // --- generalized ICP (ctx_gicp.cpp): the source's normals (slot order, 3 x fp64; null: none; released
  // with the source), in the frame the source had when they were made; the part sums of
  // icp_hip_gicp_sums (made at first use, released with the context); the sessions' epsilon.
  // src_moves counts the transforms applied to the resident source (host bookkeeping only: the
  // iterate's fused T_apply, icp_hip_apply, a device-loop batch), src_normals_moves its value when
  // the normals were made.
  double* src_normals = nullptr;
  double* gicp_parts = nullptr;  // gicp_cap parts + the merged sums (kGicpSums doubles each)
  int64_t gicp_cap = 0;
  double gicp_epsilon = 1e-3;
  uint64_t src_moves = 0, src_normals_moves = 0;

  // --- rejectors (ctx_reject.cpp): the select's histograms and states, and the pair sums' parts
  // (made at first use, released with the context)
  void* select_buf = nullptr;
  double* pair_parts = nullptr;  // pair_cap parts, then the merged record and the first-pair word
  int64_t pair_cap = 0;

  // --- voxel-grid down-sampling (ctx_voxel.cpp): the phases' device times of the last call
  double voxel_ms[5] = {0, 0, 0, 0, 0};
  bool voxel_timed = false;

  // --- outlier removal (ctx_outlier.cpp): the phases' device times of the last call
  double outlier_ms[4] = {0, 0, 0, 0};
  bool outlier_timed = false;

  // --- multi-device context (icp_hip_create_multi): the member contexts and their driver threads
  // (icp_group.cpp); the single-device fields above are then unused
  struct DeviceGroup* group = nullptr;
};

// --- ctx_clouds.cpp
void free_target(icp_hip_ctx* c);
void free_source(icp_hip_ctx* c);
// The search launch over the resident target with this context's configuration; the caller
// fills the query arrays and the lists.
icp::NNLaunch base_launch(const icp_hip_ctx* c);
// The argument check of the device-pointer entry points: ICP_HIP_EINVAL (with a message naming
// `what`) unless p is non-null, aligned, and device memory of the context's device or managed
// memory by hipPointerGetAttributes. Never dereferences p.
int check_device_ptr(const icp_hip_ctx* c, const void* p, const char* what, unsigned align = 8);
// The same for an optional output: a null pointer is fine.
int check_optional_device_ptr(const icp_hip_ctx* c, const void* p, const char* what, unsigned align = 8);
// gpu_build_octree's return code (octree_gpu.h) and text as the C ABI's error.
int fail_octree_build(int rc, const std::string& why);

// The host-staged routes of the device variants: the caller's buffer through host memory, complete
// at return. A group's buffer may be any device's, so it is copied without the member's stream.
template <typename T>
hipError_t stage_down(const icp_hip_ctx* c, std::vector<T>* h, const T* d, size_t count) {
  h->resize(count);
  if (count == 0) return hipSuccess;
  if (c->group) return hipMemcpy(h->data(), d, count * sizeof(T), hipMemcpyDeviceToHost);
  hipError_t e = hipMemcpyAsync(h->data(), d, count * sizeof(T), hipMemcpyDeviceToHost, c->stream);
  return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

template <typename T>
hipError_t stage_up(const icp_hip_ctx* c, T* d, const std::vector<T>& h) {
  if (h.empty()) return hipSuccess;
  if (c->group) return hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  hipError_t e = hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c->stream);
  return e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
}

// A group's relay of one optional device output: the host vector that the first
// member's host call fills, then staged up to the caller's buffer. Nothing when d is null.
template <typename T>
class RelayOut {
 public:
  explicit RelayOut(T* d, size_t count = 0) : d_(d), v_(d ? count : 0) {}
  void resize(size_t count) { v_.resize(d_ ? count : 0); }
  T* host() { return v_.empty() ? nullptr : v_.data(); }
  hipError_t up(const icp_hip_ctx* c) const { return stage_up(c, d_, v_); }

 private:
  T* d_;
  std::vector<T> v_;
};

// The relay's last step: every output staged up, stopping at the first failure.
template <class... Outs>
int relay_up(const icp_hip_ctx* c, const Outs&... outs) {
  hipError_t e = hipSuccess;
  ((e = e == hipSuccess ? outs.up(c) : e), ...);
  return e == hipSuccess ? ICP_HIP_OK : fail_hip("stage_up", e);
}

// The text of a compacting call's "m entries do not fit the capacity" error.
using CapText = std::string (*)(int64_t m, int64_t cap);

// A compacting call once m is known: the caller gets it even when the kept outputs (any_kept: one
// is asked for) then prove too small for it.
inline int report_m(int64_t m, int64_t cap, bool any_kept, CapText cap_text, int64_t* m_out) {
  *m_out = m;
  return any_kept && m > cap ? fail(ICP_HIP_EINVAL, cap_text(m, cap)) : ICP_HIP_OK;
}

// A *_last_timing getter's body: the count phase times of the last call, or ICP_HIP_ENOTREADY with
// none_text when none has run.
int last_timing(bool timed, const double* src, int count, const char* none_text, double* ms);

// A group's relay of a compacting call, whose outputs' size m is known only from the call itself:
// call(false, 0, &m) is the member's host call with capacity 0 and no kept output (it counts, and
// fetches what does not depend on m); call(true, m, &m) the one that fills kept outputs of m
// entries, made only when one is asked for (any_kept) and m fits the caller's capacity. *m_out is
// set even when the call then fails. The caller stages the outputs up (relay_up) after ICP_HIP_OK.
template <class Call>
int relay_count_then_fill(bool any_kept, int64_t cap, CapText cap_text, int64_t* m_out, Call call) {
  int64_t m = 0;
  const int rc = call(false, (int64_t)0, &m);
  *m_out = m;
  if (rc != ICP_HIP_OK || !any_kept) return rc;
  if (const int rc2 = report_m(m, cap, true, cap_text, m_out)) return rc2;
  return call(true, m, &m);
}

// --- ctx_prewalk.cpp
// The prewalk's one safety rule: whatever frees, regenerates or reads the record buffers (wc_box,
// wc_ents, the request records) or the debug counters calls this first: a prewalk of the last iterate
// may still be writing them on the side stream, which synchronising the main stream does not cover.
void drain_prewalk(icp_hip_ctx* c);
void prewalk_init(icp_hip_ctx* c);         // a new context: the build's default look-ahead
void prewalk_warm(icp_hip_ctx* w);         // the warm-up's context: on where the build switches it on
void prewalk_new_source(icp_hip_ctx* c);   // set_source, after the candidate cache: the request records
void prewalk_free_source(icp_hip_ctx* c);  // drained; the per-source buffers released
void prewalk_destroy(icp_hip_ctx* c);      // the side stream synchronised; all of it released
int prewalk_synchronize(icp_hip_ctx* c);   // icp_hip_synchronize's part: the side stream idle
// An iterate's three calls (enqueue_iterate). The join, before the search is enqueued on s: the
// last iterate's prewalk writes the records this search reads (and the debug counters it clears).
int prewalk_join(icp_hip_ctx* c, hipStream_t s);
// Whether this iterate prewalks, and if so the launch record's fields for it (wc_req, wc_stamp,
// ev_fork, the list); nothing else decides it. Only after a search that reuses and stores records (a
// transform applied, previous residuals), and never in the device loop: its session step
// overwrites the transform (LoopDev::core.T) that the prewalk's lead reads while it would run.
bool prewalk_arm(icp_hip_ctx* c, icp::NNLaunch& a, const icp::LoopDev* loop, bool apply);
int prewalk_launch(icp_hip_ctx* c, const icp::NNLaunch& a);  // after launch_nn of an armed iterate

// --- ctx_plane.cpp
void plane_free_target(icp_hip_ctx* c);  // free_target's part: the normals and the plane sums' buffers

// --- ctx_gicp.cpp
void gicp_free_source(icp_hip_ctx* c);  // free_source's part: the source's normals
void gicp_destroy(icp_hip_ctx* c);      // the sums' buffers released (icp_hip_destroy)

// --- ctx_reject.cpp
void reject_destroy(icp_hip_ctx* c);  // the rejectors' buffers released (icp_hip_destroy)

// --- ctx_las.cpp
void las_destroy(icp_hip_ctx* c);  // the staging buffers released (icp_hip_destroy)

// --- ctx_iterate.cpp
// The device-resident loop: k iterations (k <= kLoopRing) enqueued back to back, each one's last
// kernel stepping the session on the device (session_step.h), one host wait per batch. core is
// the session state (uploaded, then updated), recs gets the k iterations' records (outcome
// kStepNone once the session finished), step_ms (optional) each iteration's device time.
// Eligible: a single-device context (RCCL communicator or none; not the host exchange) with
// config.device_loop set.
bool icp_hip_loop_eligible(const icp_hip_ctx* c);
int icp_hip_loop_run(icp_hip_ctx* c, icp::SessionCore* core, const icp::SessionParams* p, int rules, double sigma,
                     int k, icp::LoopRec* recs, double* step_ms);

// --- ctx_comm.cpp
// The per-iteration all-gather of one record (count doubles) in rank order: RCCL on the compute
// stream, or the caller's host exchange (stream synchronised around the callback).
int all_gather_record(icp_hip_ctx* c, const double* d_local, double* d_gathered, int count, hipStream_t s);
// Attach a communicator created elsewhere (ncclCommInitAll of a multi-device context); the
// context owns it from then on.
int icp_ctx_attach_comm(icp_hip_ctx* c, ncclComm_t comm, int nranks, int rank);
// ncclCommAbort of the context's communicator (icp_hip_comm_abort without the argument checks)
void icp_ctx_abort_comm(icp_hip_ctx* c);
// Back to a world of one without a transport: the communicator destroyed, the exchange thread
// joined (after its callback returns), comm_aborted cleared.
void icp_ctx_drop_transport(icp_hip_ctx* c);

// --- icp_group.cpp, the multi-device context: every C-ABI entry point of the context's units
// dispatches here when ctx->group is set.
void group_destroy(icp_hip_ctx* c);
int group_set_target(icp_hip_ctx* c, const double* xyz, int64_t n, int max_points, int max_depth, int rules);
int group_target_build_info(icp_hip_ctx* c, int32_t* on_device, double* build_ms);
int group_set_source(icp_hip_ctx* c, const double* xyz, int64_t n);
int group_iterate(icp_hip_ctx* c, const double* T_apply, int iter, int rules, double sigma, icp_iter_stats* out);
int group_apply(icp_hip_ctx* c, const double* T);
int group_copy_query_order(icp_hip_ctx* c, int32_t* perm_out);
int group_get_source(icp_hip_ctx* c, double* xyz_out);
int group_get_correspondences(icp_hip_ctx* c, int32_t* idx_out, double* dist_out);
int group_traversal_counts(icp_hip_ctx* c, double* mean_entries, double* mean_points);
int group_cull_path(icp_hip_ctx* c, int32_t* fused);
int group_timings(icp_hip_ctx* c, int k, double* nn_ms, double* it_ms);
int group_debug_counters(icp_hip_ctx* c, uint64_t out[ICP_DBG_SLOTS]);
int group_exchange_timings(icp_hip_ctx* c, int k, double* ms);
int group_comm_info(icp_hip_ctx* c, int member, int32_t* count, int32_t* rank, int32_t* device, int32_t* transport);
int group_synchronize(icp_hip_ctx* c);
int group_set_prewalk(icp_hip_ctx* c, double look_ahead);
int group_inject_failure(icp_hip_ctx* c, int member, int where);
icp_hip_ctx* group_member(icp_hip_ctx* c, int k);
int64_t group_n_src(icp_hip_ctx* c);  // points of the last set_source, all members
