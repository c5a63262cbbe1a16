// ctx_iterate.cpp — one iterate enqueued on the context's stream in named steps, the host-driven
// iterate and the device-resident loop around it, their one host wait, and the timing rings.
#include <chrono>
#include <cmath>
#include <cstring>

#include "icp_ctx_internal.h"

using namespace icp;

// The host's wait for the device (the only wait of an iterate or of a device-loop batch): `done`
// polled in a tight loop; every 1024 polls the group's abort flag, the stream's own errors and,
// over an RCCL communicator, the communicator's asynchronous error and config.peer_timeout_ms. A
// peer process that died or a broken link leaves this rank's ncclAllGather waiting forever on the
// device: RCCL reports it as the communicator's async error, and the deadline covers what it does
// not see. Either way the communicator is aborted (the pending collective returns, the stream
// drains) and iterates fail with ERCCL until comm_init. The deadline is per iterate: `progress`
// (a count of the iterates the device has finished, e.g. a device-loop batch's published ring
// records) restarts it, so a long batch of healthy iterates is not a stalled peer. (The host
// exchange needs no deadline here: its callback ran, under its own deadline, before this wait,
// which then covers device work only.)
template <class Done, class Progress>
static int wait_device(icp_hip_ctx* c, Done done, Progress progress, const char* what) {
  hipStream_t s = c->stream;
  const bool peers = c->comm != nullptr;
  auto t0 = std::chrono::steady_clock::now();
  uint64_t seen = progress();
  for (unsigned spin = 1; !done(); spin++) {
    if ((spin & 1023u) != 0) continue;
    const uint64_t now_p = progress();
    if (now_p != seen) {  // the device finished an iterate: the deadline starts again
      seen = now_p;
      t0 = std::chrono::steady_clock::now();
    }
    if (c->abort && c->abort->load()) return fail(ICP_HIP_EEXCHANGE, std::string(what) + ": a peer device of the group failed");
    if (c->comm) {
      ncclResult_t ae = ncclSuccess;
      if (ncclCommGetAsyncError(c->comm, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress) {
        icp_ctx_abort_comm(c);
        return fail(ICP_HIP_ERCCL, std::string(what) + ": the communicator failed (" + ncclGetErrorString(ae) +
                                       "; a peer rank died or a link broke): communicator aborted, comm_init again");
      }
    }
    if (peers && c->cfg.peer_timeout_ms > 0 &&
        std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(c->cfg.peer_timeout_ms)) {
      if (c->comm) icp_ctx_abort_comm(c);
      c->comm_aborted = true;
      return fail(ICP_HIP_ERCCL, std::string(what) + ": no record within config.peer_timeout_ms (" +
                                     std::to_string(c->cfg.peer_timeout_ms) +
                                     " ms; a peer rank stalled or died): communicator aborted, comm_init again");
    }
    const hipError_t q = hipStreamQuery(s);
    if (q == hipSuccess && done()) break;
    if (q == hipSuccess) return fail(ICP_HIP_EDEVICE, std::string(what) + ": stream idle but the record was not published");
    if (q != hipErrorNotReady) return fail(ICP_HIP_EDEVICE, std::string(what) + ": " + hipGetErrorString(q));
  }
  return ICP_HIP_OK;
}

// config.wide_pass: 0 a source's first iterate (descent guesses: loose boxes) and any iterate after
// one with >= max(kWideAuto, waves / kWideAutoDiv) overflowing waves (surface data far from
// convergence); below that the ball search takes their queries sooner than a second launch (the
// blob's ~300 overflowing waves at 10M: a 100 us wide launch; profiles/r22/ab/ab_wide_auto.txt:
// 10M scene window +4.6 %, blob window +2.5 % against the fixed 256); 2 always
static constexpr double kWideAuto = 256.0;
#ifndef ICP_WIDE_AUTO_DIV
#define ICP_WIDE_AUTO_DIV 32
#endif
static constexpr double kWideAutoDiv = ICP_WIDE_AUTO_DIV;
static bool wide_pass_on(const icp_hip_ctx* c) {
  if (!c->cfg.scan32 || c->cfg.search != ICP_SEARCH_CERTIFIED || c->cfg.wide_pass == 1) return false;
  const double rel = (double)((c->n_src + 63) / 64) / kWideAutoDiv;
  const double thr = rel > kWideAuto ? rel : kWideAuto;
  return c->cfg.wide_pass == 2 || !c->have_prev || c->follow.last_wide >= thr;
}

// Step 1 of an iterate: the search's launch record over the resident source.
static NNLaunch search_launch(const icp_hip_ctx* c, const double* T_apply, bool apply, LoopDev* loop) {
  NNLaunch a = base_launch(c);
  a.loop = loop;
  a.x = c->x;
  a.y = c->y;
  a.z = c->z;
  a.pos_out = c->pos;
  a.dist_out = c->dist;
  a.n = c->n_src;
  a.apply = apply ? 1 : 0;
  if (T_apply)
    for (int k = 0; k < 12; k++) a.T[k] = T_apply[k];
  // the half pass pays off where many waves overflow: the first iterate of a source (descent
  // guesses, loose boxes; ~16 % of the waves at 10M). Later iterates overflow in ~0.2 % of the
  // waves, whose queries the ball search finishes sooner than a second serial launch.
  a.follow = carve_follow_lists(c->follow.ints, c->follow.guesses, c->follow.counts, c->n_src,
                                c->cfg.overflow_halves && !c->have_prev, wide_pass_on(c));
  a.have_prev = c->have_prev ? 1 : 0;
  a.wc_box = c->wc_box;
  a.wc_ents = c->wc_ents;
  a.wc_gen = c->wc_gen;
  a.wc_margin = c->cfg.candidate_margin / 256.0;
  a.wc_loose = c->cfg.candidate_loose / 100.0;
  a.wc_lead = (double)c->cfg.candidate_lead;
  // the wave records of the fused covariance sums (the wave search only)
  a.wstat = (c->cfg.search == ICP_SEARCH_CERTIFIED && c->cfg.fused_cull) ? c->wstat : nullptr;
  a.fz = c->it;
  return a;
}

// Step 2: the list counts and the debug counters cleared; the search's timing events (on dispatch
// packets) from ring slot `slot`, on every timing_stride-th iterate only.
static int clear_and_time(icp_hip_ctx* c, NNLaunch& a, int64_t slot, hipStream_t s) {
  HIP_TRY(c->follow.begin_search(s));
  if (c->dbg) HIP_TRY(hipMemsetAsync(c->dbg, 0, ICP_DBG_SLOTS * sizeof(unsigned long long), s));
  const bool timed = c->cfg.timing_stride > 0 && c->n_iterates % c->cfg.timing_stride == 0;
  c->timed[slot] = timed;
  a.ev_start = timed ? c->ring[slot][0] : nullptr;
  a.ev_fast_done = timed ? c->ring[slot][1] : nullptr;
  return ICP_HIP_OK;
}

static CullLaunch cull_record(const icp_hip_ctx* c, LoopDev* loop, WaveStat* wstat) {
  CullLaunch cl;
  cl.loop = loop;
  cl.x = c->x;
  cl.y = c->y;
  cl.z = c->z;
  cl.pos = c->pos;
  cl.pts = c->pts;
  cl.it = c->it;
  cl.part = c->cparts;
  cl.n = c->n_src;
  cl.dist = c->dist;
  cl.wstat = wstat;
  return cl;
}

// One of a multi-rank iterate's two record exchanges (which = 0, 1), timed where the slot is
static int gather_timed(icp_hip_ctx* c, int64_t slot, int which, const double* d_local, double* d_gathered, int count) {
  hipStream_t s = c->stream;
  hipEvent_t* xev = c->xring[slot];
  if (c->xtimed[slot] == 1) HIP_TRY(hipEventRecord(xev[2 * which], s));
  const auto h0 = std::chrono::steady_clock::now();
  const int rc = all_gather_record(c, d_local, d_gathered, count, s);
  if (c->xtimed[slot] == 2)
    c->xhost_ms[slot] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
  if (rc == ICP_HIP_OK && c->xtimed[slot] == 1) HIP_TRY(hipEventRecord(xev[2 * which + 1], s));
  return rc;
}

// Step 3: residual moments -> mean, std, threshold (no communicator: fused into the last merge level)
static int moments_step(icp_hip_ctx* c, int64_t slot, LoopDev* loop, bool multi, const MomentsFinalize& fin,
                        const CullLaunch& cl, hipStream_t s) {
  HIP_TRY(launch_moments_tail(c->dist, c->n_src, c->mparts, loop, c->tickets, c->it, multi ? nullptr : &fin, cl, s));
  // a timed multi-rank iterate also times its two record exchanges (icp_hip_exchange_timings):
  // events around the all-gathers over RCCL, the host clock around the host exchange's callback
  c->xtimed[slot] = (int8_t)(c->timed[slot] && multi ? (c->comm ? 1 : 2) : 0);
  c->xhost_ms[slot] = 0.0;
  hipEvent_t* xev = c->xring[slot];
  if (c->xtimed[slot] == 1)
    for (int k = 0; k < 4; k++)
      if (!xev[k]) HIP_TRY(hipEventCreateWithFlags(&xev[k], hipEventDisableSystemFence));
  if (multi) {
    const int rc = gather_timed(c, slot, 0, reinterpret_cast<const double*>(&c->it->m_local),
                                reinterpret_cast<double*>(c->gm), (int)(sizeof(Moments) / sizeof(double)));
    if (rc != ICP_HIP_OK) return rc;
    HIP_TRY(launch_finalize_moments(c->gm, c->nranks, c->it, fin, cl, s));
  }
  return ICP_HIP_OK;
}

// Step 4: covariance moments -> RMSE; the finished record is stored into pinned host memory (host
// loop, sequence number *seq) or steps the device session (device loop); the iterate-end event.
static int cull_step(icp_hip_ctx* c, int64_t slot, LoopDev* loop, int loop_slot, bool multi, const CullLaunch& cl,
                     hipStream_t s, uint64_t* seq) {
  IterPublish pub{nullptr, c->follow.counts, 0.0, nullptr, nullptr};
  if (loop) {
    pub.loop = loop;
    pub.rec = c->h_ring_dev + loop_slot;
  } else {
    *seq = ++c->publish_seq;
    pub.host = c->h_it_dev;
    pub.seq = (double)*seq;
  }
  HIP_TRY(launch_cull_tail(cl, c->tickets + ticket_words() / 2, multi ? nullptr : &pub, s));
  if (multi) {
    const int rc = gather_timed(c, slot, 1, reinterpret_cast<const double*>(&c->it->c_local),
                                reinterpret_cast<double*>(c->gc), (int)(sizeof(CovMoments) / sizeof(double)));
    if (rc != ICP_HIP_OK) return rc;
    HIP_TRY(launch_finalize_cov(c->gc, c->nranks, c->it, pub, s));
  }
  hipEvent_t* ev = c->ring[slot];
  HIP_TRY(hipEventRecord(ev[2], s));
  return ICP_HIP_OK;
}

// One iterate enqueued on the context's stream, no wait. Host-driven (loop_slot < 0): the
// transform T_apply (null: none) is a kernel argument and the last kernel publishes the record
// with sequence number *seq for the host's poll. Device loop (loop_slot >= 0): the transform is
// the device session's pending increment (applied when `apply`), the last kernel steps the session
// and stores the iteration's LoopRec into ring slot loop_slot.
static int enqueue_iterate(icp_hip_ctx* c, const double* T_apply, bool apply, int iter, int rules,
                           double sigma_multiplier, int loop_slot, uint64_t* seq_out) {
  if (c->comm_aborted)
    return fail(ICP_HIP_ERCCL, "iterate: the communicator was aborted (icp_hip_comm_abort or a peer failure); comm_init again");
  hipStream_t s = c->stream;
  int rc = prewalk_join(c, s);
  if (rc != ICP_HIP_OK) return rc;
  const int64_t slot = c->n_iterates % icp_hip_ctx::kTimingRing;
  LoopDev* loop = loop_slot >= 0 ? c->loopd : nullptr;
  NNLaunch a = search_launch(c, T_apply, apply, loop);
  if ((rc = clear_and_time(c, a, slot, s)) != ICP_HIP_OK) return rc;
  const bool prewalk = prewalk_arm(c, a, loop, apply);
  HIP_TRY(launch_nn(a, s));
  if (apply) c->src_moves++;  // the search moves the resident source (a device-loop iterate: may move it)
  if (prewalk && (rc = prewalk_launch(c, a)) != ICP_HIP_OK) return rc;
  const bool multi = c->comm != nullptr || c->xfn != nullptr;
  if (multi && c->inject_failure == 1) {  // testing hook: fail before joining the exchange
    c->inject_failure = 0;
    return fail(ICP_HIP_EDEVICE, "injected failure before the record exchange (icp_hip_debug_inject_failure)");
  }
  const MomentsFinalize fin{sigma_multiplier, iter, rules == ICP_RULES_ENGINE ? 1 : 0};
  const CullLaunch cl = cull_record(c, loop, a.wstat);
  if ((rc = moments_step(c, slot, loop, multi, fin, cl, s)) != ICP_HIP_OK) return rc;
  uint64_t seq = 0;
  if ((rc = cull_step(c, slot, loop, loop_slot, multi, cl, s, &seq)) != ICP_HIP_OK) return rc;
  c->n_iterates++;
  c->have_prev = true;  // the next iterate's search guesses from this one's matches
  if (seq_out) *seq_out = seq;
  return ICP_HIP_OK;
}

// A record's three list sizes (IterDev::lists, LoopRec::lists) back as counts.
static PublishedLists record_lists(const double lists[3]) {
  return PublishedLists{(unsigned int)lists[0], (unsigned int)lists[1], (unsigned int)lists[2]};
}

// The caller's statistics from the published record of a host-driven iterate.
static void stats_from_record(const icp_hip_ctx* c, const IterDev& h, icp_iter_stats* out) {
  out->n = (int64_t)h.m_global.n;
  out->mean = h.mean;
  out->std = h.sd;
  out->threshold = h.thr;
  out->valid = (int64_t)h.c_global.n;
  out->rmse = h.rmse;
  out->sum_d2 = h.c_global.sum_d2;
  out->min_d = h.m_global.dmin;
  out->max_d = h.m_global.dmax;
  out->n_bad = (int64_t)h.m_global.nbad;
  for (int k = 0; k < 3; k++) {
    out->centroid_src[k] = h.c_global.ma[k];
    out->centroid_tgt[k] = h.c_global.mb[k];
  }
  for (int k = 0; k < 9; k++) out->H[k] = h.c_global.c[k];
  const bool cert = c->cfg.search == ICP_SEARCH_CERTIFIED;
  out->n_fallback = cert ? (int64_t)c->follow.last.exact : 0;
  out->n_lane_search = cert ? (int64_t)c->follow.last.lane : 0;
  out->n_ball_search = cert ? (int64_t)c->follow.last.ball : 0;
}

extern "C" int icp_hip_iterate(icp_hip_ctx* c, const double* T_apply, int iter, int rules, double sigma_multiplier,
                               icp_iter_stats* out) {
  if (!c || !out) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return group_iterate(c, T_apply, iter, rules, sigma_multiplier, out);
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if (!c->x && c->n_src > 0) return fail(ICP_HIP_ENOTREADY, "source not set");
  HIP_TRY(hipSetDevice(c->device));
  uint64_t seq = 0;
  const int rc = enqueue_iterate(c, T_apply, T_apply != nullptr, iter, rules, sigma_multiplier, -1, &seq);
  if (rc != ICP_HIP_OK) return rc;
  // The host's only wait of the iteration: the publishing kernel stores the record with
  // system-scope stores, waits for their acknowledgement, then stores the sequence word (no
  // fence; reduce_kernels.hip finalize_cov_publish). Polling the pinned word wakes the host within
  // ~1 us; the stream is queried between polls so a device error still surfaces. The word is read
  // with acquire ordering, so the record's words are read after it.
  {
    const double want = (double)seq;
    uint64_t want_bits;
    std::memcpy(&want_bits, &want, sizeof(want));
    const uint64_t* word = reinterpret_cast<const uint64_t*>(&c->h_it->seq);
    const int wrc = wait_device(
        c, [&]() { return __atomic_load_n(word, __ATOMIC_ACQUIRE) == want_bits; }, []() { return (uint64_t)0; },
        "iterate");
    if (wrc != ICP_HIP_OK) return wrc;
  }
  const IterDev& h = *c->h_it;
  c->follow.published(record_lists(h.lists), h.n_wide);
  c->last_cull_path = h.cull_mode != 0.0 ? 1 : 0;
  stats_from_record(c, h, out);
  c->have_results = true;
  return ICP_HIP_OK;
}

bool icp_hip_loop_eligible(const icp_hip_ctx* c) {
  return c && !c->group && !c->xfn && c->cfg.device_loop && c->nodes && c->n_src > 0 && c->loopd;
}

int icp_hip_loop_run(icp_hip_ctx* c, icp::SessionCore* core, const icp::SessionParams* p, int rules, double sigma,
                     int k, icp::LoopRec* recs, double* step_ms) {
  if (!icp_hip_loop_eligible(c) || !core || !p || !recs || k < 0 || k > icp_hip_ctx::kLoopRing)
    return fail(ICP_HIP_EINVAL, "device loop: bad arguments");
  if (k == 0 || core->done) {
    for (int j = 0; j < k; j++) recs[j].outcome = icp::kStepNone;
    return ICP_HIP_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  c->h_loop->core = *core;
  c->h_loop->p = *p;
  HIP_TRY(hipMemcpyAsync(c->loopd, c->h_loop, sizeof(LoopDev), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(c->ev_batch, s));
  // the ring slots' outcome words, cleared to a sentinel: the batch's last kernels overwrite them
  // one iterate at a time (the host wait's progress)
  constexpr int32_t kUnset = 0x7fffffff;
  for (int j = 0; j < k; j++) __atomic_store_n(&c->h_ring[j].outcome, kUnset, __ATOMIC_RELAXED);
  const int64_t first = c->n_iterates;
  // Iteration j > 0 runs only if iteration j - 1 left the session going, i.e. produced a
  // transform: its search applies it. The first applies the session's pending increment.
  for (int j = 0; j < k; j++) {
    const int rc = enqueue_iterate(c, nullptr, j > 0 || core->pending, core->iter + j, rules, sigma, j, nullptr);
    if (rc != ICP_HIP_OK) return rc;
  }
  HIP_TRY(hipMemcpyAsync(c->h_loop, c->loopd, sizeof(LoopDev), hipMemcpyDeviceToHost, s));
  // (polled rather than hipStreamSynchronize: a batch over a communicator whose peer died would
  // otherwise wait forever)
  const int wrc = wait_device(
      c, [&]() { return hipStreamQuery(s) != hipErrorNotReady; },
      [&]() {
        uint64_t n = 0;
        for (int j = 0; j < k; j++) n += __atomic_load_n(&c->h_ring[j].outcome, __ATOMIC_RELAXED) != kUnset ? 1u : 0u;
        return n;
      },
      "device loop");
  if (wrc != ICP_HIP_OK) return wrc;
  const hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(ICP_HIP_EDEVICE, std::string("device loop: ") + hipGetErrorString(e));
  *core = c->h_loop->core;
  std::memcpy(recs, c->h_ring, (size_t)k * sizeof(icp::LoopRec));
  c->follow.counts_zero = true;  // every iteration's publish cleared them
  c->have_results = true;
  for (int j = k - 1; j >= 0; j--)
    if (recs[j].outcome != icp::kStepNone) {
      c->follow.published(record_lists(recs[j].lists), (double)recs[j].n_wide);
      break;
    }
  if (step_ms) {
    hipEvent_t prev = c->ev_batch;
    for (int j = 0; j < k; j++) {
      hipEvent_t end = c->ring[(first + j) % icp_hip_ctx::kTimingRing][2];
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, prev, end));
      step_ms[j] = ms;
      prev = end;
    }
  }
  return ICP_HIP_OK;
}

extern "C" {

int icp_hip_debug_counters(icp_hip_ctx* c, uint64_t out[ICP_DBG_SLOTS]) {
  if (!c || !out) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return group_debug_counters(c, out);
  std::memset(out, 0, ICP_DBG_SLOTS * sizeof(uint64_t));
  if (!c->dbg) return ICP_HIP_OK;
  HIP_TRY(hipSetDevice(c->device));
  drain_prewalk(c);  // slot ICP_DBG_PREWALK_STORES
  HIP_TRY(hipMemcpyAsync(out, c->dbg, ICP_DBG_SLOTS * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

int icp_hip_timings(icp_hip_ctx* c, int k, double* nn_ms, double* it_ms) {
  if (!c || k < 0) return fail(ICP_HIP_EINVAL, "bad arguments");
  if (c->group) return group_timings(c, k, nn_ms, it_ms);
  if (k > icp_hip_ctx::kTimingRing || k > c->n_iterates) return fail(ICP_HIP_EINVAL, "fewer iterates recorded than asked");
  HIP_TRY(hipSetDevice(c->device));
  for (int j = 0; j < k; j++) {
    const int64_t slot = (c->n_iterates - k + j) % icp_hip_ctx::kTimingRing;
    hipEvent_t* ev = c->ring[slot];
    HIP_TRY(hipEventSynchronize(ev[2]));
    double a = std::nan(""), b = std::nan("");
    if (c->timed[slot]) {
      float fa = 0.f, fb = 0.f;
      HIP_TRY(hipEventElapsedTime(&fa, ev[0], ev[1]));
      HIP_TRY(hipEventElapsedTime(&fb, ev[0], ev[2]));
      a = fa;
      b = fb;
    }
    if (nn_ms) nn_ms[j] = a;
    if (it_ms) it_ms[j] = b;
  }
  return ICP_HIP_OK;
}

int icp_hip_last_timing(icp_hip_ctx* c, double* nn_ms, double* it_ms) {
  if (!c) return fail(ICP_HIP_EINVAL, "null ctx");
  if (c->group) return group_timings(c, 1, nn_ms, it_ms);
  if (c->n_iterates == 0) return fail(ICP_HIP_ENOTREADY, "no iterate has run");
  if (!c->timed[(c->n_iterates - 1) % icp_hip_ctx::kTimingRing])
    return fail(ICP_HIP_ENOTREADY, "the last iterate was not timed (config.timing_stride)");
  return icp_hip_timings(c, 1, nn_ms, it_ms);
}

int icp_hip_exchange_timings(icp_hip_ctx* c, int k, double* ms) {
  if (!c || k < 0 || (k > 0 && !ms)) return fail(ICP_HIP_EINVAL, "bad arguments");
  if (c->group) return group_exchange_timings(c, k, ms);
  if (k > icp_hip_ctx::kTimingRing || k > c->n_iterates) return fail(ICP_HIP_EINVAL, "fewer iterates recorded than asked");
  HIP_TRY(hipSetDevice(c->device));
  for (int j = 0; j < k; j++) {
    const int64_t slot = (c->n_iterates - k + j) % icp_hip_ctx::kTimingRing;
    HIP_TRY(hipEventSynchronize(c->ring[slot][2]));
    double v = std::nan("");
    if (c->xtimed[slot] == 1) {
      float f0 = 0.f, f1 = 0.f;
      HIP_TRY(hipEventElapsedTime(&f0, c->xring[slot][0], c->xring[slot][1]));
      HIP_TRY(hipEventElapsedTime(&f1, c->xring[slot][2], c->xring[slot][3]));
      v = (double)f0 + (double)f1;
    } else if (c->xtimed[slot] == 2) {
      v = c->xhost_ms[slot];
    }
    ms[j] = v;
  }
  return ICP_HIP_OK;
}

int icp_hip_last_cull_path(icp_hip_ctx* c, int32_t* fused) {
  if (!c || !fused) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return group_cull_path(c, fused);
  if (c->last_cull_path < 0) return fail(ICP_HIP_ENOTREADY, "no host-published iterate on this source");
  *fused = c->last_cull_path;
  return ICP_HIP_OK;
}

}  // extern "C"
