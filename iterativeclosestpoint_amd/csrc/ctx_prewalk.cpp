// ctx_prewalk.cpp — the prewalk's host side (the kernels: launch_prewalk, nn_kernels.hip): its build
// switches, the side stream and buffers (icp_hip_ctx::pw), the drain, an iterate's three calls.
#include "icp_ctx_internal.h"

using namespace icp;

// The prewalk's look-ahead without a setter call (0: off).
#ifndef ICP_PREWALK_LOOK
#define ICP_PREWALK_LOOK 0
#endif
// ... which applies from this many waves up: below, an iterate is too short to hide a second
// stream's launches behind its statistics kernels (100k points: ~70 us per iterate).
static constexpr int64_t kPrewalkMinWaves = 16384;
// The side stream at the device's lowest stream priority (1), so that its waves are dispatched
// behind the statistics kernels of the main stream, or at the default priority (0).
#ifndef ICP_PREWALK_LOW_PRIO
#define ICP_PREWALK_LOW_PRIO 1
#endif
// The next search after a prewalk waits for it on the device (0: hipStreamWaitEvent in front of
// the search) or on the host (1: before the search is enqueued).
#ifndef ICP_PREWALK_JOIN_HOST
#define ICP_PREWALK_JOIN_HOST 0
#endif

void drain_prewalk(icp_hip_ctx* c) {
  if (c->pw.stream && c->pw.pending) (void)hipStreamSynchronize(c->pw.stream);
  c->pw.pending = false;
}

// What the prewalk needs beyond the candidate cache, made when it is first switched on (the
// setter, or a build whose default look-ahead is not 0) and for every source set after that: the
// side stream, its two events and the request counter (once per context), the request records
// (stamp 0: none) and the list, capped at an eighth of the waves (per source). A context that
// never prewalks has none of it. false: something could not be made; the context then runs
// without the prewalk (identical results) and `what` says why.
static bool ensure_prewalk(icp_hip_ctx* c, const char** what) {
  Prewalk& pw = c->pw;
  if (!pw.stream) {
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipStreamCreateWithPriority(&pw.stream, hipStreamNonBlocking, ICP_PREWALK_LOW_PRIO ? prio_least : 0) !=
            hipSuccess &&
        hipStreamCreateWithFlags(&pw.stream, hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();
      pw.stream = nullptr;
      *what = "the prewalk's stream could not be created";
      return false;
    }
  }
  if ((!pw.ev_fork && hipEventCreateWithFlags(&pw.ev_fork, hipEventDisableTiming) != hipSuccess) ||
      (!pw.ev_done && hipEventCreateWithFlags(&pw.ev_done, hipEventDisableTiming) != hipSuccess) ||
      (!pw.count && dalloc(&pw.count, 1) != hipSuccess)) {
    (void)hipGetLastError();
    *what = "the prewalk's events or counter could not be created";
    return false;
  }
  if (c->wc_box && c->n_src > 0 && (!pw.req || !pw.list)) {
    const size_t nw = (size_t)((c->n_src + 63) / 64);
    dfree(pw.req);
    dfree(pw.list);
    pw.cap = (unsigned int)(nw / 8 > 64 ? nw / 8 : 64);
    if (dalloc(&pw.req, 2 * nw) != hipSuccess || dalloc(&pw.list, 8 * (size_t)pw.cap) != hipSuccess ||
        hipMemsetAsync(pw.req, 0, 2 * nw * sizeof(int4), c->stream) != hipSuccess) {
      (void)hipGetLastError();
      dfree(pw.req);
      dfree(pw.list);
      *what = "no memory for the prewalk's request records";
      return false;
    }
  }
  return true;
}

void prewalk_init(icp_hip_ctx* c) { c->pw.look = (double)(ICP_PREWALK_LOOK); }

void prewalk_warm(icp_hip_ctx* w) { if ((ICP_PREWALK_LOOK) > 0) (void)icp_hip_set_prewalk(w, (double)(ICP_PREWALK_LOOK)); }

void prewalk_new_source(icp_hip_ctx* c) {
  const char* why = nullptr;
  if (c->pw.look > 0.0) (void)ensure_prewalk(c, &why);
}

void prewalk_free_source(icp_hip_ctx* c) {
  drain_prewalk(c);
  dfree(c->pw.req);
  dfree(c->pw.list);
}

void prewalk_destroy(icp_hip_ctx* c) {
  Prewalk& pw = c->pw;
  if (pw.stream) (void)hipStreamSynchronize(pw.stream);
  pw.pending = false;
  prewalk_free_source(c);
  dfree(pw.count);
  if (pw.ev_fork) (void)hipEventDestroy(pw.ev_fork);
  if (pw.ev_done) (void)hipEventDestroy(pw.ev_done);
  if (pw.stream) (void)hipStreamDestroy(pw.stream);
  pw = Prewalk();
}

int prewalk_synchronize(icp_hip_ctx* c) {
  if (c->pw.stream) HIP_TRY(hipStreamSynchronize(c->pw.stream));
  c->pw.pending = false;
  return ICP_HIP_OK;
}

int prewalk_join(icp_hip_ctx* c, hipStream_t s) {
  if (!c->pw.pending) return ICP_HIP_OK;
  if (ICP_PREWALK_JOIN_HOST) HIP_TRY(hipEventSynchronize(c->pw.ev_done));
  else HIP_TRY(hipStreamWaitEvent(s, c->pw.ev_done, 0));
  c->pw.pending = false;
  return ICP_HIP_OK;
}

bool prewalk_arm(icp_hip_ctx* c, NNLaunch& a, const LoopDev* loop, bool apply) {
  Prewalk& pw = c->pw;
  const bool prewalk = pw.look > 0.0 && (pw.explicit_ || (c->n_src + 63) / 64 >= kPrewalkMinWaves) && !loop && apply &&
                       c->have_prev && c->cfg.search == ICP_SEARCH_CERTIFIED && c->wc_box && pw.req && pw.list &&
                       pw.stream && pw.ev_fork && pw.ev_done && pw.count;
  if (prewalk) {
    a.wc_req = pw.req;
    a.wc_stamp = ++pw.stamp;
    a.ev_fork = pw.ev_fork;
    a.pw_look = pw.look;
    a.pw_list = pw.list;
    a.pw_count = pw.count;
    a.pw_cap = pw.cap;
  }
  return prewalk;
}

int prewalk_launch(icp_hip_ctx* c, const NNLaunch& a) {
  // (pending from here on: a launch that fails half-way may have enqueued its first kernels,
  // and whatever frees the record buffers drains the side stream first)
  c->pw.pending = true;
  HIP_TRY(launch_prewalk(a, c->pw.stream, c->pw.ev_fork, c->pw.ev_done));
  return ICP_HIP_OK;
}

extern "C" int icp_hip_set_prewalk(icp_hip_ctx* c, double look_ahead) {
  if (!c) return fail(ICP_HIP_EINVAL, "null ctx");
  if (!(look_ahead >= 0.0 && look_ahead <= 64.0)) return fail(ICP_HIP_EINVAL, "set_prewalk: look_ahead out of [0, 64]");
  if (c->group) return group_set_prewalk(c, look_ahead);
  if (look_ahead > 0.0) {
    HIP_TRY(hipSetDevice(c->device));
    const char* why = "";
    if (!ensure_prewalk(c, &why)) return fail(ICP_HIP_ENOMEM, std::string("set_prewalk: ") + why);
  }
  c->pw.look = look_ahead;
  c->pw.explicit_ = true;
  return ICP_HIP_OK;
}
