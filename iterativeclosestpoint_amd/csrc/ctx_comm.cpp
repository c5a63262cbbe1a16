// ctx_comm.cpp — the context's transport: the RCCL communicator or the caller's host exchange, the
// per-iteration all-gather of one record over either, and the failure hooks.
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "icp_ctx_internal.h"

using namespace icp;

// The host-exchange callback run on a thread of its own, so that the iterate can give up on it
// at config.peer_timeout_ms (the callback is the caller's code: it cannot be interrupted, only
// abandoned). One job at a time; an abandoned job finishes on its own, and join() (comm_init,
// comm_init_host, destroy) waits for it.
struct ExchangeWorker {
  std::mutex m;
  std::condition_variable cv;
  std::thread th;
  bool job = false, done = false, quit = false;
  icp_hip_exchange_fn fn = nullptr;
  void* user = nullptr;
  std::vector<double> local, all;
  int count = 0, rc = 0;

  ExchangeWorker() {
    th = std::thread([this] {
      std::unique_lock<std::mutex> lk(m);
      while (true) {
        cv.wait(lk, [this] { return job || quit; });
        if (quit && !job) return;
        lk.unlock();
        const int r = fn(user, local.data(), count, all.data());
        lk.lock();
        rc = r;
        job = false;
        done = true;
        cv.notify_all();
      }
    });
  }
  // The callback on this rank's record; 0 = done in time (gathered in `all`), 1 = the deadline
  // passed first (the job stays with the thread).
  int run(icp_hip_exchange_fn f, void* u, const double* rec, int n, int nranks, int timeout_ms) {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [this] { return !job; });  // an abandoned job first
    fn = f;
    user = u;
    count = n;
    local.assign(rec, rec + n);
    all.assign((size_t)n * nranks, 0.0);
    done = false;
    job = true;
    cv.notify_all();
    if (!cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), [this] { return done; })) return 1;
    return 0;
  }
  void join() {
    {
      std::lock_guard<std::mutex> lk(m);
      quit = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
  ~ExchangeWorker() { join(); }
};

void icp_ctx_drop_transport(icp_hip_ctx* c) {
  if (c->comm) (void)ncclCommDestroy(c->comm);
  c->comm = nullptr;
  delete c->xworker;  // waits for a callback that overran the deadline to return
  c->xworker = nullptr;
  c->comm_aborted = false;
  c->xfn = nullptr;
  c->xuser = nullptr;
  c->nranks = 1;
  c->rank = 0;
}

void icp_ctx_abort_comm(icp_hip_ctx* c) {
  if (!c->comm) return;
  (void)hipSetDevice(c->device);
  // the collectives this communicator has enqueued return (their outputs are garbage, never read:
  // the iterate that enqueued them has failed), so the stream drains
  (void)ncclCommAbort(c->comm);
  c->comm = nullptr;
  c->comm_aborted = true;
  (void)hipStreamSynchronize(c->stream);
  (void)hipGetLastError();
}

// The all-gather's receive buffers, one record per rank.
static int realloc_gather(icp_hip_ctx* c, int nranks) {
  dfree(c->gm);
  dfree(c->gc);
  HIP_TRY(dalloc(&c->gm, (size_t)nranks));
  HIP_TRY(dalloc(&c->gc, (size_t)nranks));
  return ICP_HIP_OK;
}

int icp_ctx_attach_comm(icp_hip_ctx* c, ncclComm_t comm, int nranks, int rank) {
  HIP_TRY(hipSetDevice(c->device));
  icp_ctx_drop_transport(c);
  if (const int rc = realloc_gather(c, nranks)) return rc;
  c->comm = comm;
  c->nranks = nranks;
  c->rank = rank;
  return ICP_HIP_OK;
}

int all_gather_record(icp_hip_ctx* c, const double* d_local, double* d_gathered, int count, hipStream_t s) {
  if (c->comm) {
    RCCL_TRY(ncclAllGather(d_local, d_gathered, (size_t)count, ncclDouble, c->comm, s));
    return ICP_HIP_OK;
  }
  std::vector<double> local((size_t)count), all((size_t)count * c->nranks);
  HIP_TRY(hipMemcpyAsync(local.data(), d_local, sizeof(double) * count, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (c->cfg.peer_timeout_ms > 0) {
    // the callback on the exchange thread, given up on at the deadline (it cannot be interrupted:
    // it finishes on that thread, and comm_init / comm_init_host / destroy wait for it)
    if (!c->xworker) c->xworker = new ExchangeWorker();
    if (c->xworker->run(c->xfn, c->xuser, local.data(), count, c->nranks, c->cfg.peer_timeout_ms) != 0) {
      c->comm_aborted = true;
      return fail(ICP_HIP_EEXCHANGE, "host exchange callback overran config.peer_timeout_ms (" +
                                         std::to_string(c->cfg.peer_timeout_ms) + " ms); comm_init_host again");
    }
    if (c->xworker->rc != 0) return fail(ICP_HIP_EEXCHANGE, "host exchange callback failed");
    all.swap(c->xworker->all);
  } else if (c->xfn(c->xuser, local.data(), count, all.data()) != 0) {
    return fail(ICP_HIP_EEXCHANGE, "host exchange callback failed");
  }
  HIP_TRY(hipMemcpyAsync(d_gathered, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return ICP_HIP_OK;
}

extern "C" {

int icp_hip_get_unique_id(uint8_t out[ICP_HIP_UNIQUE_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) == ICP_HIP_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId id;
  RCCL_TRY(ncclGetUniqueId(&id));
  std::memcpy(out, &id, sizeof(id));
  return ICP_HIP_OK;
}

int icp_hip_comm_init(icp_hip_ctx* c, int nranks, int rank, const uint8_t id_bytes[ICP_HIP_UNIQUE_ID_BYTES]) {
  if (c && c->group) return fail(ICP_HIP_EINVAL, "a multi-device context owns its communicators");
  if (!c || !id_bytes || nranks < 1 || rank < 0 || rank >= nranks) return fail(ICP_HIP_EINVAL, "bad comm arguments");
  HIP_TRY(hipSetDevice(c->device));
  // back to a world of one first: a failure below leaves no stale transport behind
  icp_ctx_drop_transport(c);
  if (const int rc = realloc_gather(c, nranks)) return rc;
  ncclUniqueId id;
  std::memcpy(&id, id_bytes, sizeof(id));
  ncclComm_t comm = nullptr;
  RCCL_TRY(ncclCommInitRank(&comm, nranks, id, rank));
  c->comm = comm;
  c->nranks = nranks;
  c->rank = rank;
  return ICP_HIP_OK;
}

int icp_hip_comm_init_host(icp_hip_ctx* c, int nranks, int rank, icp_hip_exchange_fn exchange, void* user) {
  if (c && c->group) return fail(ICP_HIP_EINVAL, "a multi-device context owns its communicators");
  if (!c || nranks < 1 || rank < 0 || rank >= nranks || (nranks > 1 && !exchange))
    return fail(ICP_HIP_EINVAL, "bad comm arguments");
  HIP_TRY(hipSetDevice(c->device));
  icp_ctx_drop_transport(c);
  if (!exchange) return ICP_HIP_OK;  // a world of one without a transport
  if (const int rc = realloc_gather(c, nranks)) return rc;
  c->xfn = exchange;
  c->xuser = user;
  c->nranks = nranks;
  c->rank = rank;
  return ICP_HIP_OK;
}

int icp_hip_comm_info(icp_hip_ctx* c, int member, int32_t* count, int32_t* rank, int32_t* device, int32_t* transport) {
  if (!c) return fail(ICP_HIP_EINVAL, "null ctx");
  if (c->group) return group_comm_info(c, member, count, rank, device, transport);
  if (member != 0) return fail(ICP_HIP_EINVAL, "a single-device context has member 0 only");
  int n = c->nranks, r = c->rank, d = c->device;
  if (c->comm) {
    // RCCL's own view of the communicator, not the arguments it was created with
    RCCL_TRY(ncclCommCount(c->comm, &n));
    RCCL_TRY(ncclCommUserRank(c->comm, &r));
    RCCL_TRY(ncclCommCuDevice(c->comm, &d));
  }
  if (count) *count = n;
  if (rank) *rank = r;
  if (device) *device = d;
  if (transport) *transport = c->comm ? ICP_XPORT_RCCL : c->xfn ? ICP_XPORT_CALLBACK : ICP_XPORT_AUTO;
  return ICP_HIP_OK;
}

int icp_hip_comm_abort(icp_hip_ctx* c) {
  if (!c) return fail(ICP_HIP_EINVAL, "null ctx");
  if (c->group) return fail(ICP_HIP_EINVAL, "a multi-device context aborts its communicators itself");
  icp_ctx_abort_comm(c);
  return ICP_HIP_OK;
}

int icp_hip_debug_inject_failure(icp_hip_ctx* c, int member, int where) {
  if (!c || where < 0 || where > 1) return fail(ICP_HIP_EINVAL, "bad arguments");
  if (c->group) return group_inject_failure(c, member, where);
  if (member != 0) return fail(ICP_HIP_EINVAL, "a single-device context has member 0 only");
  c->inject_failure = where;
  return ICP_HIP_OK;
}

}  // extern "C"
