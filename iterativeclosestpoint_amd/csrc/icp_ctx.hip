// icp_ctx.hip — the C-ABI context of libicp_hip.so (include/icp_hip.h): configuration, lifetime, warm-up,
// error string. Beside it: ctx_comm.cpp (transport), ctx_clouds.cpp, ctx_iterate.cpp, ctx_prewalk.cpp.
//
// One context = one GPU = one HIP stream. Everything that belongs to the path lives in HBM for
// the whole registration: the linear octree (64-B node records), the leaf-ordered target
// (32-B points), the Morton-ordered source shard as SoA x/y/z, per-query match position and
// residual, block partials. Per iteration the host sees one 1 KB record (IterDev).
// Multi-GPU: each rank holds its shard of the source and a replica of the octree; the two
// per-iteration exchanges are RCCL all-gathers of one Moments / one CovMoments record, merged
// on the device in rank order, so every rank computes bitwise-identical statistics.
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/icp_host.h"
#include "icp_ctx_internal.h"

using namespace icp;

static thread_local std::string g_err;
void icp_ctx_set_error(const char* msg) { g_err = msg; }

// Process warm-up (icp_hip_config.no_warmup = 0). HIP loads a kernel's code object and sizes the
// queue's scratch at the kernel's first launch in the process; without a warm-up that cost
// (+1.3 ms at 10M, measured: first iterate 4.15 ms cold, 2.85 ms warm) lands in the first iterate
// of the first registration. A 3-iterate registration of a small synthetic pair on a private
// context with the same search options (the same kernel instances: first-iterate descent, half
// pass, ball search, the storing and the reusing search, full and fused culls) loads them, once
// per (device, options) per process. Failures are ignored: the real context works without it.
static void warm_kernels(int device, const icp_hip_config& conf) {
  static std::mutex mu;
  static std::vector<std::pair<int, uint64_t>> done;
  const uint64_t key = (uint64_t)conf.search | (uint64_t)conf.scan_groups << 4 | (uint64_t)conf.certify_prev << 8 |
                       (uint64_t)(conf.debug_counters != 0) << 12 | (uint64_t)conf.fused_cull << 13 |
                       (uint64_t)conf.overflow_halves << 14 | (uint64_t)conf.scan32 << 15 |
                       (uint64_t)conf.candidate_cache << 16 | (uint64_t)conf.ball_mode << 17 |
                       (uint64_t)conf.wide_pass << 19;
  std::lock_guard<std::mutex> lk(mu);
  for (const auto& d : done)
    if (d.first == device && d.second == key) return;
  done.emplace_back(device, key);
  const std::string saved = g_err;
  constexpr int64_t kN = 4096;
  std::vector<double> tgt(3 * kN), src(3 * kN);
  double Ttrue[16];
  icp_synth_spec sp;
  icp_synth_default(&sp);
  icp_hip_config wc = conf;
  wc.no_warmup = 1;
  wc.timing_stride = 0;
  wc.peer_timeout_ms = 0;
  icp_hip_ctx* w = nullptr;
  if (icp_synth_pair(&sp, kN, kN, tgt.data(), src.data(), Ttrue) == 0 && icp_hip_create_ex(&w, device, &wc) == 0 &&
      icp_hip_set_target(w, tgt.data(), kN, 10, 20, ICP_RULES_ENGINE) == 0 && icp_hip_set_source(w, src.data(), kN) == 0) {
    prewalk_warm(w);
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    icp_iter_stats st;
    for (int k = 0; k < 3; ++k)
      if (icp_hip_iterate(w, k ? I : nullptr, k, ICP_RULES_ENGINE, 3.0, &st) != 0) break;
  }
  icp_hip_destroy(w);
  icp_ctx_set_error(saved.c_str());
}

// What is wrong with a configuration (candidate_loose 0 already replaced by its default), or null.
static const char* check_config(const icp_hip_config& conf) {
  for (int k = 0; k < 3; k++)
    if (conf.reserved[k] != 0) return "config: reserved words must be zero";
  if (conf.wide_pass < 0 || conf.wide_pass > 2) return "config: wide_pass out of [0, 2]";
  if (conf.peer_timeout_ms < 0) return "config: peer_timeout_ms must be >= 0";
  if (conf.no_warmup != 0 && conf.no_warmup != 1) return "config: no_warmup must be 0 or 1";
  if (conf.ball_mode < 0 || conf.ball_mode > 2) return "config: ball_mode out of [0, 2]";
  if (conf.search != ICP_SEARCH_CERTIFIED && conf.search != ICP_SEARCH_REFERENCE) return "config: unknown search";
  if (conf.octree_builder != ICP_BUILD_AUTO && conf.octree_builder != ICP_BUILD_HOST) return "config: unknown octree builder";
  if (conf.scan_groups != 1 && conf.scan_groups != 2 && conf.scan_groups != 4) return "config: scan_groups must be 1, 2 or 4";
  if (conf.xcd_blocks < 0 || conf.xcd_blocks > (1 << 20)) return "config: xcd_blocks out of [0, 2^20]";
  if (conf.candidate_cache != 0 && conf.candidate_cache != 1) return "config: candidate_cache must be 0 or 1";
  if (conf.candidate_margin < 0 || conf.candidate_margin > 1024) return "config: candidate_margin out of [0, 1024]";
  if (conf.candidate_loose < 100 || conf.candidate_loose > 100000) return "config: candidate_loose out of [100, 100000]";
  if (conf.candidate_lead < 0 || conf.candidate_lead > 64) return "config: candidate_lead out of [0, 64]";
  if (conf.fused_cull < 0 || conf.fused_cull > 1) return "config: fused_cull must be 0 or 1";
  if (conf.overflow_halves != 0 && conf.overflow_halves != 1) return "config: overflow_halves must be 0 or 1";
  if (conf.query_order != 0 && conf.query_order != 1) return "config: query_order must be 0 or 1";
  if (conf.certify_prev < 0 || conf.certify_prev > 3) return "config: certify_prev out of [0, 3]";
  if (conf.device_loop != 0 && conf.device_loop != 1) return "config: device_loop must be 0 or 1";
  if (conf.timing_stride < 0) return "config: timing_stride must be >= 0";
  if (!(conf.join_factor >= 1.0 && conf.join_factor <= 1e6)) return "config: join_factor out of [1, 1e6]";
  return nullptr;
}

extern "C" {

int icp_hip_device_count(int* count) {
  HIP_TRY(hipGetDeviceCount(count));
  return ICP_HIP_OK;
}

void icp_hip_config_default(icp_hip_config* cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->search = ICP_SEARCH_CERTIFIED;
  cfg->scan32 = 1;
  cfg->cell_starts = 1;
  cfg->octree_builder = ICP_BUILD_AUTO;
  cfg->join_factor = 3.0;
  cfg->debug_counters = 0;
  cfg->xcd_blocks = 256;
  cfg->scan_groups = 4;
  cfg->candidate_cache = 1;
  cfg->candidate_margin = 16;
  cfg->candidate_loose = 1500;
  cfg->candidate_lead = 8;
  cfg->fused_cull = 1;
  cfg->overflow_halves = 0;
  cfg->device_loop = 0;
  cfg->timing_stride = 0;
  cfg->peer_timeout_ms = 0;
  cfg->config_version = ICP_HIP_CONFIG_VERSION;
}

int icp_hip_create(icp_hip_ctx** out, int device) { return icp_hip_create_ex(out, device, nullptr); }

int icp_hip_create_ex(icp_hip_ctx** out, int device, const icp_hip_config* cfg) {
  if (!out) return fail(ICP_HIP_EINVAL, "null out");
  *out = nullptr;
  icp_hip_config conf;
  icp_hip_config_default(&conf);
  // the version word comes first: checked before the struct is copied (a struct of another
  // header version may be shorter than this one)
  if (cfg && cfg->config_version != ICP_HIP_CONFIG_VERSION)
    return fail(ICP_HIP_EINVAL, "config: config_version is not ICP_HIP_CONFIG_VERSION (start from icp_hip_config_default "
                                "of this header)");
  if (cfg) conf = *cfg;
  if (conf.candidate_loose == 0) conf.candidate_loose = 1500;
  if (const char* bad = check_config(conf)) return fail(ICP_HIP_EINVAL, bad);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(ICP_HIP_EDEVICE, std::string("no HIP device available: ") + hipGetErrorString(e));
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  if (device >= ndev) return fail(ICP_HIP_EINVAL, "device ordinal out of range");
  HIP_TRY(hipSetDevice(device));
  icp_hip_ctx* c = new icp_hip_ctx();
  c->device = device;
  c->cfg = conf;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(ICP_HIP_EDEVICE, "hipStreamCreate failed");
  }
  for (hipEvent_t* ev : {&c->ev_it0, &c->ev_it1}) (void)hipEventCreate(ev);
  (void)hipEventCreateWithFlags(&c->ev_batch, hipEventDisableSystemFence);
  prewalk_init(c);  // (its stream and buffers: at set_source)
  // The per-iterate timing ring only measures elapsed times: no system-scope fence on record
  // (a default event's release writes back L2, ~5 us of GPU idle per record between kernels).
  for (auto& r : c->ring)
    for (hipEvent_t& ev : r) (void)hipEventCreateWithFlags(&ev, hipEventDisableSystemFence);
  if (dalloc(&c->it, 1) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&c->h_it), sizeof(IterDev), hipHostMallocMapped | hipHostMallocCoherent) !=
          hipSuccess ||
      hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_it_dev), c->h_it, 0) != hipSuccess ||
      dalloc(&c->counters, 2) != hipSuccess || c->follow.alloc(-1) != hipSuccess ||
      dalloc(&c->loopd, 1) != hipSuccess ||
      dalloc(&c->tickets, (size_t)ticket_words()) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&c->h_loop), sizeof(LoopDev)) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&c->h_ring), icp_hip_ctx::kLoopRing * sizeof(LoopRec),
                    hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_ring_dev), c->h_ring, 0) != hipSuccess ||
      (conf.debug_counters && dalloc(&c->dbg, ICP_DBG_SLOTS) != hipSuccess)) {
    icp_hip_destroy(c);
    return fail(ICP_HIP_ENOMEM, "context allocation failed");
  }
  (void)hipMemset(c->it, 0, sizeof(IterDev));
  (void)hipMemset(c->tickets, 0, (size_t)ticket_words() * sizeof(unsigned int));
  if (c->dbg) (void)hipMemset(c->dbg, 0, ICP_DBG_SLOTS * sizeof(unsigned long long));
  std::memset(c->h_it, 0, sizeof(IterDev));
  if (!conf.no_warmup) warm_kernels(device, conf);
  *out = c;
  return ICP_HIP_OK;
}

void icp_hip_destroy(icp_hip_ctx* c) {
  if (!c) return;
  if (c->group) {
    group_destroy(c);
    delete c;
    return;
  }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  prewalk_destroy(c);
  las_destroy(c);
  reject_destroy(c);
  gicp_destroy(c);
  free_source(c);
  free_target(c);
  dfree(c->it);
  dfree(c->counters);
  c->follow.release(true);
  dfree(c->tickets);
  dfree(c->dbg);
  dfree(c->gm);
  dfree(c->gc);
  if (c->h_it) (void)hipHostFree(c->h_it);
  dfree(c->loopd);
  if (c->h_loop) (void)hipHostFree(c->h_loop);
  if (c->h_ring) (void)hipHostFree(c->h_ring);
  if (c->ev_batch) (void)hipEventDestroy(c->ev_batch);
  icp_ctx_drop_transport(c);
  for (hipEvent_t ev : {c->ev_it0, c->ev_it1})
    if (ev) (void)hipEventDestroy(ev);
  for (auto& r : c->ring)
    for (hipEvent_t ev : r)
      if (ev) (void)hipEventDestroy(ev);
  for (auto& r : c->xring)
    for (hipEvent_t ev : r)
      if (ev) (void)hipEventDestroy(ev);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int icp_hip_synchronize(icp_hip_ctx* c) {
  if (!c) return fail(ICP_HIP_EINVAL, "null ctx");
  if (c->group) return group_synchronize(c);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return prewalk_synchronize(c);
}

const char* icp_hip_last_error(void) { return g_err.c_str(); }

}  // extern "C"
