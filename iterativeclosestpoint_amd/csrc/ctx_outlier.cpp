// ctx_outlier.cpp — the context side of outlier removal: the argument checks, the
// call's private octree and scratch, the phases of outlier_kernels.hip on the context's stream with
// the two small read-backs between them, and the host, device and group forms around that core
// (§3.8). It reads no target or source of the context and changes none.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "icp_ctx_internal.h"
#include "octree_gpu.h"
#include "phase_events.h"

using namespace icp;

namespace {

// The private octree's shape: the CLI's (leaves of at most 10 points, depth at most 20). The
// results do not depend on it.
constexpr int kOutlierLeafPoints = 10;
constexpr int kOutlierMaxDepth = 20;

std::string outlier_cap_text(int64_t m, int64_t cap) {
  return "outlier_filter: " + std::to_string(m) + " points kept, the outputs' capacity is " + std::to_string(cap);
}

// The checks that need no device: everything of the definition but the coordinates.
int outlier_args(icp_hip_ctx* c, const double* xyz, int64_t n, int mode, int k, double param, int64_t* m_out) {
  if (!c || !m_out) return fail(ICP_HIP_EINVAL, "outlier_filter: null argument");
  *m_out = 0;
  if (mode != ICP_OUTLIER_STATISTICAL && mode != ICP_OUTLIER_RADIUS)
    return fail(ICP_HIP_EINVAL, "outlier_filter: unknown mode " + std::to_string(mode));
  if (n < 2 || n > INT32_MAX) return fail(ICP_HIP_EINVAL, "outlier_filter: n must be in [2, 2^31 - 1]");
  if (mode == ICP_OUTLIER_STATISTICAL) {
    const int64_t kmax = n - 1 < ICP_HIP_KNN_MAX ? n - 1 : ICP_HIP_KNN_MAX;
    if (k < 1 || k > kmax) return fail(ICP_HIP_EINVAL, "outlier_filter: k must be in [1, min(" + std::to_string(ICP_HIP_KNN_MAX) + ", n - 1)]");
    if (!std::isfinite(param)) return fail(ICP_HIP_EINVAL, "outlier_filter: std_ratio must be finite");
  } else {
    if (k < 1 || k > n - 1) return fail(ICP_HIP_EINVAL, "outlier_filter: the minimum of neighbours must be in [1, n - 1]");
    if (!std::isfinite(param) || !(param > 0.0)) return fail(ICP_HIP_EINVAL, "outlier_filter: the radius must be finite and > 0");
  }
  if (!xyz) return fail(ICP_HIP_EINVAL, "outlier_filter: null cloud");
  return ICP_HIP_OK;
}

// The call after the argument checks, in its host form (to_host: the cloud is uploaded, the outputs
// get the first m entries of scratch buffers) or on the caller's device buffers.
int outlier_core(icp_hip_ctx* c, const double* xyz_in, int64_t n, int mode, int k, double param, int64_t cap,
                 bool to_host, double* xyz_out, int32_t* index_out, double* score_out, int64_t* m_out,
                 icp_outlier_stats* stats) {
  OutlierHead hd;  // before the scratch: outlives the copies into it
  std::memset(&hd, 0, sizeof(hd));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  PhaseEvents<5> ev;  // build, scores, statistics, flags + sum, gather
  ScopedOctree oct;
  DevScratch S;
  double* up = nullptr;
  if (to_host) HIP_TRY(call_upload(S, &up, xyz_in, 3 * (size_t)n, s));
  const double* d_xyz = to_host ? up : xyz_in;
  CallOut<double> xyz(xyz_out, to_host), scores(score_out, to_host);
  CallOut<int32_t> index(index_out, to_host);

  HIP_TRY(ev.mark(0, s));
  {
    std::string why;
    if (const int rc = gpu_build_octree(d_xyz, n, kOutlierLeafPoints, kOutlierMaxDepth, s, &oct.t, &why))
      return fail_octree_build(rc, why);
  }
  HIP_TRY(ev.mark(1, s));
  const int levels = oct.t.max_inner_depth + 1 > 0 ? oct.t.max_inner_depth + 1 : 1;

  OutlierHead* head = nullptr;
  double *score = nullptr, *parts = nullptr;
  int32_t *flag = nullptr, *pos = nullptr;
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  HIP_TRY(outlier_temp_bytes(n, &tmp_bytes));
  HIP_TRY(S.alloc(&head, 1));
  HIP_TRY(S.alloc(&score, (size_t)n));
  HIP_TRY(S.alloc(&parts, 2 * (size_t)outlier_num_parts(n)));
  HIP_TRY(S.alloc(&flag, (size_t)n));
  HIP_TRY(S.alloc(&pos, (size_t)n));
  HIP_TRY(S.alloc(&tmp, tmp_bytes));

  HIP_TRY(ev.mark(2, s));
  HIP_TRY(launch_outlier_scores(oct.t.nodes, oct.t.pts, levels, n, mode, k, param, score, s));
  HIP_TRY(ev.mark(3, s));
  HIP_TRY(ev.mark(4, s));
  HIP_TRY(launch_outlier_stats(score, n, mode, k, param, parts, head, s));
  HIP_TRY(ev.mark(5, s));
  HIP_TRY(hipMemcpyAsync(&hd, head, sizeof(hd), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // the head record: the statistics the caller gets
  const double mean = hd.mean, sd = hd.sd, thr = hd.threshold;

  HIP_TRY(ev.mark(6, s));
  HIP_TRY(launch_outlier_flags(tmp, tmp_bytes, score, n, mode, flag, pos, head, s));
  HIP_TRY(ev.mark(7, s));
  HIP_TRY(hipMemcpyAsync(&hd, head, sizeof(hd), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // m: the capacity check needs it
  const int64_t m = hd.m;
  const bool any_kept = xyz_out || index_out;
  if (const int rc = report_m(m, cap, any_kept, outlier_cap_text, m_out)) return rc;

  if (any_kept) {
    HIP_TRY(xyz.prepare(S, 3 * (size_t)m));
    HIP_TRY(index.prepare(S, (size_t)m));
    HIP_TRY(ev.mark(8, s));
    HIP_TRY(launch_outlier_gather(d_xyz, n, flag, pos, xyz.dev(), index.dev(), s));
    HIP_TRY(ev.mark(9, s));
    HIP_TRY(xyz.download(3 * (size_t)m, s));
    HIP_TRY(index.download((size_t)m, s));
  }
  HIP_TRY(scores.copy_from(score, (size_t)n, s));  // the scores feed the later phases: always the call's own buffer
  HIP_TRY(hipStreamSynchronize(s));
  if (stats) {
    stats->n = n;
    stats->kept = m;
    stats->mean = mean;
    stats->std = sd;
    stats->threshold = thr;
  }
  double ms[5];
  HIP_TRY(ev.read(ms));
  const double phases[4] = {ms[0], ms[1], ms[2], ms[3] + ms[4]};  // the compaction: both its intervals
  std::memcpy(c->outlier_ms, phases, sizeof(phases));
  c->outlier_timed = true;
  return ICP_HIP_OK;
}

}  // namespace

extern "C" {

int icp_hip_outlier_filter(icp_hip_ctx* c, const double* xyz, int64_t n, int mode, int k, double param, int64_t cap,
                           double* xyz_out, int32_t* index_out, double* score_out, int64_t* m_out,
                           icp_outlier_stats* stats) {
  if (const int rc = outlier_args(c, xyz, n, mode, k, param, m_out)) return rc;
  if (c->group)
    return icp_hip_outlier_filter(group_member(c, 0), xyz, n, mode, k, param, cap, xyz_out, index_out, score_out, m_out,
                                  stats);
  return outlier_core(c, xyz, n, mode, k, param, cap, true, xyz_out, index_out, score_out, m_out, stats);
}

int icp_hip_outlier_filter_device(icp_hip_ctx* c, const double* d_xyz, int64_t n, int mode, int k, double param,
                                  int64_t cap, double* d_xyz_out, int32_t* d_index_out, double* d_score_out,
                                  int64_t* m_out, icp_outlier_stats* stats) {
  const char* what = "outlier_filter_device";
  if (!c || !m_out) return fail(ICP_HIP_EINVAL, "outlier_filter_device: null argument");
  *m_out = 0;
  if (const int rc = check_device_ptr(c, d_xyz, what)) return rc;
  if (const int rc = check_optional_device_ptr(c, d_xyz_out, what)) return rc;
  if (const int rc = check_optional_device_ptr(c, d_index_out, what, 4)) return rc;
  if (const int rc = check_optional_device_ptr(c, d_score_out, what)) return rc;
  if (const int rc = outlier_args(c, d_xyz, n, mode, k, param, m_out)) return rc;
  if (!c->group)
    return outlier_core(c, d_xyz, n, mode, k, param, cap, false, d_xyz_out, d_index_out, d_score_out, m_out, stats);
  // the first member, through host memory (the buffers may be another device's)
  std::vector<double> h;
  HIP_TRY(stage_down(c, &h, d_xyz, 3 * (size_t)n));
  RelayOut<double> p(d_xyz_out), sc(d_score_out, (size_t)n);
  RelayOut<int32_t> ix(d_index_out);
  const int rc = relay_count_then_fill(  // the counting call fetches the scores and the statistics too
      d_xyz_out || d_index_out, cap, outlier_cap_text, m_out, [&](bool fill, int64_t mcap, int64_t* m) {
        if (fill) p.resize(3 * (size_t)mcap), ix.resize((size_t)mcap);
        return icp_hip_outlier_filter(group_member(c, 0), h.data(), n, mode, k, param, mcap, p.host(), ix.host(),
                                      fill ? nullptr : sc.host(), m, stats);
      });
  if (rc != ICP_HIP_OK) return rc;
  return relay_up(c, p, ix, sc);
}

int icp_hip_outlier_last_timing(icp_hip_ctx* c, double ms[4]) {
  if (!c || !ms) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) c = group_member(c, 0);
  return last_timing(c->outlier_timed, c->outlier_ms, 4, "no outlier call has run on this context", ms);
}

}  // extern "C"
