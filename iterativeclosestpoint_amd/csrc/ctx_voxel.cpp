// ctx_voxel.cpp — the context side of voxel-grid down-sampling: the argument
// checks, the call's scratch, the five phases of voxel_kernels.hip on the context's stream with the
// two small read-backs between them, and the host, device and group forms around that core
// (§3.8). It reads no target or source of the context and changes none.
#include <cstring>
#include <string>
#include <vector>

#include "icp_ctx_internal.h"
#include "phase_events.h"
#include "voxel_host.h"

using namespace icp;

namespace {

// The call after the pointer checks, in its host form (to_host: the cloud is uploaded, the outputs
// get the first m entries of scratch buffers) or on the caller's device buffers.
int voxel_core(icp_hip_ctx* c, const double* xyz_in, int64_t n, double h, const double* origin, int mode, int64_t cap,
               bool to_host, double* xyz_out, int32_t* first_out, int32_t* count_out, int64_t* m_out,
               double origin_out[3]) {
  VoxelHead hd;  // before the scratch: outlives the copies into it
  std::memset(&hd, 0, sizeof(hd));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  PhaseEvents<5> ev;  // bounds, keys, sort, runs, reduce
  DevScratch S;
  double* up = nullptr;
  if (to_host) HIP_TRY(call_upload(S, &up, xyz_in, 3 * (size_t)n, s));
  const double* d_xyz = to_host ? up : xyz_in;
  CallOut<double> xyz(xyz_out, to_host);
  CallOut<int32_t> first(first_out, to_host), count(count_out, to_host);
  VoxelHead* head = nullptr;
  double* parts = nullptr;
  uint64_t *keys = nullptr, *keys_sorted = nullptr;
  int32_t *idx = nullptr, *idx_sorted = nullptr;
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  HIP_TRY(voxel_temp_bytes(n, &tmp_bytes));
  HIP_TRY(S.alloc(&head, 1));
  HIP_TRY(S.alloc(&parts, 4 * (size_t)voxel_bounds_parts(n)));
  HIP_TRY(S.alloc(&keys, (size_t)n));
  HIP_TRY(S.alloc(&keys_sorted, (size_t)n));
  HIP_TRY(S.alloc(&idx, (size_t)n + 1));  // later the run starts (n + 1 entries)
  HIP_TRY(S.alloc(&idx_sorted, (size_t)n));
  HIP_TRY(S.alloc(&tmp, tmp_bytes));

  HIP_TRY(ev.mark(0, s));
  HIP_TRY(launch_voxel_bounds(d_xyz, n, origin, parts, head, s));
  HIP_TRY(ev.mark(1, s));
  HIP_TRY(ev.mark(2, s));
  HIP_TRY(launch_voxel_keys(d_xyz, n, h, head, keys, idx, s));
  HIP_TRY(ev.mark(3, s));
  HIP_TRY(hipMemcpyAsync(&hd, head, sizeof(hd), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // the one read of the flags, before the sort
  if (hd.n_bad) return fail(ICP_HIP_EINVAL, voxel_nonfinite_text(hd.n_bad));
  if (hd.flags) return fail(ICP_HIP_EINVAL, voxel_range_text(hd.flags));
  if (origin_out)
    for (int a = 0; a < 3; a++) origin_out[a] = hd.origin[a];

  HIP_TRY(ev.mark(4, s));
  HIP_TRY(launch_voxel_sort(tmp, tmp_bytes, keys, keys_sorted, idx, idx_sorted, n, hd.max_key, s));
  HIP_TRY(ev.mark(5, s));
  // the unsorted keys and the identity are spent: their buffers hold the flags, their sum, the starts
  int32_t* flag = reinterpret_cast<int32_t*>(keys);
  int32_t* pos = flag + n;
  int32_t* starts = idx;
  HIP_TRY(ev.mark(6, s));
  HIP_TRY(launch_voxel_runs(tmp, tmp_bytes, keys_sorted, n, flag, pos, starts, head, s));
  HIP_TRY(ev.mark(7, s));
  HIP_TRY(hipMemcpyAsync(&hd, head, sizeof(hd), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // m: the capacity check needs it
  const int64_t m = hd.m;
  const bool any_out = xyz_out || first_out || count_out;
  if (const int rc = report_m(m, cap, any_out, voxel_cap_text, m_out)) return rc;

  if (any_out) {
    HIP_TRY(xyz.prepare(S, 3 * (size_t)m));
    HIP_TRY(first.prepare(S, (size_t)m));
    HIP_TRY(count.prepare(S, (size_t)m));
    HIP_TRY(ev.mark(8, s));
    HIP_TRY(launch_voxel_reduce(d_xyz, idx_sorted, starts, head, m, mode, xyz.dev(), first.dev(), count.dev(), s));
    HIP_TRY(ev.mark(9, s));
    HIP_TRY(xyz.download(3 * (size_t)m, s));
    HIP_TRY(first.download((size_t)m, s));
    HIP_TRY(count.download((size_t)m, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  HIP_TRY(ev.read(c->voxel_ms));
  c->voxel_timed = true;
  return ICP_HIP_OK;
}

int voxel_args(icp_hip_ctx* c, const double* xyz, int64_t n, double h, const double* origin, int mode, int64_t* m_out) {
  if (!c || !m_out) return fail(ICP_HIP_EINVAL, "voxel_downsample: null argument");
  *m_out = 0;
  std::string why;
  if (const int rc = voxel_check_args(n, h, origin, mode, &why)) return fail(rc, why);
  if (!xyz) return fail(ICP_HIP_EINVAL, "voxel_downsample: null cloud");
  return ICP_HIP_OK;
}

}  // namespace

extern "C" {

int icp_hip_voxel_downsample(icp_hip_ctx* c, const double* xyz, int64_t n, double voxel, const double* origin, int mode,
                             int64_t cap, double* xyz_out, int32_t* first_out, int32_t* count_out, int64_t* m_out,
                             double origin_out[3]) {
  if (const int rc = voxel_args(c, xyz, n, voxel, origin, mode, m_out)) return rc;
  if (c->group)
    return icp_hip_voxel_downsample(group_member(c, 0), xyz, n, voxel, origin, mode, cap, xyz_out, first_out, count_out,
                                    m_out, origin_out);
  return voxel_core(c, xyz, n, voxel, origin, mode, cap, true, xyz_out, first_out, count_out, m_out, origin_out);
}

int icp_hip_voxel_downsample_device(icp_hip_ctx* c, const double* d_xyz, int64_t n, double voxel, const double* origin,
                                    int mode, int64_t cap, double* d_xyz_out, int32_t* d_first_out, int32_t* d_count_out,
                                    int64_t* m_out, double origin_out[3]) {
  const char* what = "voxel_downsample_device";
  if (!c || !m_out) return fail(ICP_HIP_EINVAL, "voxel_downsample_device: null argument");
  *m_out = 0;
  if (const int rc = check_device_ptr(c, d_xyz, what)) return rc;
  if (const int rc = check_optional_device_ptr(c, d_xyz_out, what)) return rc;
  if (const int rc = check_optional_device_ptr(c, d_first_out, what, 4)) return rc;
  if (const int rc = check_optional_device_ptr(c, d_count_out, what, 4)) return rc;
  if (const int rc = voxel_args(c, d_xyz, n, voxel, origin, mode, m_out)) return rc;
  if (!c->group)
    return voxel_core(c, d_xyz, n, voxel, origin, mode, cap, false, d_xyz_out, d_first_out, d_count_out, m_out, origin_out);
  // the first member, through host memory (the buffers may be another device's)
  std::vector<double> h;
  HIP_TRY(stage_down(c, &h, d_xyz, 3 * (size_t)n));
  RelayOut<double> p(d_xyz_out);
  RelayOut<int32_t> f(d_first_out), k(d_count_out);
  const int rc = relay_count_then_fill(
      d_xyz_out || d_first_out || d_count_out, cap, voxel_cap_text, m_out, [&](bool fill, int64_t mcap, int64_t* m) {
        if (fill) p.resize(3 * (size_t)mcap), f.resize((size_t)mcap), k.resize((size_t)mcap);
        return icp_hip_voxel_downsample(group_member(c, 0), h.data(), n, voxel, origin, mode, mcap, p.host(), f.host(),
                                        k.host(), m, origin_out);
      });
  if (rc != ICP_HIP_OK) return rc;
  return relay_up(c, p, f, k);
}

int icp_hip_voxel_last_timing(icp_hip_ctx* c, double ms[5]) {
  if (!c || !ms) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) c = group_member(c, 0);
  return last_timing(c->voxel_timed, c->voxel_ms, 5, "no voxel call has run on this context", ms);
}

}  // extern "C"
