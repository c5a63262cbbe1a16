// ctx_plane.cpp — the context side of point-to-plane ICP: the k-nearest-neighbour
// query over the resident octree, the target's normals (estimated, set, read back) and the plane
// sums of the last iterate. Beside the reference's loop: none of it changes what an iterate computes.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "icp_ctx_internal.h"
#include "plane_solve.h"

using namespace icp;

void plane_free_target(icp_hip_ctx* c) {
  dfree(c->normals);
  dfree(c->plane_parts);
  c->plane_cap = 0;
}

namespace {

// Queries per launch of the k-NN calls: bounds the scratch of the host variant (n x k outputs).
constexpr int64_t kKnnSlice = (int64_t)1 << 22;

int knn_k_check(int k) {
  return k < 1 || k > ICP_HIP_KNN_MAX ? fail(ICP_HIP_EINVAL, "knn: k out of range [1, 32]") : ICP_HIP_OK;
}

int knn_check(const icp_hip_ctx* c, int k) {
  if (const int rc = knn_k_check(k)) return rc;
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if ((int64_t)k > c->n_tgt) return fail(ICP_HIP_EINVAL, "knn: k exceeds the target size");
  return ICP_HIP_OK;
}

// knn after the argument checks. to_host: q and the outputs are host buffers, a slice at a time
// through the scratch; otherwise they are the caller's device buffers.
int knn_core(icp_hip_ctx* c, bool to_host, const double* q, int64_t n, int k, int32_t* idx_out, double* d2_out) {
  HIP_TRY(hipSetDevice(c->device));
  const int64_t cap = std::min(n, kKnnSlice);
  DevScratch S;
  CallOut<int32_t> idx(idx_out, to_host);
  CallOut<double> d2(d2_out, to_host);
  double* up = nullptr;
  if (to_host) HIP_TRY(S.alloc(&up, 3 * (size_t)cap));
  HIP_TRY(idx.prepare(S, (size_t)cap * k));
  HIP_TRY(d2.prepare(S, (size_t)cap * k));
  for (int64_t off = 0; off < n; off += kKnnSlice) {
    const int64_t m = std::min(n - off, kKnnSlice);
    if (to_host) HIP_TRY(hipMemcpyAsync(up, q + 3 * off, 3 * sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_knn(c->nodes, c->pts, c->levels, to_host ? up : q + 3 * off, m, k, idx.dev((size_t)off * k),
                       d2.dev((size_t)off * k), c->stream));
    HIP_TRY(idx.download((size_t)m * k, c->stream, (size_t)off * k));
    HIP_TRY(d2.download((size_t)m * k, c->stream, (size_t)off * k));
    // the host form's scratch is the next slice's too; the device form waits once, for all slices
    if (to_host || off + m == n) HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return ICP_HIP_OK;
}

// The caller's normals (device buffer, caller's target order) into the context, leaf order; the
// context's normals are replaced only when every row is of unit length or zero.
int set_normals_core(icp_hip_ctx* c, const double* d_aos) {
  unsigned h_bad = 0;  // before its source's owner: outlives the copy
  DevScratch S;
  double* leaf = nullptr;
  unsigned* bad = nullptr;
  HIP_TRY(S.alloc(&leaf, 3 * (size_t)c->n_tgt));
  HIP_TRY(S.alloc(&bad, 1));
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(unsigned), c->stream));
  HIP_TRY(launch_normals_to_leaf(c->pts, d_aos, leaf, c->n_tgt, bad, c->stream));
  HIP_TRY(hipMemcpyAsync(&h_bad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (h_bad != 0)
    return fail(ICP_HIP_EINVAL, "set_target_normals: " + std::to_string(h_bad) + " rows are neither of unit length nor zero");
  dfree(c->normals);
  c->normals = S.keep(leaf);
  return ICP_HIP_OK;
}

}  // namespace

extern "C" {

int icp_hip_knn(icp_hip_ctx* c, const double* q, int64_t n, int k, int32_t* idx_out, double* d2_out) {
  if (!c || n < 0 || (n > 0 && !q)) return fail(ICP_HIP_EINVAL, "bad arguments");
  if (c->group) return icp_hip_knn(group_member(c, 0), q, n, k, idx_out, d2_out);  // the replicated octree
  if (const int rc = knn_check(c, k)) return rc;
  if (n == 0 || (!idx_out && !d2_out)) return ICP_HIP_OK;
  return knn_core(c, true, q, n, k, idx_out, d2_out);
}

int icp_hip_knn_device(icp_hip_ctx* c, const double* d_q, int64_t n, int k, int32_t* d_idx_out, double* d_d2_out) {
  if (!c || n < 0) return fail(ICP_HIP_EINVAL, "bad arguments");
  if (const int rc = check_device_ptr(c, d_q, "knn_device")) return rc;
  if (const int rc = check_optional_device_ptr(c, d_idx_out, "knn_device", 4)) return rc;
  if (const int rc = check_optional_device_ptr(c, d_d2_out, "knn_device")) return rc;
  if (c->group) {  // the first member's replica, through host memory (the buffers may be another device's)
    if (const int rc = knn_k_check(k)) return rc;
    std::vector<double> hq;
    RelayOut<int32_t> idx(d_idx_out, (size_t)n * k);
    RelayOut<double> d(d_d2_out, (size_t)n * k);
    HIP_TRY(stage_down(c, &hq, d_q, 3 * (size_t)n));
    if (const int rc = icp_hip_knn(group_member(c, 0), hq.data(), n, k, idx.host(), d.host())) return rc;
    return relay_up(c, idx, d);
  }
  if (const int rc = knn_check(c, k)) return rc;
  if (n == 0 || (!d_idx_out && !d_d2_out)) return ICP_HIP_OK;
  return knn_core(c, false, d_q, n, k, d_idx_out, d_d2_out);
}

int icp_hip_estimate_target_normals(icp_hip_ctx* c, int k, const double* viewpoint) {
  if (!c) return fail(ICP_HIP_EINVAL, "null context");
  if (c->group) return icp_hip_estimate_target_normals(group_member(c, 0), k, viewpoint);
  if (k < 3 || k > ICP_HIP_KNN_MAX) return fail(ICP_HIP_EINVAL, "estimate_target_normals: k out of range [3, 32]");
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if ((int64_t)k > c->n_tgt) return fail(ICP_HIP_EINVAL, "estimate_target_normals: k exceeds the target size");
  if (viewpoint)
    for (int a = 0; a < 3; a++)
      if (!(viewpoint[a] - viewpoint[a] == 0.0)) return fail(ICP_HIP_EINVAL, "estimate_target_normals: non-finite viewpoint");
  HIP_TRY(hipSetDevice(c->device));
  DevScratch S;
  double* leaf = nullptr;
  HIP_TRY(S.alloc(&leaf, 3 * (size_t)c->n_tgt));
  HIP_TRY(launch_target_normals(c->nodes, c->pts, c->levels, c->n_tgt, k, viewpoint ? 1 : 0, viewpoint, leaf, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  dfree(c->normals);
  c->normals = S.keep(leaf);
  return ICP_HIP_OK;
}

int icp_hip_set_target_normals(icp_hip_ctx* c, const double* n_xyz) {
  if (!c || !n_xyz) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return icp_hip_set_target_normals(group_member(c, 0), n_xyz);
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  HIP_TRY(hipSetDevice(c->device));
  DevScratch S;
  double* up = nullptr;
  HIP_TRY(call_upload(S, &up, n_xyz, 3 * (size_t)c->n_tgt, c->stream));
  return set_normals_core(c, up);
}

int icp_hip_set_target_normals_device(icp_hip_ctx* c, const double* d_n_xyz) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  if (const int rc = check_device_ptr(c, d_n_xyz, "set_target_normals_device")) return rc;
  if (c->group) {
    icp_hip_ctx* m = group_member(c, 0);
    if (!m->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
    std::vector<double> h;
    HIP_TRY(stage_down(c, &h, d_n_xyz, 3 * (size_t)m->n_tgt));
    return icp_hip_set_target_normals(m, h.data());
  }
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  HIP_TRY(hipSetDevice(c->device));
  return set_normals_core(c, d_n_xyz);
}

int icp_hip_get_target_normals(icp_hip_ctx* c, double* n_xyz_out) {
  if (!c || !n_xyz_out) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return icp_hip_get_target_normals(group_member(c, 0), n_xyz_out);
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if (!c->normals) return fail(ICP_HIP_ENOTREADY, "the target has no normals");
  HIP_TRY(hipSetDevice(c->device));
  DevScratch S;
  double* aos = nullptr;
  HIP_TRY(S.alloc(&aos, 3 * (size_t)c->n_tgt));
  HIP_TRY(launch_normals_from_leaf(c->pts, c->normals, aos, c->n_tgt, c->stream));
  HIP_TRY(hipMemcpyAsync(n_xyz_out, aos, 3 * sizeof(double) * c->n_tgt, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

int icp_hip_get_target_normals_device(icp_hip_ctx* c, double* d_n_xyz_out) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  if (const int rc = check_device_ptr(c, d_n_xyz_out, "get_target_normals_device")) return rc;
  if (c->group) {
    icp_hip_ctx* m = group_member(c, 0);
    std::vector<double> h(3 * (size_t)m->n_tgt);
    const int rc = icp_hip_get_target_normals(m, h.data());
    if (rc != ICP_HIP_OK) return rc;
    HIP_TRY(stage_up(c, d_n_xyz_out, h));
    return ICP_HIP_OK;
  }
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if (!c->normals) return fail(ICP_HIP_ENOTREADY, "the target has no normals");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_normals_from_leaf(c->pts, c->normals, d_n_xyz_out, c->n_tgt, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

// icp_hip_plane_sums (thr null: the device record's threshold) and icp_hip_plane_sums_at.
static int plane_sums_core(icp_hip_ctx* c, const double origin[3], const double* thr, icp_plane_sums* out) {
  if (!c || !origin || !out) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return fail(ICP_HIP_EINVAL, "plane_sums: not on a multi-device context (the sums are not exchanged)");
  if (c->comm || c->xfn) return fail(ICP_HIP_EINVAL, "plane_sums: not on a context with a communicator (the sums are not exchanged)");
  for (int a = 0; a < 3; a++)
    if (!(origin[a] - origin[a] == 0.0)) return fail(ICP_HIP_EINVAL, "plane_sums: non-finite origin");
  if (thr && *thr != *thr) return fail(ICP_HIP_EINVAL, "plane_sums_at: the threshold is NaN");
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if (!c->normals) return fail(ICP_HIP_ENOTREADY, "the target has no normals");
  if (!c->have_results) return fail(ICP_HIP_ENOTREADY, "no iteration has run on this source");
  HIP_TRY(hipSetDevice(c->device));
  const int64_t nparts = plane_num_parts(c->n_src);
  if (!c->plane_parts || c->plane_cap < nparts) {
    dfree(c->plane_parts);
    c->plane_cap = 0;
    HIP_TRY(dalloc(&c->plane_parts, (size_t)(nparts + 1) * kPlaneSums));
    c->plane_cap = nparts;
  }
  PlaneLaunch a;
  a.x = c->x;
  a.y = c->y;
  a.z = c->z;
  a.pos = c->pos;
  a.dist = c->dist;
  a.pts = c->pts;
  a.normals = c->normals;
  a.it = c->it;
  for (int k = 0; k < 3; k++) a.origin[k] = origin[k];
  a.n = c->n_src;
  a.parts = c->plane_parts;
  a.out = c->plane_parts + (size_t)c->plane_cap * kPlaneSums;
  a.thr = thr ? *thr : 0.0;
  double h[kPlaneSums];
  HIP_TRY(thr ? launch_plane_sums_at(a, c->stream) : launch_plane_sums(a, c->stream));
  HIP_TRY(hipMemcpyAsync(h, a.out, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // the call's one host wait
  std::memset(out, 0, sizeof(*out));
  int m = 0;
  for (int p = 0; p < 6; p++)
    for (int q = p; q < 6; q++) {
      out->A[6 * p + q] = h[m];
      out->A[6 * q + p] = h[m];
      m++;
    }
  for (int p = 0; p < 6; p++) out->g[p] = h[21 + p];
  out->sum_r2 = h[27];
  out->n = (int64_t)h[28];
  out->n_skipped = (int64_t)h[29];
  for (int k = 0; k < 3; k++) out->origin[k] = origin[k];
  return ICP_HIP_OK;
}

int icp_hip_plane_sums(icp_hip_ctx* c, const double origin[3], icp_plane_sums* out) {
  return plane_sums_core(c, origin, nullptr, out);
}

int icp_hip_plane_sums_at(icp_hip_ctx* c, const double origin[3], double threshold, icp_plane_sums* out) {
  return plane_sums_core(c, origin, &threshold, out);
}

void icp_plane_solve(const icp_plane_sums* sums, double T[16], int32_t* ok) { icp::plane_solve(sums, T, ok); }

}  // extern "C"
