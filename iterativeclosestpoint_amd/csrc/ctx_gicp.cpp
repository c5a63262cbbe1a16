// ctx_gicp.cpp — the context side of generalized ICP: the source's normals
// (estimated over a private octree of the resident source, set, read back) and the plane-to-plane
// sums of the last iterate. Beside the reference's loop: none of it changes what an iterate computes.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "icp_ctx_internal.h"
#include "octree_gpu.h"
#include "plane_solve.h"

using namespace icp;

void gicp_free_source(icp_hip_ctx* c) { dfree(c->src_normals); }

void gicp_destroy(icp_hip_ctx* c) {
  dfree(c->gicp_parts);
  c->gicp_cap = 0;
}

namespace {

// The private octree's shape: the CLI's (leaves of at most 10 points, depth at most 20). The
// normals do not depend on it: the neighbour set and the sums' order are traversal-free.
constexpr int kSrcTreeLeafPoints = 10;
constexpr int kSrcTreeMaxDepth = 20;

constexpr double kGicpEpsMin = 0x1p-20;

bool is_finite(double v) { return v - v == 0.0; }

// The checks every source-normals call shares: a single-device context without a communicator that
// holds a source.
int src_normals_check(const icp_hip_ctx* c, const char* what) {
  if (c->group)
    return fail(ICP_HIP_EINVAL, std::string(what) + ": not on a multi-device context (the source is sharded)");
  if (c->comm || c->xfn)
    return fail(ICP_HIP_EINVAL, std::string(what) + ": not on a context with a communicator (the source is sharded)");
  if (c->n_src == 0 || !c->x) return fail(ICP_HIP_ENOTREADY, "source not set");
  return ICP_HIP_OK;
}

void keep_src_normals(icp_hip_ctx* c, DevScratch& S, double* slot) {
  dfree(c->src_normals);
  c->src_normals = S.keep(slot);
  c->src_normals_moves = c->src_moves;
}

// The caller's normals (device buffer, caller's source order) into the context, slot order; the
// context's normals are replaced only when every row is of unit length or zero.
int set_src_normals_core(icp_hip_ctx* c, const double* d_aos) {
  unsigned h_bad = 0;  // before its source's owner: outlives the copy
  DevScratch S;
  double* slot = nullptr;
  unsigned* bad = nullptr;
  HIP_TRY(S.alloc(&slot, 3 * (size_t)c->n_src));
  HIP_TRY(S.alloc(&bad, 1));
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(unsigned), c->stream));
  HIP_TRY(launch_src_normals_to_slot(c->perm, d_aos, slot, c->n_src, bad, c->stream));
  HIP_TRY(hipMemcpyAsync(&h_bad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (h_bad != 0)
    return fail(ICP_HIP_EINVAL, "set_source_normals: " + std::to_string(h_bad) + " rows are neither of unit length nor zero");
  keep_src_normals(c, S, slot);
  return ICP_HIP_OK;
}

// icp_hip_gicp_sums (thr null: the device record's threshold) and icp_hip_gicp_sums_at.
int gicp_sums_core(icp_hip_ctx* c, const double origin[3], const double R[9], double eps, const double* thr,
                   icp_gicp_sums* out) {
  if (!c || !origin || !R || !out) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return fail(ICP_HIP_EINVAL, "gicp_sums: not on a multi-device context (the sums are not exchanged)");
  if (c->comm || c->xfn) return fail(ICP_HIP_EINVAL, "gicp_sums: not on a context with a communicator (the sums are not exchanged)");
  for (int a = 0; a < 3; a++)
    if (!is_finite(origin[a])) return fail(ICP_HIP_EINVAL, "gicp_sums: non-finite origin");
  for (int a = 0; a < 9; a++)
    if (!is_finite(R[a])) return fail(ICP_HIP_EINVAL, "gicp_sums: non-finite entry of R_src");
  for (int p = 0; p < 3; p++)
    for (int q = 0; q < 3; q++) {
      const double v = (R[3 * p] * R[3 * q] + R[3 * p + 1] * R[3 * q + 1]) + R[3 * p + 2] * R[3 * q + 2];
      if (!(std::fabs(v - (p == q ? 1.0 : 0.0)) <= 1e-9)) return fail(ICP_HIP_EINVAL, "gicp_sums: R_src is not orthonormal");
    }
  if (!(eps >= kGicpEpsMin && eps <= 1.0)) return fail(ICP_HIP_EINVAL, "gicp_sums: epsilon outside [2^-20, 1]");
  if (thr && *thr != *thr) return fail(ICP_HIP_EINVAL, "gicp_sums_at: the threshold is NaN");
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if (!c->normals) return fail(ICP_HIP_ENOTREADY, "the target has no normals");
  if (!c->src_normals) return fail(ICP_HIP_ENOTREADY, "the source has no normals");
  if (!c->have_results) return fail(ICP_HIP_ENOTREADY, "no iteration has run on this source");
  HIP_TRY(hipSetDevice(c->device));
  const int64_t nparts = gicp_num_parts(c->n_src);
  if (!c->gicp_parts || c->gicp_cap < nparts) {
    dfree(c->gicp_parts);
    c->gicp_cap = 0;
    HIP_TRY(dalloc(&c->gicp_parts, (size_t)(nparts + 1) * kGicpSums));
    c->gicp_cap = nparts;
  }
  GicpLaunch a;
  a.x = c->x;
  a.y = c->y;
  a.z = c->z;
  a.pos = c->pos;
  a.dist = c->dist;
  a.pts = c->pts;
  a.normals = c->normals;
  a.src_normals = c->src_normals;
  a.it = c->it;
  for (int k = 0; k < 3; k++) a.origin[k] = origin[k];
  for (int k = 0; k < 9; k++) a.R[k] = R[k];
  a.f = 1.0 - eps;
  a.n = c->n_src;
  a.parts = c->gicp_parts;
  a.out = c->gicp_parts + (size_t)c->gicp_cap * kGicpSums;
  a.thr = thr ? *thr : 0.0;
  double h[kGicpSums];
  HIP_TRY(thr ? launch_gicp_sums_at(a, c->stream) : launch_gicp_sums(a, c->stream));
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
  out->n_iso_src = (int64_t)h[29];
  out->n_iso_tgt = (int64_t)h[30];
  for (int k = 0; k < 3; k++) out->origin[k] = origin[k];
  out->epsilon = eps;
  return ICP_HIP_OK;
}

}  // namespace

extern "C" {

int icp_hip_estimate_source_normals(icp_hip_ctx* c, int k, const double* viewpoint) {
  if (!c) return fail(ICP_HIP_EINVAL, "null context");
  if (const int rc = src_normals_check(c, "estimate_source_normals")) return rc;
  if (k < 3 || k > ICP_HIP_KNN_MAX) return fail(ICP_HIP_EINVAL, "estimate_source_normals: k out of range [3, 32]");
  if ((int64_t)k > c->n_src) return fail(ICP_HIP_EINVAL, "estimate_source_normals: k exceeds the source size");
  if (viewpoint)
    for (int a = 0; a < 3; a++)
      if (!is_finite(viewpoint[a])) return fail(ICP_HIP_EINVAL, "estimate_source_normals: non-finite viewpoint");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int64_t n = c->n_src;
  unsigned h_bad = 0;  // before its source's owner: outlives the copy
  ScopedOctree oct;
  DevScratch S;
  double *aos = nullptr, *leaf = nullptr, *slot = nullptr;
  unsigned* bad = nullptr;
  HIP_TRY(S.alloc(&aos, 3 * (size_t)n));
  HIP_TRY(S.alloc(&bad, 1));
  // the resident source in the caller's order: the neighbours' tie rule is the caller's index
  HIP_TRY(launch_scatter_aos(c->perm, c->x, c->y, c->z, aos, n, s));
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(unsigned), s));
  HIP_TRY(launch_count_nonfinite(aos, n, bad, s));
  HIP_TRY(hipMemcpyAsync(&h_bad, bad, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h_bad != 0)
    return fail(ICP_HIP_EINVAL, "estimate_source_normals: " + std::to_string(h_bad) +
                                    " source points have a non-finite coordinate (icp_hip_set_source_normals takes normals for such a source)");
  {
    std::string why;
    if (const int rc = gpu_build_octree(aos, n, kSrcTreeLeafPoints, kSrcTreeMaxDepth, s, &oct.t, &why))
      return fail_octree_build(rc, why);
  }
  const int levels = oct.t.max_inner_depth + 1 > 0 ? oct.t.max_inner_depth + 1 : 1;
  HIP_TRY(S.alloc(&leaf, 3 * (size_t)n));
  HIP_TRY(S.alloc(&slot, 3 * (size_t)n));
  HIP_TRY(launch_target_normals(oct.t.nodes, oct.t.pts, levels, n, k, viewpoint ? 1 : 0, viewpoint, leaf, s));
  // the private tree's leaf order -> the caller's order (over the coordinates' copy) -> slot order
  HIP_TRY(launch_normals_from_leaf(oct.t.pts, leaf, aos, n, s));
  HIP_TRY(launch_src_normals_to_slot(c->perm, aos, slot, n, nullptr, s));
  HIP_TRY(hipStreamSynchronize(s));
  keep_src_normals(c, S, slot);
  return ICP_HIP_OK;
}

int icp_hip_set_source_normals(icp_hip_ctx* c, const double* n_xyz) {
  if (!c || !n_xyz) return fail(ICP_HIP_EINVAL, "null argument");
  if (const int rc = src_normals_check(c, "set_source_normals")) return rc;
  HIP_TRY(hipSetDevice(c->device));
  DevScratch S;
  double* up = nullptr;
  HIP_TRY(call_upload(S, &up, n_xyz, 3 * (size_t)c->n_src, c->stream));
  return set_src_normals_core(c, up);
}

int icp_hip_set_source_normals_device(icp_hip_ctx* c, const double* d_n_xyz) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  if (const int rc = check_device_ptr(c, d_n_xyz, "set_source_normals_device")) return rc;
  if (const int rc = src_normals_check(c, "set_source_normals_device")) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return set_src_normals_core(c, d_n_xyz);
}

int icp_hip_get_source_normals(icp_hip_ctx* c, double* n_xyz_out) {
  if (!c || !n_xyz_out) return fail(ICP_HIP_EINVAL, "null argument");
  if (const int rc = src_normals_check(c, "get_source_normals")) return rc;
  if (!c->src_normals) return fail(ICP_HIP_ENOTREADY, "the source has no normals");
  HIP_TRY(hipSetDevice(c->device));
  DevScratch S;
  double* aos = nullptr;
  HIP_TRY(S.alloc(&aos, 3 * (size_t)c->n_src));
  HIP_TRY(launch_src_normals_from_slot(c->perm, c->src_normals, aos, c->n_src, c->stream));
  HIP_TRY(hipMemcpyAsync(n_xyz_out, aos, 3 * sizeof(double) * c->n_src, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

int icp_hip_get_source_normals_device(icp_hip_ctx* c, double* d_n_xyz_out) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  if (const int rc = check_device_ptr(c, d_n_xyz_out, "get_source_normals_device")) return rc;
  if (const int rc = src_normals_check(c, "get_source_normals_device")) return rc;
  if (!c->src_normals) return fail(ICP_HIP_ENOTREADY, "the source has no normals");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_src_normals_from_slot(c->perm, c->src_normals, d_n_xyz_out, c->n_src, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

int icp_hip_gicp_sums(icp_hip_ctx* c, const double origin[3], const double R_src[9], double epsilon,
                      icp_gicp_sums* out) {
  return gicp_sums_core(c, origin, R_src, epsilon, nullptr, out);
}

int icp_hip_gicp_sums_at(icp_hip_ctx* c, const double origin[3], const double R_src[9], double epsilon,
                         double threshold, icp_gicp_sums* out) {
  return gicp_sums_core(c, origin, R_src, epsilon, &threshold, out);
}

void icp_gicp_solve(const icp_gicp_sums* sums, double T[16], int32_t* ok) {
  if (ok) *ok = 0;
  if (!sums) return;
  icp_plane_sums p;
  std::memset(&p, 0, sizeof(p));
  std::memcpy(p.A, sums->A, sizeof(p.A));
  std::memcpy(p.g, sums->g, sizeof(p.g));
  p.sum_r2 = sums->sum_r2;
  p.n = sums->n;
  std::memcpy(p.origin, sums->origin, sizeof(p.origin));
  icp::plane_solve(&p, T, ok);
}

int icp_hip_set_gicp_epsilon(icp_hip_ctx* c, double epsilon) {
  if (!c) return fail(ICP_HIP_EINVAL, "null context");
  if (!(epsilon >= kGicpEpsMin && epsilon <= 1.0)) return fail(ICP_HIP_EINVAL, "set_gicp_epsilon: epsilon outside [2^-20, 1]");
  if (c->group) return fail(ICP_HIP_EINVAL, "set_gicp_epsilon: not on a multi-device context");
  c->gicp_epsilon = epsilon;
  return ICP_HIP_OK;
}

}  // extern "C"
