// ctx_reject.cpp — the context side of the correspondence rejectors: the rank
// select over the last iterate's residuals and the pair sums at a caller's threshold. Beside the
// reference's loop: none of it changes what an iterate computes or left resident.
#include <cmath>
#include <cstring>
#include <string>

#include "icp_ctx_internal.h"

using namespace icp;

void reject_destroy(icp_hip_ctx* c) {
  if (c->select_buf) (void)hipFree(c->select_buf);
  c->select_buf = nullptr;
  dfree(c->pair_parts);
  c->pair_cap = 0;
}

namespace {

// What the three calls refuse alike, as icp_hip_plane_sums does (before any kernel runs).
int reject_check(const icp_hip_ctx* c, const char* what) {
  const std::string w(what);
  if (c->group) return fail(ICP_HIP_EINVAL, w + ": not on a multi-device context (the residuals are not exchanged)");
  if (c->comm || c->xfn)
    return fail(ICP_HIP_EINVAL, w + ": not on a context with a communicator (the residuals are not exchanged)");
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if (!c->have_results) return fail(ICP_HIP_ENOTREADY, "no iteration has run on this source");
  return ICP_HIP_OK;
}

}  // namespace

extern "C" {

int icp_hip_residual_select(icp_hip_ctx* c, double fraction, int64_t rank, icp_select_result* out) {
  if (!c || !out) return fail(ICP_HIP_EINVAL, "null argument");
  std::memset(out, 0, sizeof(*out));
  if (rank < 0) return fail(ICP_HIP_EINVAL, "residual_select: negative rank");
  if (rank == 0 && !(fraction > 0.0 && fraction <= 1.0))
    return fail(ICP_HIP_EINVAL, "residual_select: the fraction is not in (0, 1]");
  if (const int rc = reject_check(c, "residual_select")) return rc;
  if (c->n_src == 0) return fail(ICP_HIP_EINVAL, "residual_select: no finite residual");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->select_buf) HIP_TRY(hipMalloc(&c->select_buf, select_scratch_bytes()));
  SelectState h;
  HIP_TRY(launch_residual_select(c->dist, c->n_src, fraction, rank, c->select_buf, c->stream));
  HIP_TRY(hipMemcpyAsync(&h, select_result(c->select_buf), sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // the call's one host wait
  out->n_finite = (int64_t)h.n_finite;
  if (h.status == kSelectEmpty) return fail(ICP_HIP_EINVAL, "residual_select: no finite residual");
  if (h.status == kSelectRange)
    return fail(ICP_HIP_EINVAL, "residual_select: rank " + std::to_string(h.rank) + " exceeds the " +
                                    std::to_string(h.n_finite) + " finite residuals");
  std::memcpy(&out->value, &h.key, sizeof(double));
  out->rank = (int64_t)h.rank;
  out->n_less = (int64_t)h.n_less;
  out->n_equal = (int64_t)h.n_equal;
  return ICP_HIP_OK;
}

int icp_hip_pair_sums(icp_hip_ctx* c, double threshold, icp_pair_sums* out) {
  if (!c || !out) return fail(ICP_HIP_EINVAL, "null argument");
  if (threshold != threshold) return fail(ICP_HIP_EINVAL, "pair_sums: the threshold is NaN");
  if (const int rc = reject_check(c, "pair_sums")) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const int64_t nparts = pair_num_parts(c->n_src);
  // the parts, the merged record (kPairRec + 1 doubles) and the first-pair word behind them
  constexpr size_t kTail = kPairRec + 2;
  if (!c->pair_parts || c->pair_cap < nparts) {
    dfree(c->pair_parts);
    c->pair_cap = 0;
    HIP_TRY(dalloc(&c->pair_parts, (size_t)nparts * kPairRec + kTail));
    c->pair_cap = nparts;
  }
  PairLaunch a;
  a.x = c->x;
  a.y = c->y;
  a.z = c->z;
  a.pos = c->pos;
  a.dist = c->dist;
  a.pts = c->pts;
  a.thr = threshold;
  a.n = c->n_src;
  a.parts = c->pair_parts;
  a.out = c->pair_parts + (size_t)c->pair_cap * kPairRec;
  a.first = reinterpret_cast<unsigned*>(a.out + kPairRec + 1);
  double h[kPairRec + 1];
  HIP_TRY(launch_pair_sums(a, c->stream));
  HIP_TRY(hipMemcpyAsync(h, a.out, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // the call's one host wait
  std::memset(out, 0, sizeof(*out));
  out->threshold = threshold;
  out->n_finite = (int64_t)h[kPairRec];
  out->valid = (int64_t)h[0];
  out->sum_d2 = h[1];
  out->rmse = out->valid > 0 ? std::sqrt(h[1] / h[0]) : 0.0;  // icpengine.cpp:274-278
  for (int k = 0; k < 3; k++) {
    out->centroid_src[k] = h[2 + k];
    out->centroid_tgt[k] = h[5 + k];
  }
  for (int k = 0; k < 9; k++) out->H[k] = h[8 + k];
  return ICP_HIP_OK;
}

}  // extern "C"
