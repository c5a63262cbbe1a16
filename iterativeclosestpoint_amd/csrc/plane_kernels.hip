// plane_kernels.hip — the point-to-plane normal equations of an iterate's valid pairs (DESIGN.md
// §3.9), fp64, no FMA. A call of its own after the iterate: it reads the moved source, the matches,
// the residuals, the device record's threshold (or the caller's: launch_plane_sums_at), the target
// points and the normals at the matches, and writes none of them.
//  k_plane_sums   fixed parts of 4096 queries (as k_moments): thread t of a part adds its queries
//                 t + 256 j (j < 16) in order, then the block's fixed tree (block_sum).
//  k_plane_merge  the parts added in index order, one thread per sum.
// The bits depend neither on the run nor on which search path settled which query.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "nn_device.h"

namespace icp {
namespace {
using namespace dev;

constexpr int kPlanePart = 4096;
constexpr int kPlaneBlock = 256;

// AT: the caller's threshold (a.thr) and only finite residuals, instead of the device record's.
template <bool AT>
__global__ void __launch_bounds__(kPlaneBlock) k_plane_sums(PlaneLaunch a) {
  __shared__ double red[(kPlaneBlock / kWave) * kPlaneSums];
  const int64_t base = (int64_t)blockIdx.x * kPlanePart;
  const double thr = AT ? a.thr : a.it->thr;
  const double ox = a.origin[0], oy = a.origin[1], oz = a.origin[2];
  double v[kPlaneSums];
#pragma unroll
  for (int k = 0; k < kPlaneSums; k++) v[k] = 0.0;
  for (int j = 0; j < kPlanePart / kPlaneBlock; j++) {
    const int64_t i = base + threadIdx.x + (int64_t)j * kPlaneBlock;
    if (i >= a.n) break;
    const double d = a.dist[i];
    if (!(d <= thr)) continue;  // the cull's rule (icpengine.cpp:265); a NaN residual is invalid
    if (AT && !__builtin_isfinite(d)) continue;  // an infinite threshold takes every finite pair
    const int32_t pos = a.pos[i];
    const double nx = a.normals[3 * (int64_t)pos], ny = a.normals[3 * (int64_t)pos + 1],
                 nz = a.normals[3 * (int64_t)pos + 2];
    if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
      v[29] += 1.0;
      continue;
    }
    const TgtPt* p = a.pts + pos;
    const double2 bxy = *reinterpret_cast<const double2*>(&p->x);
    const double ax = a.x[i], ay = a.y[i], az = a.z[i];
    const double r = (nx * (ax - bxy.x) + ny * (ay - bxy.y)) + nz * (az - p->z);
    const double px = ax - ox, py = ay - oy, pz = az - oz;
    // J = (a' x n, n)
    const double J[6] = {py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz};
    int m = 0;
#pragma unroll
    for (int p_ = 0; p_ < 6; p_++) {
#pragma unroll
      for (int q = p_; q < 6; q++) v[m++] += J[p_] * J[q];
    }
#pragma unroll
    for (int p_ = 0; p_ < 6; p_++) v[21 + p_] += J[p_] * r;
    v[27] += r * r;
    v[28] += 1.0;
  }
  block_sum<kPlaneSums>(v, red);
  if (threadIdx.x < kPlaneSums) {
    // v[] is indexed by a constant below: every thread holds the block's sums
    double out = 0.0;
#pragma unroll
    for (int k = 0; k < kPlaneSums; k++) out = threadIdx.x == k ? v[k] : out;
    a.parts[(int64_t)blockIdx.x * kPlaneSums + threadIdx.x] = out;
  }
}

__global__ void __launch_bounds__(64) k_plane_merge(const double* __restrict__ parts, int64_t nparts,
                                                    double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= kPlaneSums) return;
  double s = 0.0;
  for (int64_t p = 0; p < nparts; p++) s += parts[p * kPlaneSums + k];
  out[k] = s;
}

}  // namespace

int64_t plane_num_parts(int64_t n) { return (n + kPlanePart - 1) / kPlanePart; }

namespace {
template <bool AT>
hipError_t launch_plane(const PlaneLaunch& a, hipStream_t s) {
  const int64_t nparts = plane_num_parts(a.n);
  if (nparts > 0) hipLaunchKernelGGL(k_plane_sums<AT>, dim3((unsigned)nparts), dim3(kPlaneBlock), 0, s, a);
  hipLaunchKernelGGL(k_plane_merge, dim3(1), dim3(64), 0, s, a.parts, nparts, a.out);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_plane_sums(const PlaneLaunch& a, hipStream_t s) { return launch_plane<false>(a, s); }
hipError_t launch_plane_sums_at(const PlaneLaunch& a, hipStream_t s) { return launch_plane<true>(a, s); }

}  // namespace icp
