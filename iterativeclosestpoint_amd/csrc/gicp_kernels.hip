// gicp_kernels.hip — the generalized-ICP ("plane-to-plane") normal equations of an iterate's valid
// pairs, fp64, no FMA, and the source normals' moves between the caller's order
// and slot order. A call of its own after the iterate, as plane_kernels.hip: it reads the moved
// source, the matches, the residuals, the threshold, the target points and both clouds' normals,
// and writes none of them.
//  gicp_pair_terms  the 28 terms of one pair: the one place that fixes their operation order
//                   (tests/gicp_reference.py gicp_terms mirrors it line for line).
//  k_gicp_sums      fixed parts of 4096 queries: thread t of a part adds its queries t + 256 j
//                   (j < 16) in order, then the block's fixed tree (block_sum).
//  k_gicp_merge     the parts added in index order, one thread per sum.
// The bits depend neither on the run nor on which search path settled which query.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "nn_device.h"

namespace icp {
namespace {
using namespace dev;

constexpr int kGicpPart = 4096;
constexpr int kGicpBlock = 256;

// One pair: the moved source point a, its match b, the source normal n0 in the frame it was made
// in (R takes it to a's frame), the target normal nb, f = 1 - epsilon, o the origin of the step.
// t[0..20]: J^T M J's upper triangle row by row, t[21..26]: J^T M r, t[27]: r^T M r, with
// M = (C_a + C_b)^-1, C = I - f n n^T, J = [-[a - o]x | I].
__device__ __forceinline__ void gicp_pair_terms(double ax, double ay, double az, double bx, double by, double bz,
                                                double n0x, double n0y, double n0z, double nbx, double nby,
                                                double nbz, const double* R, double f, double ox, double oy,
                                                double oz, double (&t)[28]) {
  const double nax = (R[0] * n0x + R[1] * n0y) + R[2] * n0z;
  const double nay = (R[3] * n0x + R[4] * n0y) + R[5] * n0z;
  const double naz = (R[6] * n0x + R[7] * n0y) + R[8] * n0z;
  // S = C_a + C_b
  const double s00 = 2.0 - f * (nax * nax + nbx * nbx);
  const double s11 = 2.0 - f * (nay * nay + nby * nby);
  const double s22 = 2.0 - f * (naz * naz + nbz * nbz);
  const double s01 = 0.0 - f * (nax * nay + nbx * nby);
  const double s02 = 0.0 - f * (nax * naz + nbx * nbz);
  const double s12 = 0.0 - f * (nay * naz + nby * nbz);
  // M = S^-1 by the adjugate
  const double c00 = s11 * s22 - s12 * s12;
  const double c01 = s02 * s12 - s01 * s22;
  const double c02 = s01 * s12 - s02 * s11;
  const double c11 = s00 * s22 - s02 * s02;
  const double c12 = s01 * s02 - s00 * s12;
  const double c22 = s00 * s11 - s01 * s01;
  const double det = (s00 * c00 + s01 * c01) + s02 * c02;
  const double m00 = c00 / det, m01 = c01 / det, m02 = c02 / det;
  const double m11 = c11 / det, m12 = c12 / det, m22 = c22 / det;
  const double rx = ax - bx, ry = ay - by, rz = az - bz;
  const double px = ax - ox, py = ay - oy, pz = az - oz;
  // y = M r
  const double yx = (m00 * rx + m01 * ry) + m02 * rz;
  const double yy = (m01 * rx + m11 * ry) + m12 * rz;
  const double yz = (m02 * rx + m12 * ry) + m22 * rz;
  // Q = [a']x M: column q is a' x (column q of M)
  const double q00 = py * m02 - pz * m01, q10 = pz * m00 - px * m02, q20 = px * m01 - py * m00;
  const double q01 = py * m12 - pz * m11, q11 = pz * m01 - px * m12, q21 = px * m11 - py * m01;
  const double q02 = py * m22 - pz * m12, q12 = pz * m02 - px * m22, q22 = px * m12 - py * m02;
  // the rotation block Q [a']x^T: row p is a' x (row p of Q)
  t[0] = py * q02 - pz * q01;
  t[1] = pz * q00 - px * q02;
  t[2] = px * q01 - py * q00;
  t[3] = q00;
  t[4] = q01;
  t[5] = q02;
  t[6] = pz * q10 - px * q12;
  t[7] = px * q11 - py * q10;
  t[8] = q10;
  t[9] = q11;
  t[10] = q12;
  t[11] = px * q21 - py * q20;
  t[12] = q20;
  t[13] = q21;
  t[14] = q22;
  t[15] = m00;
  t[16] = m01;
  t[17] = m02;
  t[18] = m11;
  t[19] = m12;
  t[20] = m22;
  // g = (a' x y, y)
  t[21] = py * yz - pz * yy;
  t[22] = pz * yx - px * yz;
  t[23] = px * yy - py * yx;
  t[24] = yx;
  t[25] = yy;
  t[26] = yz;
  t[27] = (rx * yx + ry * yy) + rz * yz;
}

// AT: the caller's threshold (a.thr) and only finite residuals, instead of the device record's.
template <bool AT>
__global__ void __launch_bounds__(kGicpBlock) k_gicp_sums(GicpLaunch a) {
  __shared__ double red[(kGicpBlock / kWave) * kGicpSums];
  const int64_t base = (int64_t)blockIdx.x * kGicpPart;
  const double thr = AT ? a.thr : a.it->thr;
  double v[kGicpSums];
#pragma unroll
  for (int k = 0; k < kGicpSums; k++) v[k] = 0.0;
  for (int j = 0; j < kGicpPart / kGicpBlock; j++) {
    const int64_t i = base + threadIdx.x + (int64_t)j * kGicpBlock;
    if (i >= a.n) break;
    const double d = a.dist[i];
    if (!(d <= thr)) continue;  // the cull's rule; a NaN residual is invalid
    if (AT && !__builtin_isfinite(d)) continue;  // an infinite threshold takes every finite pair
    const int32_t pos = a.pos[i];
    const double nbx = a.normals[3 * (int64_t)pos], nby = a.normals[3 * (int64_t)pos + 1],
                 nbz = a.normals[3 * (int64_t)pos + 2];
    const double n0x = a.src_normals[3 * i], n0y = a.src_normals[3 * i + 1], n0z = a.src_normals[3 * i + 2];
    const TgtPt* p = a.pts + pos;
    const double2 bxy = *reinterpret_cast<const double2*>(&p->x);
    double t[28];
    gicp_pair_terms(a.x[i], a.y[i], a.z[i], bxy.x, bxy.y, p->z, n0x, n0y, n0z, nbx, nby, nbz, a.R, a.f, a.origin[0],
                    a.origin[1], a.origin[2], t);
#pragma unroll
    for (int k = 0; k < 28; k++) v[k] += t[k];
    v[28] += 1.0;
    if (n0x == 0.0 && n0y == 0.0 && n0z == 0.0) v[29] += 1.0;
    if (nbx == 0.0 && nby == 0.0 && nbz == 0.0) v[30] += 1.0;
  }
  block_sum<kGicpSums>(v, red);
  if (threadIdx.x < kGicpSums) {
    // v[] is indexed by a constant below: every thread holds the block's sums
    double out = 0.0;
#pragma unroll
    for (int k = 0; k < kGicpSums; k++) out = threadIdx.x == k ? v[k] : out;
    a.parts[(int64_t)blockIdx.x * kGicpSums + threadIdx.x] = out;
  }
}

__global__ void __launch_bounds__(64) k_gicp_merge(const double* __restrict__ parts, int64_t nparts,
                                                   double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= kGicpSums) return;
  double s = 0.0;
  for (int64_t p = 0; p < nparts; p++) s += parts[p * kGicpSums + k];
  out[k] = s;
}

// slot[k] = aos[perm[k]]: normals in the caller's source order into slot order. With bad, the rows
// that are neither of unit length nor zero are counted (k_normals_to_leaf's rule).
__global__ void __launch_bounds__(256) k_src_normals_to_slot(const int32_t* __restrict__ perm,
                                                             const double* __restrict__ aos,
                                                             double* __restrict__ slot, int64_t n, unsigned* bad) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t o = perm[k];
  const double x = aos[3 * o], y = aos[3 * o + 1], z = aos[3 * o + 2];
  if (bad) {
    const double nn = x * x + y * y + z * z;
    const bool ok = (x == 0.0 && y == 0.0 && z == 0.0) || __builtin_fabs(nn - 1.0) <= 1e-12;  // NaN: not ok
    if (!ok) atomicAdd(bad, 1u);
  }
  slot[3 * k] = x;
  slot[3 * k + 1] = y;
  slot[3 * k + 2] = z;
}

__global__ void __launch_bounds__(256) k_src_normals_from_slot(const int32_t* __restrict__ perm,
                                                               const double* __restrict__ slot,
                                                               double* __restrict__ aos, int64_t n) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int64_t o = perm[k];
  aos[3 * o] = slot[3 * k];
  aos[3 * o + 1] = slot[3 * k + 1];
  aos[3 * o + 2] = slot[3 * k + 2];
}

// *bad += the points of an AoS cloud with a non-finite coordinate.
__global__ void __launch_bounds__(256) k_count_nonfinite(const double* __restrict__ aos, int64_t n, unsigned* bad) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double x = aos[3 * k], y = aos[3 * k + 1], z = aos[3 * k + 2];
  if (!(x - x == 0.0) || !(y - y == 0.0) || !(z - z == 0.0)) atomicAdd(bad, 1u);
}

inline unsigned grid_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

template <bool AT>
hipError_t launch_gicp(const GicpLaunch& a, hipStream_t s) {
  const int64_t nparts = gicp_num_parts(a.n);
  if (nparts > 0) hipLaunchKernelGGL(k_gicp_sums<AT>, dim3((unsigned)nparts), dim3(kGicpBlock), 0, s, a);
  hipLaunchKernelGGL(k_gicp_merge, dim3(1), dim3(64), 0, s, a.parts, nparts, a.out);
  return hipGetLastError();
}

}  // namespace

int64_t gicp_num_parts(int64_t n) { return (n + kGicpPart - 1) / kGicpPart; }

hipError_t launch_gicp_sums(const GicpLaunch& a, hipStream_t s) { return launch_gicp<false>(a, s); }
hipError_t launch_gicp_sums_at(const GicpLaunch& a, hipStream_t s) { return launch_gicp<true>(a, s); }

hipError_t launch_src_normals_to_slot(const int32_t* perm, const double* aos, double* slot, int64_t n, unsigned* bad,
                                      hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_src_normals_to_slot, dim3(grid_for(n, 256)), dim3(256), 0, s, perm, aos, slot, n, bad);
  return hipGetLastError();
}

hipError_t launch_src_normals_from_slot(const int32_t* perm, const double* slot, double* aos, int64_t n,
                                        hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_src_normals_from_slot, dim3(grid_for(n, 256)), dim3(256), 0, s, perm, slot, aos, n);
  return hipGetLastError();
}

hipError_t launch_count_nonfinite(const double* aos, int64_t n, unsigned* bad, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_count_nonfinite, dim3(grid_for(n, 256)), dim3(256), 0, s, aos, n, bad);
  return hipGetLastError();
}

}  // namespace icp
