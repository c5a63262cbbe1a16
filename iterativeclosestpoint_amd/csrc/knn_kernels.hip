// knn_kernels.hip — k nearest neighbours through the resident octree, and the target's normals
// built on them, all fp64, no FMA:
//  (the walk itself: knn_walk.h)
//  k_knn             one thread per query: the k target points smallest under (fl(d2), original
//                    index), ascending. The tie rule is the index, not the 1-NN's visit order: the
//                    set then does not depend on the traversal and a brute-force check is defined.
//  k_target_normals  the same walk with the target points themselves as queries, in leaf order
//                    (neighbouring threads walk the same nodes), then the covariance of the k
//                    neighbours and its smallest eigenvector (the Jacobi of svd3_impl.h).
//  k_normals_to_leaf / _from_leaf  normals between the caller's target order and leaf order.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "knn_walk.h"
#include "nn_device.h"
#include "svd3_impl.h"

namespace icp {
namespace {
using namespace dev;

__device__ __forceinline__ bool finite3(double x, double y, double z) {
  return __builtin_fabs(x) < __builtin_inf() && __builtin_fabs(y) < __builtin_inf() &&
         __builtin_fabs(z) < __builtin_inf();
}

__global__ void __launch_bounds__(256) k_knn(const NodeRec* __restrict__ nodes, const TgtPt* __restrict__ pts,
                                             int levels, const double* __restrict__ q, int64_t n, int k,
                                             int32_t* __restrict__ idx_out, double* __restrict__ d2_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long knn_smem[];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;  // no barriers below
  const int bs = blockDim.x;
  const KnnLds l = knn_lds(knn_smem, levels, k);
  const double qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
  int cnt = 0;
  if (finite3(qx, qy, qz)) cnt = knn_walk<false>(nodes, pts, qx, qy, qz, k, l.st, l.ld, l.lp, bs);
  for (int r = 0; r < k; r++) {
    if (idx_out) idx_out[i * k + r] = r < cnt ? pts[l.lp[r * bs]].orig : -1;
    if (d2_out) d2_out[i * k + r] = r < cnt ? l.ld[r * bs] : __builtin_nan("");
  }
}

// A neighbourhood defines a plane only when its second eigenvalue is above this fraction of the
// first (sqrt(eps), as kPlanePivotMin): below it the smallest eigenvector keeps fewer than half
// its digits, and on collinear points it is made of the sums' rounding. A guard, not a tuned value.
constexpr double kNormalRankMin = 0x1p-26;

struct View {
  double v[3];
};

__global__ void __launch_bounds__(256) k_target_normals(const NodeRec* __restrict__ nodes,
                                                        const TgtPt* __restrict__ pts, int levels, int64_t n, int k,
                                                        int has_view, View view, double* __restrict__ normals) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long knn_smem[];
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;  // no barriers below
  const int bs = blockDim.x;
  const KnnLds l = knn_lds(knn_smem, levels, k);
  const double2 qxy = *reinterpret_cast<const double2*>(&pts[j].x);
  const double qx = qxy.x, qy = qxy.y, qz = pts[j].z;
  const int cnt = knn_walk<false>(nodes, pts, qx, qy, qz, k, l.st, l.ld, l.lp, bs);
  // the mean in neighbour order, then the centred second moments
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int r = 0; r < cnt; r++) {
    const TgtPt* p = pts + l.lp[r * bs];
    sx += p->x;
    sy += p->y;
    sz += p->z;
  }
  const double mx = sx / (double)k, my = sy / (double)k, mz = sz / (double)k;
  double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
  for (int r = 0; r < cnt; r++) {
    const TgtPt* p = pts + l.lp[r * bs];
    const double dx = p->x - mx, dy = p->y - my, dz = p->z - mz;
    c00 += dx * dx;
    c01 += dx * dy;
    c02 += dx * dz;
    c11 += dy * dy;
    c12 += dy * dz;
    c22 += dz * dz;
  }
  const double C[9] = {c00, c01, c02, c01, c11, c12, c02, c12, c22};
  double U[9], S[3], V[9];
  svd::jacobi_svd3(C, U, S, V);
  // C is symmetric positive semi-definite: its singular values are its eigenvalues (descending)
  // and V's third column the eigenvector of the smallest
  double nx = 0.0, ny = 0.0, nz = 0.0;
  if (S[1] > kNormalRankMin * S[0]) {
    nx = V[2];
    ny = V[5];
    nz = V[8];
    const double len = __builtin_sqrt(nx * nx + ny * ny + nz * nz);
    nx /= len;
    ny /= len;
    nz /= len;
    bool flip;
    if (has_view) {
      flip = nx * (view.v[0] - qx) + ny * (view.v[1] - qy) + nz * (view.v[2] - qz) < 0.0;
    } else {
      const double ax = __builtin_fabs(nx), ay = __builtin_fabs(ny), az = __builtin_fabs(nz);
      double lead = nx, la = ax;
      if (ay > la) {
        lead = ny;
        la = ay;
      }
      if (az > la) lead = nz;
      flip = lead < 0.0;
    }
    if (flip) {
      nx = -nx;
      ny = -ny;
      nz = -nz;
    }
    if (!(len > 0.0)) nx = ny = nz = 0.0;
  }
  normals[3 * j] = nx;
  normals[3 * j + 1] = ny;
  normals[3 * j + 2] = nz;
}

__global__ void __launch_bounds__(256) k_normals_to_leaf(const TgtPt* __restrict__ pts, const double* __restrict__ aos,
                                                         double* __restrict__ leaf, int64_t n, unsigned* bad) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t o = pts[j].orig;
  const double x = aos[3 * o], y = aos[3 * o + 1], z = aos[3 * o + 2];
  const double nn = x * x + y * y + z * z;
  const bool ok = (x == 0.0 && y == 0.0 && z == 0.0) || __builtin_fabs(nn - 1.0) <= 1e-12;  // NaN: not ok
  if (!ok) atomicAdd(bad, 1u);
  leaf[3 * j] = x;
  leaf[3 * j + 1] = y;
  leaf[3 * j + 2] = z;
}

__global__ void __launch_bounds__(256) k_normals_from_leaf(const TgtPt* __restrict__ pts,
                                                           const double* __restrict__ leaf, double* __restrict__ aos,
                                                           int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t o = pts[j].orig;
  aos[3 * o] = leaf[3 * j];
  aos[3 * o + 1] = leaf[3 * j + 1];
  aos[3 * o + 2] = leaf[3 * j + 2];
}

inline unsigned grid_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

int knn_block_threads(int levels, int k) {
  // per thread: levels x 8 B of stack, k x (8 + 4) B of list; stack plus list <= 64 KiB per block
  const size_t per = (size_t)levels * 8 + (size_t)k * 12;
  if (per * 256 <= 65536) return 256;
  if (per * 128 <= 65536) return 128;
  return 64;  // levels <= 61 (max_depth <= 60), k <= 32: 872 B per thread, 54.5 KiB
}

hipError_t launch_knn(const NodeRec* nodes, const TgtPt* pts, int levels, const double* q_aos, int64_t n, int k,
                      int32_t* idx_out, double* d2_out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int lv = levels < 1 ? 1 : levels;
  const int bs = knn_block_threads(lv, k);
  const size_t shmem = knn_lds_bytes(lv, k, bs);
  if (shmem > 65536) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_knn, dim3(grid_for(n, bs)), dim3(bs), shmem, s, nodes, pts, lv, q_aos, n, k, idx_out, d2_out);
  return hipGetLastError();
}

hipError_t launch_target_normals(const NodeRec* nodes, const TgtPt* pts, int levels, int64_t n, int k, int has_view,
                                 const double view[3], double* normals, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int lv = levels < 1 ? 1 : levels;
  const int bs = knn_block_threads(lv, k);
  const size_t shmem = knn_lds_bytes(lv, k, bs);
  if (shmem > 65536) return hipErrorInvalidValue;
  View v;
  for (int c = 0; c < 3; c++) v.v[c] = has_view ? view[c] : 0.0;
  hipLaunchKernelGGL(k_target_normals, dim3(grid_for(n, bs)), dim3(bs), shmem, s, nodes, pts, lv, n, k, has_view, v,
                     normals);
  return hipGetLastError();
}

hipError_t launch_normals_to_leaf(const TgtPt* pts, const double* aos, double* leaf, int64_t n, unsigned* bad,
                                  hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_normals_to_leaf, dim3(grid_for(n, 256)), dim3(256), 0, s, pts, aos, leaf, n, bad);
  return hipGetLastError();
}

hipError_t launch_normals_from_leaf(const TgtPt* pts, const double* leaf, double* aos, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_normals_from_leaf, dim3(grid_for(n, 256)), dim3(256), 0, s, pts, leaf, aos, n);
  return hipGetLastError();
}

}  // namespace icp
