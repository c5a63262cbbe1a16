// outlier_kernels.hip — statistical and radius outlier removal on the device (the
// definition: include/icp_hip.h), over a private octree of the cloud, all fp64, no FMA:
//   scores      one thread per point in leaf order (neighbouring threads walk the same nodes).
//               Statistical: knn_walk (knn_walk.h) with the thread's own leaf position skipped, the
//               list and the stack in LDS; the epilogue adds the k roots in list order and stores
//               the score at the point's original index. Radius: a DFS with only the stack in LDS
//               that counts the points with fl(d2) <= r2 and ends once the count reaches k.
//   statistics  sums of (score - c) and (score - c)^2, c = score[0], over fixed parts of 4096
//               consecutive scores (16 consecutive scores per thread, a fixed tree over the block),
//               then one block over the parts and the head record: mean, std, threshold.
//   compaction  a flag per point from the head's threshold, hipCUB's exclusive sum, the number of
//               kept points, and the gather of indices and coordinates (stable: indices ascend).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

#include "kernels.h"
#include "knn_walk.h"
#include "nn_device.h"

namespace icp {
namespace {
using namespace dev;

constexpr int kOutPart = 4096;      // scores per part of the statistics
constexpr int kOutPerThread = 16;   // consecutive scores per thread of a part's block (256 threads)

inline unsigned grid_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

__global__ void __launch_bounds__(256) k_outlier_scores_knn(const NodeRec* __restrict__ nodes,
                                                            const TgtPt* __restrict__ pts, int levels, int64_t n, int k,
                                                            double* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long outlier_smem[];
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;  // no barriers below
  const int bs = blockDim.x;
  const KnnLds l = knn_lds(outlier_smem, levels, k);
  const double2 qxy = *reinterpret_cast<const double2*>(&pts[j].x);
  const double2 qzw = *reinterpret_cast<const double2*>(&pts[j].z);
  const int32_t orig = (int32_t)(uint32_t)(unsigned long long)__double_as_longlong(qzw.y);
  const int cnt = knn_walk<true>(nodes, pts, qxy.x, qxy.y, qzw.x, k, l.st, l.ld, l.lp, bs, (int32_t)j);
  double sum = 0.0;
  for (int r = 0; r < cnt; r++) sum += __builtin_sqrt(l.ld[r * bs]);  // neighbour order (+0.0 + d is d)
  score[orig] = sum / (double)k;
}

// The points other than `self` with fl(d2) <= r2, saturated at k: knn_walk's traversal (nearest
// child first, the siblings of a level as one stack entry with a 16-bit lower-bound key) against
// the fixed bound r2. A node is skipped when its squared box distance s > r2, strictly (monotone
// rounding: a point with fl(d2) <= r2 lies only in nodes with s <= r2).
__device__ __forceinline__ int radius_count(const NodeRec* __restrict__ nodes, const TgtPt* __restrict__ pts,
                                            double qx, double qy, double qz, double r2, int k, int32_t self,
                                            unsigned long long* st, int bs) {
  int cnt = 0;
  const uint32_t thr_key = key16(r2);
  int sp = 0;
  int32_t node = 0;
  double lx = nodes[0].lo[0], ly = nodes[0].lo[1], lz = nodes[0].lo[2];
  double hx = nodes[0].hi[0], hy = nodes[0].hi[1], hz = nodes[0].hi[2];
  double s = box_s(lx, ly, lz, hx, hy, hz, qx, qy, qz);
  while (true) {
    bool entered = false;
    if (!(s > r2)) {
      const int2 topo = *reinterpret_cast<const int2*>(&nodes[node].first);
      const int32_t first = topo.x;
      const uint32_t meta = (uint32_t)topo.y;
      if (meta & kLeafBit) {
        const int32_t lcnt = (int32_t)(meta & ~kLeafBit);
        for (int32_t c = 0; c < lcnt; c++) {
          if (first + c == self) continue;
          const double d2 = d2_to(pts + first + c, qx, qy, qz);
          if (d2 <= r2) {
            cnt++;
            if (cnt == k) return cnt;
          }
        }
      } else {
        const OctantDist od = octant_dist(lx, ly, lz, hx, hy, hz, qx, qy, qz);
        const uint32_t mask = meta & 0xffu;
        double bs_ = __builtin_inf();
        uint32_t o1 = 0;
        bool any = false;
#pragma unroll
        for (int o = 0; o < 8; o++) {
          const double c = od.of(o);
          const bool take = ((mask >> o) & 1u) && (c < bs_ || !any);
          bs_ = take ? c : bs_;
          o1 = take ? (uint32_t)o : o1;
          any = any || take;
        }
        const uint32_t rem = mask & ~(1u << o1);
        uint32_t kmin = 0xffffu;
#pragma unroll
        for (int o = 0; o < 8; o++) {
          const uint32_t kk = key16(od.of(o));
          kmin = ((rem >> o) & 1u) && kk < kmin ? kk : kmin;
        }
        if (rem && kmin <= thr_key) {  // key16 is monotone: a larger key means every sibling has s > r2
          st[sp * bs] = ((unsigned long long)kmin << 48) | ((unsigned long long)mask << 40) |
                        ((unsigned long long)rem << 32) | (uint32_t)first;
          sp++;
        }
        node = first + __builtin_popcount(mask & ((1u << o1) - 1u));
        if (o1 & 1u) lx = od.mx; else hx = od.mx;
        if (o1 & 2u) ly = od.my; else hy = od.my;
        if (o1 & 4u) lz = od.mz; else hz = od.mz;
        s = bs_;
        entered = true;
      }
    }
    if (entered) continue;
    if (sp == 0) break;
    const unsigned long long e = st[(sp - 1) * bs];
    uint32_t rem = (uint32_t)(e >> 32) & 0xffu;
    const uint32_t pmask = (uint32_t)(e >> 40) & 0xffu;
    const int32_t first = (int32_t)(uint32_t)e;
    const uint32_t o = (uint32_t)__builtin_ctz(rem);
    rem &= rem - 1u;
    if (rem == 0) sp--;
    else st[(sp - 1) * bs] = (e & ~(0xffull << 32)) | ((unsigned long long)rem << 32);
    node = first + __builtin_popcount(pmask & ((1u << o) - 1u));
    const NodeBox nb = load_node_box(nodes + node);
    lx = nb.l01.x; ly = nb.l01.y; lz = nb.l2h0.x; hx = nb.l2h0.y; hy = nb.h12.x; hz = nb.h12.y;
    s = box_s(lx, ly, lz, hx, hy, hz, qx, qy, qz);
  }
  return cnt;
}

__global__ void __launch_bounds__(256) k_outlier_scores_radius(const NodeRec* __restrict__ nodes,
                                                               const TgtPt* __restrict__ pts, int64_t n, int k,
                                                               double r2, double* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long outlier_smem[];
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;  // no barriers below
  const double2 qxy = *reinterpret_cast<const double2*>(&pts[j].x);
  const double2 qzw = *reinterpret_cast<const double2*>(&pts[j].z);
  const int32_t orig = (int32_t)(uint32_t)(unsigned long long)__double_as_longlong(qzw.y);
  const int cnt = radius_count(nodes, pts, qxy.x, qxy.y, qzw.x, r2, k, (int32_t)j, outlier_smem + threadIdx.x,
                               (int)blockDim.x);
  score[orig] = (double)cnt;
}

// Statistics, the parts: part b = (sum of x_i - c, sum of (x_i - c)^2) over its 4096 scores, c the
// first score of the array. A thread adds its 16 consecutive scores in index order; the block's
// tree is block_sum's (a wave's DPP tree, then the four waves in order). Slots past n add +0.0.
__global__ void __launch_bounds__(256) k_outlier_moments(const double* __restrict__ score, int64_t n,
                                                         double* __restrict__ parts) {
  __shared__ double red[2 * 4];
  const double c = score[0];
  const int64_t i0 = (int64_t)blockIdx.x * kOutPart + (int64_t)threadIdx.x * kOutPerThread;
  double v[2] = {0.0, 0.0};
  for (int e = 0; e < kOutPerThread; e++) {
    const int64_t i = i0 + e;
    if (i < n) {
      const double d = score[i] - c;
      v[0] = v[0] + d;
      v[1] = v[1] + d * d;
    }
  }
  block_sum<2>(v, red);
  if (threadIdx.x == 0) {
    parts[2 * blockIdx.x] = v[0];
    parts[2 * blockIdx.x + 1] = v[1];
  }
}

// Statistics, the head: thread t adds the parts t, t + 256, ... in that order, the block's tree
// again, then mean = c + S1 / n, var = S2 / n - (S1 / n)^2 (not below 0), std = sqrt(var) and the
// threshold: mean + ratio * std (one product, one sum), or the radius mode's k.
__global__ void __launch_bounds__(256) k_outlier_head(const double* __restrict__ score, int64_t n,
                                                      const double* __restrict__ parts, int nparts, int mode,
                                                      double param, int k, OutlierHead* __restrict__ head) {
  __shared__ double red[2 * 4];
  double v[2] = {0.0, 0.0};
  for (int p = threadIdx.x; p < nparts; p += 256) {
    v[0] = v[0] + parts[2 * p];
    v[1] = v[1] + parts[2 * p + 1];
  }
  block_sum<2>(v, red);
  if (threadIdx.x == 0) {
    const double c = score[0];
    const double m1 = v[0] / (double)n;
    double var = v[1] / (double)n - m1 * m1;
    var = var > 0.0 ? var : 0.0;
    const double mean = c + m1, sd = __builtin_sqrt(var);
    head->mean = mean;
    head->sd = sd;
    head->threshold = mode == ICP_OUTLIER_STATISTICAL ? mean + param * sd : (double)k;
    head->m = 0;
    head->pad = 0;
  }
}

// Compaction: keep i iff score <= threshold (the cull's comparison), or in the radius mode iff the
// saturated count is k.
__global__ void __launch_bounds__(256) k_outlier_flags(const double* __restrict__ score, int64_t n, int mode,
                                                       const OutlierHead* __restrict__ head, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double t = head->threshold;
  flag[i] = (mode == ICP_OUTLIER_STATISTICAL ? score[i] <= t : score[i] == t) ? 1 : 0;
}

__global__ void k_outlier_m(const int32_t* __restrict__ flag, const int32_t* __restrict__ pos, int64_t n,
                            OutlierHead* __restrict__ head) {
  head->m = pos[n - 1] + flag[n - 1];
}

__global__ void __launch_bounds__(256) k_outlier_gather(const double* __restrict__ xyz, int64_t n,
                                                        const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                                        double* __restrict__ xyz_out, int32_t* __restrict__ index_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const int64_t r = pos[i];
  if (index_out) index_out[r] = (int32_t)i;
  if (xyz_out) {
    xyz_out[3 * r] = xyz[3 * i];
    xyz_out[3 * r + 1] = xyz[3 * i + 1];
    xyz_out[3 * r + 2] = xyz[3 * i + 2];
  }
}

}  // namespace

int outlier_num_parts(int64_t n) { return (int)((n + kOutPart - 1) / kOutPart); }

hipError_t outlier_temp_bytes(int64_t n, size_t* bytes) {
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n, nullptr);
}

hipError_t launch_outlier_scores(const NodeRec* nodes, const TgtPt* pts, int levels, int64_t n, int mode, int k,
                                 double param, double* score, hipStream_t s) {
  const int lv = levels < 1 ? 1 : levels;
  const int kl = mode == ICP_OUTLIER_STATISTICAL ? k : 0;  // the radius mode keeps no list
  const int bs = knn_block_threads(lv, kl);
  const size_t shmem = knn_lds_bytes(lv, kl, bs);
  if (shmem > 65536) return hipErrorInvalidValue;
  if (mode == ICP_OUTLIER_STATISTICAL)
    hipLaunchKernelGGL(k_outlier_scores_knn, dim3(grid_for(n, bs)), dim3(bs), shmem, s, nodes, pts, lv, n, k, score);
  else
    hipLaunchKernelGGL(k_outlier_scores_radius, dim3(grid_for(n, bs)), dim3(bs), shmem, s, nodes, pts, n, k,
                       param * param, score);
  return hipGetLastError();
}

hipError_t launch_outlier_stats(const double* score, int64_t n, int mode, int k, double param, double* parts,
                                OutlierHead* head, hipStream_t s) {
  const int nparts = outlier_num_parts(n);
  hipLaunchKernelGGL(k_outlier_moments, dim3((unsigned)nparts), dim3(256), 0, s, score, n, parts);
  hipLaunchKernelGGL(k_outlier_head, dim3(1), dim3(256), 0, s, score, n, parts, nparts, mode, param, k, head);
  return hipGetLastError();
}

hipError_t launch_outlier_flags(void* tmp, size_t tmp_bytes, const double* score, int64_t n, int mode, int32_t* flag,
                                int32_t* pos, OutlierHead* head, hipStream_t s) {
  hipLaunchKernelGGL(k_outlier_flags, dim3(grid_for(n, 256)), dim3(256), 0, s, score, n, mode, head, flag);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, flag, pos, (int)n, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_outlier_m, dim3(1), dim3(1), 0, s, flag, pos, n, head);
  return hipGetLastError();
}

hipError_t launch_outlier_gather(const double* xyz, int64_t n, const int32_t* flag, const int32_t* pos, double* xyz_out,
                                 int32_t* index_out, hipStream_t s) {
  hipLaunchKernelGGL(k_outlier_gather, dim3(grid_for(n, 256)), dim3(256), 0, s, xyz, n, flag, pos, xyz_out, index_out);
  return hipGetLastError();
}

}  // namespace icp
