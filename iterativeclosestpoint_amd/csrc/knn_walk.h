// knn_walk.h — the k-NN walk of the octree and its LDS columns, shared by the kernels that run it:
// k_knn and k_target_normals (knn_kernels.hip) and the statistical outlier scores
// (outlier_kernels.hip). Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "nn_device.h"

namespace icp {
namespace dev {

// The walk of k_target_sep (nn_ball.hip) with a k-entry list instead of the scalar best: nearest
// child first, the remaining siblings of a level as one stack entry with a 16-bit lower-bound key.
// The list holds (fl(d2), leaf position) ascending under (fl(d2), original index), in LDS, entry j
// of a thread at [j * bs] like the stack, so a wave's accesses fall on different banks (a list
// indexed dynamically in registers would live in scratch). Once it is full, kd is its last entry's
// d2: a node is skipped only when its squared box distance s > kd, strictly (monotone rounding:
// every point inside has fl(d2) >= s; at equality a point inside can still win on its index), and
// a point replaces the last entry when (d2, orig) < (kd, its orig). The original index of a list
// entry is read from the point record only on a tie of d2.
// SKIP: the point at leaf position `self` (the query itself, excluded by position and so by index)
// never enters the list; without SKIP `self` is unused and the code is the walk without it.
// Returns the entries found (k when the target holds at least k points besides a skipped one).
template <bool SKIP>
__device__ __forceinline__ int knn_walk(const NodeRec* __restrict__ nodes, const TgtPt* __restrict__ pts, double qx,
                                        double qy, double qz, int k, unsigned long long* st, double* ld, int32_t* lp,
                                        int bs, int32_t self = -1) {
  int cnt = 0;
  double kd = __builtin_inf();
  uint32_t thr_key = key16(kd);
  int sp = 0;
  int32_t node = 0;
  double lx = nodes[0].lo[0], ly = nodes[0].lo[1], lz = nodes[0].lo[2];
  double hx = nodes[0].hi[0], hy = nodes[0].hi[1], hz = nodes[0].hi[2];
  double s = box_s(lx, ly, lz, hx, hy, hz, qx, qy, qz);
  while (true) {
    bool entered = false;
    if (!(s > kd)) {
      const int2 topo = *reinterpret_cast<const int2*>(&nodes[node].first);
      const int32_t first = topo.x;
      const uint32_t meta = (uint32_t)topo.y;
      if (meta & kLeafBit) {
        const int32_t lcnt = (int32_t)(meta & ~kLeafBit);
        for (int32_t c = 0; c < lcnt; c++) {
          if (SKIP && first + c == self) continue;
          const TgtPt* p = pts + first + c;
          const double2 pxy = *reinterpret_cast<const double2*>(&p->x);
          const double2 pzw = *reinterpret_cast<const double2*>(&p->z);
          const double dx = pxy.x - qx, dy = pxy.y - qy, dz = pzw.x - qz;
          const double d2 = dx * dx + dy * dy + dz * dz;  // d2_to's arithmetic
          const int32_t orig = (int32_t)(uint32_t)(unsigned long long)__double_as_longlong(pzw.y);
          if (cnt == k) {
            if (d2 > kd) continue;
            if (d2 == kd && orig > pts[lp[(k - 1) * bs]].orig) continue;
          }
          int j = cnt < k ? cnt : k - 1;
          while (j > 0) {
            const double ed = ld[(j - 1) * bs];
            const int32_t ep = lp[(j - 1) * bs];
            if (ed < d2 || (ed == d2 && pts[ep].orig < orig)) break;
            ld[j * bs] = ed;
            lp[j * bs] = ep;
            j--;
          }
          ld[j * bs] = d2;
          lp[j * bs] = first + c;
          if (cnt < k) cnt++;
          if (cnt == k) {
            kd = ld[(k - 1) * bs];
            thr_key = key16(kd);
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
          // the first existing child when every distance is infinite (an overflowing query)
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
        if (rem) {
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
    bool found = false;
    while (sp > 0) {
      const unsigned long long e = st[(sp - 1) * bs];
      if ((uint32_t)(e >> 48) > thr_key) {  // key16 is monotone: every remaining child has s > kd
        sp--;
        continue;
      }
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
      found = true;
      break;
    }
    if (!found) break;
  }
  return cnt;
}

// This thread's columns of the block's LDS: the stack (levels entries), the list's d2 and positions.
struct KnnLds {
  unsigned long long* st;
  double* ld;
  int32_t* lp;
};
__device__ __forceinline__ KnnLds knn_lds(unsigned long long* lds, int levels, int k) {
  const int bs = blockDim.x;
  KnnLds l;
  l.st = lds + threadIdx.x;
  l.ld = reinterpret_cast<double*>(lds + (size_t)levels * bs) + threadIdx.x;
  l.lp = reinterpret_cast<int32_t*>(lds + (size_t)(levels + k) * bs) + threadIdx.x;
  return l;
}

}  // namespace dev

// The LDS of a block of bs threads (knn_block_threads owns bs): the stacks, then the lists.
inline size_t knn_lds_bytes(int levels, int k, int bs) { return ((size_t)levels * 8 + (size_t)k * 12) * bs; }

}  // namespace icp
