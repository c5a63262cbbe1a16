// voxel_host.h — voxel-grid down-sampling on the host, header only, no GPU
// (exported as icp_voxel_downsample; built alone under the sanitizers by `make voxel_asan`). The
// device path (voxel_kernels.hip, ctx_voxel.cpp) computes the same function bit for bit.
//
// Cells: c_a = floor((x_a - o_a) / h) in fp64 as written (one subtraction, one division, floor), o
// the caller's origin or the cloud's per-axis minimum; every c_a in [0, 2^21);
// key = cz << 42 | cy << 21 | cx. A voxel is a distinct key; voxels leave in ascending key order and
// a voxel's points are taken in ascending original index. Per voxel: count, first (its lowest
// index) and the point: the coordinates of `first` (ICP_VOXEL_FIRST), or o + s_0 / count
// (ICP_VOXEL_CENTROID) with d_i = x_i - o over the voxel's points i = 0..count-1, the 64 partials
// s_l = +0.0 + d_l + d_{l+64} + ... and the fold s_l += s_{l+w}, w = 32, 16, 8, 4, 2, 1. Absent
// lanes are +0.0 and adding them is exact, so 16 lanes folded with w = 8..1 give the same bits
// whenever count <= 16: the one freedom an implementation has (and this one takes).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/icp_hip.h"

namespace icp {

constexpr int kVoxelCellBits = 21;
constexpr double kVoxelCells = 2097152.0;  // 2^21 cells per axis
constexpr int kVoxelLanes = 64;            // partial sums of a voxel
constexpr int kVoxelPacked = 16;           // a voxel of at most this many points: 16 lanes do
// what went wrong with a cell index (the flag word of the device's key pass)
constexpr unsigned kVoxelBelow = 1u, kVoxelBeyond = 2u;

inline bool voxel_finite(double v) { return v - v == 0.0; }

// The checks that need no point: EINVAL with the reason in *why, or ICP_HIP_OK.
inline int voxel_check_args(int64_t n, double h, const double* origin, int mode, std::string* why) {
  if (!(voxel_finite(h) && h > 0.0)) return *why = "voxel_downsample: the voxel edge must be finite and > 0", ICP_HIP_EINVAL;
  if (n < 1 || n > (int64_t)0x7fffffff) return *why = "voxel_downsample: n outside [1, 2^31 - 1]", ICP_HIP_EINVAL;
  if (mode != ICP_VOXEL_CENTROID && mode != ICP_VOXEL_FIRST) return *why = "voxel_downsample: unknown mode", ICP_HIP_EINVAL;
  if (origin)
    for (int a = 0; a < 3; a++)
      if (!voxel_finite(origin[a])) return *why = "voxel_downsample: non-finite origin", ICP_HIP_EINVAL;
  return ICP_HIP_OK;
}

inline std::string voxel_nonfinite_text(uint64_t count) {
  return "voxel_downsample: " + std::to_string(count) + " non-finite coordinates";
}

inline std::string voxel_range_text(unsigned flags) {
  return flags & kVoxelBelow ? "voxel_downsample: a point lies below the caller's origin (cell index < 0)"
                             : "voxel_downsample: the grid is too fine for the extent (cell index >= 2^21)";
}

inline std::string voxel_cap_text(int64_t m, int64_t cap) {
  return "voxel_downsample: " + std::to_string(m) + " voxels exceed the outputs' capacity " + std::to_string(cap);
}

// The fold of L (64 or 16) partials into s[0].
inline void voxel_fold(double* s, int L) {
  for (int w = L / 2; w >= 1; w >>= 1)
    for (int l = 0; l < w; l++) s[l] = s[l] + s[l + w];
}

struct VoxelKeyed {
  uint64_t key;
  int32_t idx;
};

// The whole function. Returns ICP_HIP_OK or ICP_HIP_EINVAL (the reason in *why); *m_out is the
// number of voxels whenever the cells were valid (also when m > cap refused the outputs, which are
// then untouched). Any of the three outputs may be null; all null: count only.
inline int voxel_downsample_host(const double* xyz, int64_t n, double h, const double* origin, int mode, int64_t cap,
                                 double* xyz_out, int32_t* first_out, int32_t* count_out, int64_t* m_out,
                                 double origin_out[3], std::string* why) {
  *m_out = 0;
  if (const int rc = voxel_check_args(n, h, origin, mode, why)) return rc;
  if (!xyz) return *why = "voxel_downsample: null cloud", ICP_HIP_EINVAL;
  double o[3] = {INFINITY, INFINITY, INFINITY};
  uint64_t bad = 0;
  for (int64_t i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) {
      const double v = xyz[3 * i + a];
      if (!voxel_finite(v)) bad++;
      else if (v < o[a]) o[a] = v;
    }
  if (bad) return *why = voxel_nonfinite_text(bad), ICP_HIP_EINVAL;
  for (int a = 0; a < 3; a++) o[a] = origin ? origin[a] : o[a] + 0.0;  // a zero minimum is +0.0
  if (origin_out)
    for (int a = 0; a < 3; a++) origin_out[a] = o[a];

  std::vector<VoxelKeyed> ks((size_t)n);
  unsigned flags = 0;
  for (int64_t i = 0; i < n; i++) {
    uint64_t key = 0;
    for (int a = 0; a < 3; a++) {
      const double q = std::floor((xyz[3 * i + a] - o[a]) / h);
      if (!(q >= 0.0)) flags |= kVoxelBelow;
      else if (!(q < kVoxelCells)) flags |= kVoxelBeyond;
      else key |= (uint64_t)q << (kVoxelCellBits * a);
    }
    ks[(size_t)i] = {key, (int32_t)i};
  }
  if (flags) return *why = voxel_range_text(flags), ICP_HIP_EINVAL;
  std::sort(ks.begin(), ks.end(),
            [](const VoxelKeyed& p, const VoxelKeyed& q) { return p.key != q.key ? p.key < q.key : p.idx < q.idx; });

  int64_t m = 1;
  for (int64_t i = 1; i < n; i++) m += ks[(size_t)i].key != ks[(size_t)i - 1].key;
  *m_out = m;
  if (!xyz_out && !first_out && !count_out) return ICP_HIP_OK;
  if (m > cap) return *why = voxel_cap_text(m, cap), ICP_HIP_EINVAL;

  int64_t r = 0;
  for (int64_t st = 0; st < n; r++) {
    int64_t en = st + 1;
    while (en < n && ks[(size_t)en].key == ks[(size_t)st].key) en++;
    const int64_t cnt = en - st;
    const int32_t first = ks[(size_t)st].idx;
    if (first_out) first_out[r] = first;
    if (count_out) count_out[r] = (int32_t)cnt;
    if (xyz_out && mode == ICP_VOXEL_FIRST) {
      for (int a = 0; a < 3; a++) xyz_out[3 * r + a] = xyz[3 * (int64_t)first + a];
    } else if (xyz_out) {
      const int L = cnt <= kVoxelPacked ? kVoxelPacked : kVoxelLanes;
      double s[3][kVoxelLanes];
      for (int a = 0; a < 3; a++)
        for (int l = 0; l < L; l++) s[a][l] = 0.0;
      for (int64_t j = 0; j < cnt; j++) {
        const double* p = xyz + 3 * (int64_t)ks[(size_t)(st + j)].idx;
        const int l = (int)(j & (kVoxelLanes - 1));
        for (int a = 0; a < 3; a++) s[a][l] = s[a][l] + (p[a] - o[a]);
      }
      for (int a = 0; a < 3; a++) {
        voxel_fold(s[a], L);
        xyz_out[3 * r + a] = o[a] + s[a][0] / (double)cnt;
      }
    }
    st = en;
  }
  return ICP_HIP_OK;
}

}  // namespace icp
