// voxel_kernels.hip — voxel-grid down-sampling on the device (the definition and
// its host statement: voxel_host.h). Five phases on one stream:
//   1. bounds  per-axis minimum of the cloud and the count of non-finite coordinates (block parts,
//              then one block over the parts: min and an integer count, so the route does not show)
//   2. keys    one thread per point: key = cz << 42 | cy << 21 | cx, the identity permutation beside
//              it; the largest key and the out-of-range flags reduced per block, one atomicMax /
//              atomicOr per block (order-free: neither reaches an output)
//   3. sort    hipCUB radix sort of (key, index), stable: indices ascend inside a run of equal keys
//   4. runs    head flags, their exclusive sum, the run starts and the number of runs m
//   5. reduce  per run its count, first index and point (k_voxel_reduce)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

#include "kernels.h"
#include "voxel_host.h"
#include "wave_stats.h"

namespace icp {

namespace {

constexpr int kBoundsBlocks = 1024;  // at most this many parts of phase 1

inline unsigned grid_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

// Phase 1a: the cloud as 3n doubles, grid-strided (coalesced); part b = (min x, min y, min z, bad).
__global__ void __launch_bounds__(256) k_voxel_bounds(const double* __restrict__ xyz, int64_t n3,
                                                      double* __restrict__ parts) {
  __shared__ double red[4][4];
  double lo0 = __builtin_inf(), lo1 = __builtin_inf(), lo2 = __builtin_inf();
  unsigned long long bad = 0;
  const int step = (int)(gridDim.x * blockDim.x);  // <= 2^18
  const int e0 = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  int a = e0 % 3;  // the axis of element e, kept without a 64-bit division per trip
  const int da = step % 3;
  for (int64_t e = e0; e < n3; e += step) {
    const double v = xyz[e];
    if (!finite_d(v)) bad++;
    else {
      lo0 = (a == 0 && v < lo0) ? v : lo0;
      lo1 = (a == 1 && v < lo1) ? v : lo1;
      lo2 = (a == 2 && v < lo2) ? v : lo2;
    }
    a += da;
    a = a >= 3 ? a - 3 : a;
  }
  double nb = (double)bad;  // < 2^53: exact
  for (int o = 32; o >= 1; o >>= 1) {
    const double a0 = __shfl_xor(lo0, o, 64), a1 = __shfl_xor(lo1, o, 64), a2 = __shfl_xor(lo2, o, 64);
    lo0 = a0 < lo0 ? a0 : lo0;
    lo1 = a1 < lo1 ? a1 : lo1;
    lo2 = a2 < lo2 ? a2 : lo2;
    nb += __shfl_xor(nb, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w][0] = lo0, red[w][1] = lo1, red[w][2] = lo2, red[w][3] = nb;
  __syncthreads();
  if (threadIdx.x < 4) {
    double v = red[0][threadIdx.x];
    for (int q = 1; q < 4; q++) {
      const double u = red[q][threadIdx.x];
      v = threadIdx.x == 3 ? v + u : (u < v ? u : v);
    }
    parts[4 * blockIdx.x + threadIdx.x] = v;
  }
}

// Phase 1b: one wave over the parts; the head's origin (a zero minimum is +0.0; the caller's origin
// as it is), the non-finite count, and the words phase 2 accumulates into cleared.
__global__ void __launch_bounds__(64) k_voxel_bounds_fin(const double* __restrict__ parts, int nparts, int use_origin,
                                                         VoxelOrigin og, VoxelHead* __restrict__ head) {
  double lo0 = __builtin_inf(), lo1 = __builtin_inf(), lo2 = __builtin_inf(), nb = 0.0;
  for (int b = threadIdx.x; b < nparts; b += 64) {
    const double a0 = parts[4 * b], a1 = parts[4 * b + 1], a2 = parts[4 * b + 2];
    lo0 = a0 < lo0 ? a0 : lo0;
    lo1 = a1 < lo1 ? a1 : lo1;
    lo2 = a2 < lo2 ? a2 : lo2;
    nb += parts[4 * b + 3];
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const double a0 = __shfl_xor(lo0, o, 64), a1 = __shfl_xor(lo1, o, 64), a2 = __shfl_xor(lo2, o, 64);
    lo0 = a0 < lo0 ? a0 : lo0;
    lo1 = a1 < lo1 ? a1 : lo1;
    lo2 = a2 < lo2 ? a2 : lo2;
    nb += __shfl_xor(nb, o, 64);
  }
  if (threadIdx.x == 0) {
    head->origin[0] = use_origin ? og.o[0] : lo0 + 0.0;
    head->origin[1] = use_origin ? og.o[1] : lo1 + 0.0;
    head->origin[2] = use_origin ? og.o[2] : lo2 + 0.0;
    head->n_bad = (unsigned long long)nb;
    head->max_key = 0;
    head->flags = 0;
    head->m = 0;
  }
}

// Phase 2: a point's key and its index. An out-of-range (or non-finite) cell sets a flag and
// contributes no bits: the host fails on the flag before anything reads such a key.
__global__ void __launch_bounds__(256) k_voxel_keys(const double* __restrict__ xyz, int64_t n, double h,
                                                    VoxelHead* head, uint64_t* __restrict__ keys,
                                                    int32_t* __restrict__ idx) {
  __shared__ unsigned long long rkey[4];
  __shared__ unsigned rflag[4];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long key = 0;
  unsigned flags = 0;
  if (i < n) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double q = floor((xyz[3 * i + a] - head->origin[a]) / h);
      if (!(q >= 0.0)) flags |= kVoxelBelow;
      else if (!(q < kVoxelCells)) flags |= kVoxelBeyond;
      else key |= (unsigned long long)q << (kVoxelCellBits * a);
    }
    keys[i] = key;
    idx[i] = (int32_t)i;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)key, o, 64), hi = __shfl_xor((unsigned)(key >> 32), o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    key = other > key ? other : key;
    flags |= __shfl_xor(flags, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) rkey[w] = key, rflag[w] = flags;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 4; q++) {
      key = rkey[q] > key ? rkey[q] : key;
      flags |= rflag[q];
    }
    atomicMax(&head->max_key, key);
    if (flags) atomicOr(&head->flags, flags);
  }
}

// Phase 4: the head of every run of equal keys ...
__global__ void k_voxel_heads(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// ... and, from the exclusive sum of the flags, run r's first slot in starts[r]; starts[m] = n.
// starts holds n + 1 entries (m <= n).
__global__ void k_voxel_starts(const int32_t* __restrict__ flag, const int32_t* __restrict__ pos, int64_t n,
                               int32_t* __restrict__ starts, VoxelHead* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) starts[pos[i]] = (int32_t)i;
  if (i == n - 1) {
    const int32_t m = pos[i] + flag[i];
    starts[m] = (int32_t)n;
    head->m = m;
  }
}

// The value of lane (l + N) mod 16 of the lane's row of 16 (DPP row_ror; which way the row turns
// does not matter to voxel_fold16 below).
template <int N>
__device__ __forceinline__ double row_rot(double x) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0x120 + N, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0x120 + N, 0xf, 0xf, false);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// The model's fold over a row of 16 lanes, w = 8, 4, 2, 1: lane l adds the value w lanes on (mod 16).
// After the step w every lane of the row holds a value of period w, so the lane w / 2 on and the
// lane w / 2 back hold the same bits, and lane 0 of the row ends with s_0 of voxel_fold (IEEE
// addition commutes). Every lane of the wave takes part (DPP reads no disabled lane).
__device__ __forceinline__ double voxel_fold16(double s) {
  s = s + row_rot<8>(s);
  s = s + row_rot<12>(s);
  s = s + row_rot<14>(s);
  s = s + row_rot<15>(s);
  return s;
}

// The model's fold over the wave: w = 32 by a half swap, w = 16 by a row swap (wave_stats.h), then
// the rows. Lane 0 ends with s_0.
__device__ __forceinline__ double voxel_fold64(double s) {
  double t = s;
  dev::swap_d<true>(s, t);
  s = s + t;
  t = s;
  dev::swap_d<false>(s, t);
  s = s + t;
  return voxel_fold16(s);
}

struct VoxelReduce {
  const double* xyz;      // the caller's cloud
  const int32_t* idx;     // sorted indices
  const int32_t* starts;  // m + 1 run starts
  const VoxelHead* head;  // the origin
  int64_t m;
  int mode;
  double* xyz_out;  // any of the three may be null
  int32_t* first_out;
  int32_t* count_out;
};

__device__ __forceinline__ void voxel_store(const VoxelReduce& a, int64_t r, int32_t first, int32_t cnt, double p0,
                                            double p1, double p2) {
  if (a.first_out) a.first_out[r] = first;
  if (a.count_out) a.count_out[r] = cnt;
  if (a.xyz_out) {
    a.xyz_out[3 * r] = p0;
    a.xyz_out[3 * r + 1] = p1;
    a.xyz_out[3 * r + 2] = p2;
  }
}

// Phase 5. A wave owns four consecutive runs, one per row of 16 lanes. When none of the four is
// longer than 16 points the rows work side by side: lane l of a row takes point l of its run and
// the row folds with w = 8..1. Otherwise the wave takes its runs one after the other, lane-strided
// over all 64 lanes (lane l sums points l, l + 64, ... in that order: n / 64 trips for a run of n)
// and folds with w = 32..1: for a run of at most 16 points that is the same bits. Coordinates are
// gathered through the sorted indices from the caller's cloud. Every branch around a fold is
// wave-uniform.
__global__ void __launch_bounds__(256) k_voxel_reduce(const VoxelReduce a) {
  const int lane = threadIdx.x & 63, row = lane >> 4, rl = lane & 15;
  const int64_t r0 = 4 * ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
  if (r0 >= a.m) return;
  const double o0 = a.head->origin[0], o1 = a.head->origin[1], o2 = a.head->origin[2];
  const int64_t r = r0 + row;
  const bool have = r < a.m;
  const int32_t st = have ? a.starts[r] : 0;
  const int32_t cnt = have ? a.starts[r + 1] - st : 0;
  const bool centroid = a.mode == ICP_VOXEL_CENTROID && a.xyz_out;

  if (dev::wballot(cnt > kVoxelPacked) == 0ull) {
    const bool in = rl < cnt;
    int32_t id = 0;
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (in && (centroid || rl == 0)) {
      id = a.idx[(int64_t)st + rl];
      const double* p = a.xyz + 3 * (int64_t)id;
      d0 = p[0], d1 = p[1], d2 = p[2];
    }
    if (!centroid) {  // the first point's own bits (or no point asked for)
      if (in && rl == 0) voxel_store(a, r, id, cnt, d0, d1, d2);
      return;
    }
    double s0 = 0.0 + (in ? d0 - o0 : 0.0), s1 = 0.0 + (in ? d1 - o1 : 0.0), s2 = 0.0 + (in ? d2 - o2 : 0.0);
    s0 = voxel_fold16(s0);
    s1 = voxel_fold16(s1);
    s2 = voxel_fold16(s2);
    if (in && rl == 0) {
      const double c = (double)cnt;
      voxel_store(a, r, id, cnt, o0 + s0 / c, o1 + s1 / c, o2 + s2 / c);
    }
    return;
  }

  for (int g = 0; g < 4; g++) {
    const int64_t gst = __shfl(st, 16 * g, 64);
    const int64_t gcnt = __shfl(cnt, 16 * g, 64);
    if (gcnt == 0) break;  // past the last run
    const int32_t* ix = a.idx + gst;
    if (!centroid) {
      if (lane == 0) {
        const int32_t id = ix[0];
        const double* p = a.xyz + 3 * (int64_t)id;
        voxel_store(a, r0 + g, id, (int32_t)gcnt, p[0], p[1], p[2]);
      }
      continue;
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int64_t i = lane;
    for (; i + 192 < gcnt; i += 256) {  // four trips' gathers in flight, added in trip order
      const double* p = a.xyz + 3 * (int64_t)ix[i];
      const double* q = a.xyz + 3 * (int64_t)ix[i + 64];
      const double* u = a.xyz + 3 * (int64_t)ix[i + 128];
      const double* v = a.xyz + 3 * (int64_t)ix[i + 192];
      const double p0 = p[0], p1 = p[1], p2 = p[2], q0 = q[0], q1 = q[1], q2 = q[2];
      const double u0 = u[0], u1 = u[1], u2 = u[2], v0 = v[0], v1 = v[1], v2 = v[2];
      s0 = s0 + (p0 - o0), s1 = s1 + (p1 - o1), s2 = s2 + (p2 - o2);
      s0 = s0 + (q0 - o0), s1 = s1 + (q1 - o1), s2 = s2 + (q2 - o2);
      s0 = s0 + (u0 - o0), s1 = s1 + (u1 - o1), s2 = s2 + (u2 - o2);
      s0 = s0 + (v0 - o0), s1 = s1 + (v1 - o1), s2 = s2 + (v2 - o2);
    }
    for (; i < gcnt; i += 64) {
      const double* p = a.xyz + 3 * (int64_t)ix[i];
      s0 = s0 + (p[0] - o0), s1 = s1 + (p[1] - o1), s2 = s2 + (p[2] - o2);
    }
    s0 = voxel_fold64(s0);
    s1 = voxel_fold64(s1);
    s2 = voxel_fold64(s2);
    if (lane == 0) {
      const double c = (double)gcnt;
      voxel_store(a, r0 + g, ix[0], (int32_t)gcnt, o0 + s0 / c, o1 + s1 / c, o2 + s2 / c);
    }
  }
}

}  // namespace

int voxel_bounds_parts(int64_t n) {
  const int64_t b = (3 * n + 1023) / 1024;  // about four coordinates per thread at least
  return (int)(b < 1 ? 1 : (b > kBoundsBlocks ? kBoundsBlocks : b));
}

hipError_t voxel_temp_bytes(int64_t n, size_t* bytes) {
  size_t sort_b = 0, scan_b = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                    (const int32_t*)nullptr, (int32_t*)nullptr, (int)n, 0, 64, nullptr);
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_b, (const int32_t*)nullptr, (int32_t*)nullptr, (int)n, nullptr);
  if (e != hipSuccess) return e;
  *bytes = sort_b > scan_b ? sort_b : scan_b;
  return hipSuccess;
}

hipError_t launch_voxel_bounds(const double* xyz, int64_t n, const double* origin, double* parts, VoxelHead* head,
                               hipStream_t s) {
  const int nparts = voxel_bounds_parts(n);
  VoxelOrigin og{{0.0, 0.0, 0.0}};
  if (origin)
    for (int a = 0; a < 3; a++) og.o[a] = origin[a];
  hipLaunchKernelGGL(k_voxel_bounds, dim3((unsigned)nparts), dim3(256), 0, s, xyz, 3 * n, parts);
  hipLaunchKernelGGL(k_voxel_bounds_fin, dim3(1), dim3(64), 0, s, parts, nparts, origin ? 1 : 0, og, head);
  return hipGetLastError();
}

hipError_t launch_voxel_keys(const double* xyz, int64_t n, double h, VoxelHead* head, uint64_t* keys, int32_t* idx,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_voxel_keys, dim3(grid_for(n, 256)), dim3(256), 0, s, xyz, n, h, head, keys, idx);
  return hipGetLastError();
}

hipError_t launch_voxel_sort(void* tmp, size_t tmp_bytes, const uint64_t* keys, uint64_t* keys_out, const int32_t* idx,
                             int32_t* idx_out, int64_t n, uint64_t max_key, hipStream_t s) {
  int end_bit = 1;  // the bits of the largest key, as the octree build sizes its sort
  while (end_bit < 64 && (max_key >> end_bit) != 0) end_bit++;
  return hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys, keys_out, idx, idx_out, (int)n, 0, end_bit, s);
}

hipError_t launch_voxel_runs(void* tmp, size_t tmp_bytes, const uint64_t* sorted_keys, int64_t n, int32_t* flag,
                             int32_t* pos, int32_t* starts, VoxelHead* head, hipStream_t s) {
  hipLaunchKernelGGL(k_voxel_heads, dim3(grid_for(n, 256)), dim3(256), 0, s, sorted_keys, n, flag);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, flag, pos, (int)n, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_voxel_starts, dim3(grid_for(n, 256)), dim3(256), 0, s, flag, pos, n, starts, head);
  return hipGetLastError();
}

hipError_t launch_voxel_reduce(const double* xyz, const int32_t* idx, const int32_t* starts, const VoxelHead* head,
                               int64_t m, int mode, double* xyz_out, int32_t* first_out, int32_t* count_out,
                               hipStream_t s) {
  const VoxelReduce a{xyz, idx, starts, head, m, mode, xyz_out, first_out, count_out};
  hipLaunchKernelGGL(k_voxel_reduce, dim3(grid_for(m, 16)), dim3(256), 0, s, a);  // 16 runs per block
  return hipGetLastError();
}

}  // namespace icp
