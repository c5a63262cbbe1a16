// query_order_gpu.hip — the kd query order of query_order.cpp, built on the device.
//
// The host partition splits a range of n > bucket queries at h = n/2 rounded up to a multiple of
// 64 (of `bucket` inside a wave's 64; h = n - unit when that reaches n), on the longest axis of the
// range's bounding box, with nth_element. The split positions depend on the sizes only, so every
// level of the recursion is a fixed list of segments: the host lays the segments out level by
// level (a level holds every segment, in position order; the last level is the last one in which a
// segment still splits).
//
// Coordinates. Keys and boxes are fp32, but of the coordinate relative to one origin per cloud:
//   c(v, a) = (float)((finite(v) ? v : 0.0) - origin[a]) + 0.0f,   the subtraction in fp64,
// so that a georeferenced cloud (|v| ~ 5e6, fp32 ulp 0.5 m) keeps the resolution of its extent. A
// non-finite coordinate counts as 0, as on the host. The + 0.0f makes a zero +0.0: coordinates
// that compare equal (-0.0 and +0.0) get one key, as they tie on the host. The origin is taken
// once, before the first level, from a strided sample: stride = ceil(n / 1024), the points 0,
// stride, 2 stride, ... (at most 1024 of them); per axis the finite sample values sorted ascending,
// origin[a] = the value at index count / 2, or 0.0 when no sample value is finite (the sign of a
// zero origin does not reach c). A median, not a box corner or a mean:
// a few far outliers in the cloud (or in a segment) do not move it, and the bulk keeps its
// resolution. The origin is per cloud, not per segment.
//
// Per level the device
//   1. takes each splitting segment's bounding box over c (one workgroup per segment; segments
//      larger than kChunk slots from chunk boxes: min and max are exact, so the route does not
//      show) and picks its longest axis: extent hi - lo in fp32, the largest wins, ties go to the
//      lower axis (the host's strict > scan);
//   2. keys every slot with (segment start << 32 | k), k = the order-preserving image of the bits
//      of c on the segment's axis (sign bit set: all bits flipped, else the sign bit set), and
//      radix-sorts the permutation by it (hipCUB, stable): every segment
//      ends up sorted along its axis, ties in the order the previous level left, so its first h
//      queries are its h smallest, which is what nth_element guarantees.
// Finished segments (size <= bucket) keep their place and their order: their key is their start
// alone (k = 0). The first level starts from the identity. ~20 levels at 10M. Any kd partition
// gives the same correspondences (the search is exact); this one has the host order's bucket
// geometry.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "dev_scratch.h"
#include "query_order.h"

namespace icp {

namespace {

struct Origin {
  double o[3];
};

// the fp32 coordinate relative to the cloud's origin (non-finite: 0; a zero result: +0.0)
__device__ __forceinline__ float coord32(double v, double o) {
  return (float)((__builtin_isfinite(v) ? v : 0.0) - o) + 0.0f;
}

constexpr int kOriginSample = 1024;
constexpr uint8_t kNoAxis = 3;  // a finished segment: no key

// The strided sample the origin is the median of.
__global__ void k_sample(const double* __restrict__ xyz, int64_t stride, int m, double* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  for (int a = 0; a < 3; a++) out[3 * k + a] = xyz[3 * (k * stride) + a];
}

__device__ __forceinline__ uint32_t okey(float f) {  // order-preserving (non-NaN floats)
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

constexpr int32_t kChunk = 16384;  // segments larger than this take their box from chunks

// block-wide min/max of 3 lo + 3 hi floats into red[6][blockDim/64]; thread 0 gets the results
__device__ __forceinline__ void block_box(float lo[3], float hi[3], float (*red)[4]) {
#pragma unroll
  for (int a = 0; a < 3; a++) {
    for (int o = 32; o >= 1; o >>= 1) {
      const float l = __shfl_xor(lo[a], o, 64), h = __shfl_xor(hi[a], o, 64);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
    for (int a = 0; a < 3; a++) {
      red[a][w] = lo[a];
      red[3 + a][w] = hi[a];
    }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = blockDim.x >> 6;
    for (int a = 0; a < 3; a++) {
      float l = red[a][0], h = red[3 + a][0];
      for (int q = 1; q < nw; q++) {
        l = red[a][q] < l ? red[a][q] : l;
        h = red[3 + a][q] > h ? red[3 + a][q] : h;
      }
      lo[a] = l;
      hi[a] = h;
    }
  }
}

__device__ __forceinline__ uint8_t longest_axis(const float lo[3], const float hi[3]) {
  int ax = 0;
  for (int a = 1; a < 3; a++)
    if (hi[a] - lo[a] > hi[ax] - lo[ax]) ax = a;
  return (uint8_t)ax;
}

// Big segments: the box of each chunk of kChunk slots (one workgroup each) ...
__global__ void __launch_bounds__(256) k_chunk_bbox(const double* __restrict__ xyz, const int32_t* __restrict__ perm,
                                                    const int32_t* __restrict__ cstart, const int32_t* __restrict__ clen,
                                                    Origin og, float* __restrict__ cbox) {
  __shared__ float red[6][4];
  const int c = blockIdx.x;
  const int32_t s0 = cstart[c], n = clen[c];
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int32_t k = threadIdx.x; k < n; k += blockDim.x) {
    const int64_t j = perm[s0 + k];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float v = coord32(xyz[3 * j + a], og.o[a]);
      lo[a] = v < lo[a] ? v : lo[a];
      hi[a] = v > hi[a] ? v : hi[a];
    }
  }
  block_box(lo, hi, red);
  if (threadIdx.x == 0)
    for (int a = 0; a < 3; a++) {
      cbox[6 * c + a] = lo[a];
      cbox[6 * c + 3 + a] = hi[a];
    }
}

// ... then each big segment's axis from its chunks' boxes (one thread per big segment).
__global__ void k_big_axis(const float* __restrict__ cbox, const int32_t* __restrict__ bseg,
                           const int32_t* __restrict__ bfirst, int nbig, uint8_t* __restrict__ axis) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nbig) return;
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int c = bfirst[b]; c < bfirst[b + 1]; c++)
    for (int a = 0; a < 3; a++) {
      lo[a] = cbox[6 * c + a] < lo[a] ? cbox[6 * c + a] : lo[a];
      hi[a] = cbox[6 * c + 3 + a] > hi[a] ? cbox[6 * c + 3 + a] : hi[a];
    }
  axis[bseg[b]] = longest_axis(lo, hi);
}

// One workgroup per segment: the longest axis of its bounding box (ties: the lower axis, as the
// host's strict > scan).
__global__ void __launch_bounds__(256) k_seg_axis(const double* __restrict__ xyz, const int32_t* __restrict__ perm,
                                                  const int32_t* __restrict__ starts,
                                                  const int32_t* __restrict__ sizes, int bucket, Origin og,
                                                  uint8_t* __restrict__ axis) {
  __shared__ float red[6][4];
  const int seg = blockIdx.x;
  const int32_t s0 = starts[seg], sz = sizes[seg];
  if (sz > kChunk) return;  // a big segment: the chunk path (k_chunk_bbox, k_big_axis)
  if (sz <= bucket) {  // finished: never split again
    if (threadIdx.x == 0) axis[seg] = kNoAxis;
    return;
  }
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int32_t k = threadIdx.x; k < sz; k += blockDim.x) {
    const int64_t j = perm[s0 + k];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float v = coord32(xyz[3 * j + a], og.o[a]);
      lo[a] = v < lo[a] ? v : lo[a];
      hi[a] = v > hi[a] ? v : hi[a];
    }
  }
  block_box(lo, hi, red);
  if (threadIdx.x == 0) axis[seg] = longest_axis(lo, hi);
}

// Sort key of every slot: its segment's start (high word) and its coordinate on that segment's axis
// (a finished segment: the start alone).
__global__ void k_seg_keys(const double* __restrict__ xyz, const int32_t* __restrict__ perm,
                           const int32_t* __restrict__ starts, int nseg, const uint8_t* __restrict__ axis,
                           Origin og, int64_t n, uint64_t* __restrict__ keys) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  int lo = 0, hi = nseg;  // the last segment with start <= k
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (starts[mid] <= k) lo = mid;
    else hi = mid;
  }
  const int ax = axis[lo];
  uint32_t low = 0;
  if (ax != kNoAxis) {
    const int64_t j = perm[k];
    low = okey(coord32(xyz[3 * j + ax], og.o[ax]));
  }
  keys[k] = ((uint64_t)(uint32_t)starts[lo] << 32) | low;
}

__global__ void k_iota(int32_t* p, int64_t n) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) p[k] = (int32_t)k;
}

inline unsigned grid_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// The host recursion's split position (query_order.cpp: multiples of 64 while the range is
// larger than a wave, of `bucket` inside it).
inline int64_t split_at(int64_t n, int bucket) {
  const int64_t unit = n > 64 ? 64 : bucket;
  int64_t h = ((n / 2 + unit - 1) / unit) * unit;
  if (h >= n) h = n - unit;
  return h;
}

#define QO_TRY(expr)                  \
  do {                                \
    hipError_t e_ = (expr);           \
    if (e_ != hipSuccess) return e_;  \
  } while (0)

// The cloud's origin (header comment): per axis the median of the finite coordinates of a strided
// sample of at most kOriginSample points. d_sample: 3 * kOriginSample doubles. Synchronises s.
hipError_t cloud_origin(const double* d_xyz, int64_t n, double* d_sample, hipStream_t s, Origin* og) {
  const int64_t stride = (n + kOriginSample - 1) / kOriginSample;
  const int m = (int)((n + stride - 1) / stride);
  std::vector<double> h(3 * (size_t)m);
  hipLaunchKernelGGL(k_sample, dim3(grid_for(m, 256)), dim3(256), 0, s, d_xyz, stride, m, d_sample);
  QO_TRY(hipGetLastError());
  QO_TRY(hipMemcpyAsync(h.data(), d_sample, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  QO_TRY(hipStreamSynchronize(s));
  std::vector<double> v;
  v.reserve((size_t)m);
  for (int a = 0; a < 3; a++) {
    v.clear();
    for (int k = 0; k < m; k++)
      if (std::isfinite(h[3 * (size_t)k + a])) v.push_back(h[3 * (size_t)k + a]);
    std::sort(v.begin(), v.end());
    og->o[a] = v.empty() ? 0.0 : v[v.size() / 2];
  }
  return hipSuccess;
}

}  // namespace

hipError_t gpu_kd_query_order(const double* d_xyz, int64_t n, int bucket, int32_t* d_perm, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (n > 0x7fffffff || bucket < 1 || 64 % bucket != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_iota, dim3(grid_for(n, 256)), dim3(256), 0, s, d_perm, n);
  if (n <= bucket) return hipGetLastError();
  // the levels of the recursion: every segment, in position order
  std::vector<std::vector<int32_t>> lv_start, lv_size;
  {
    std::vector<int32_t> st{0}, sz{(int32_t)n};
    while (true) {
      bool splits = false;
      for (int32_t v : sz) splits = splits || v > bucket;
      if (!splits) break;
      lv_start.push_back(st);
      lv_size.push_back(sz);
      std::vector<int32_t> st2, sz2;
      st2.reserve(st.size() * 2);
      sz2.reserve(st.size() * 2);
      for (size_t k = 0; k < st.size(); k++) {
        if (sz[k] > bucket) {
          const int32_t h = (int32_t)split_at(sz[k], bucket);
          st2.push_back(st[k]);
          sz2.push_back(h);
          st2.push_back(st[k] + h);
          sz2.push_back(sz[k] - h);
        } else {
          st2.push_back(st[k]);
          sz2.push_back(sz[k]);
        }
      }
      st.swap(st2);
      sz.swap(sz2);
    }
  }
  size_t max_seg = 0;
  for (const auto& v : lv_start) max_seg = std::max(max_seg, v.size());
  DevScratch S;  // every level ends synchronised; a failed one leaves the wait to the release
  int32_t *d_starts = nullptr, *d_sizes = nullptr, *perm_alt = nullptr;
  uint8_t* d_axis = nullptr;
  uint64_t *keys = nullptr, *keys_alt = nullptr;
  uint8_t* d_chunks = nullptr;  // chunk boxes + chunk / big-segment tables
  size_t chunk_cap = 0;
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
  int sbits = 1;
  while (((int64_t)1 << sbits) <= n) sbits++;
  const int end_bit = 32 + sbits;
  QO_TRY(S.alloc(&d_starts, max_seg));
  QO_TRY(S.alloc(&d_sizes, max_seg));
  QO_TRY(S.alloc(&d_axis, max_seg));
  QO_TRY(S.alloc(&perm_alt, (size_t)n));
  QO_TRY(S.alloc(&keys, (size_t)n));
  QO_TRY(S.alloc(&keys_alt, (size_t)n));
  QO_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys, keys_alt, d_perm, perm_alt, (int)n, 0,
                                            end_bit, s));
  QO_TRY(S.alloc(&tmp, tmp_bytes));
  double* d_sample = nullptr;
  QO_TRY(S.alloc(&d_sample, 3 * (size_t)kOriginSample));
  Origin og;
  QO_TRY(cloud_origin(d_xyz, n, d_sample, s, &og));
  for (size_t L = 0; L < lv_start.size(); L++) {
    const int nseg = (int)lv_start[L].size();
    QO_TRY(hipMemcpyAsync(d_starts, lv_start[L].data(), nseg * sizeof(int32_t), hipMemcpyHostToDevice, s));
    QO_TRY(hipMemcpyAsync(d_sizes, lv_size[L].data(), nseg * sizeof(int32_t), hipMemcpyHostToDevice, s));
    {
      // big segments (the top levels): their boxes from chunks of kChunk slots, many workgroups each
      std::vector<int32_t> cst, cln, bseg, bfirst{0};
      for (int k = 0; k < nseg; k++) {
        if (lv_size[L][k] <= kChunk) continue;
        for (int32_t o = 0; o < lv_size[L][k]; o += kChunk) {
          cst.push_back(lv_start[L][k] + o);
          cln.push_back(std::min(kChunk, lv_size[L][k] - o));
        }
        bseg.push_back(k);
        bfirst.push_back((int32_t)cst.size());
      }
      if (!bseg.empty()) {
        const size_t nc = cst.size(), nb = bseg.size();
        if (nc > chunk_cap) {
          chunk_cap = nc;
          QO_TRY(S.regrow(&d_chunks, chunk_cap * (6 * sizeof(float) + 3 * sizeof(int32_t)) + 2 * sizeof(int32_t)));
        }
        float* cbox = reinterpret_cast<float*>(d_chunks);
        int32_t* ci = reinterpret_cast<int32_t*>(cbox + 6 * chunk_cap);
        QO_TRY(hipMemcpyAsync(ci, cst.data(), nc * sizeof(int32_t), hipMemcpyHostToDevice, s));
        QO_TRY(hipMemcpyAsync(ci + chunk_cap, cln.data(), nc * sizeof(int32_t), hipMemcpyHostToDevice, s));
        QO_TRY(hipMemcpyAsync(ci + 2 * chunk_cap, bseg.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice, s));
        QO_TRY(hipMemcpyAsync(ci + 2 * chunk_cap + nb, bfirst.data(), (nb + 1) * sizeof(int32_t),
                              hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_chunk_bbox, dim3((unsigned)nc), dim3(256), 0, s, d_xyz, d_perm, ci, ci + chunk_cap, og, cbox);
        hipLaunchKernelGGL(k_big_axis, dim3(grid_for((int64_t)nb, 64)), dim3(64), 0, s, cbox, ci + 2 * chunk_cap,
                           ci + 2 * chunk_cap + nb, (int)nb, d_axis);
        QO_TRY(hipGetLastError());
        QO_TRY(hipStreamSynchronize(s));  // the host tables are read by the copies above
      }
    }
    const int32_t big = *std::max_element(lv_size[L].begin(), lv_size[L].end());
    const int bs = big <= 128 ? 64 : 256;  // deep levels: one wave per (small) segment
    hipLaunchKernelGGL(k_seg_axis, dim3((unsigned)nseg), dim3(bs), 0, s, d_xyz, d_perm, d_starts, d_sizes, bucket,
                       og, d_axis);
    hipLaunchKernelGGL(k_seg_keys, dim3(grid_for(n, 256)), dim3(256), 0, s, d_xyz, d_perm, d_starts, nseg, d_axis, og,
                       n, keys);
    QO_TRY(hipGetLastError());
    QO_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, keys, keys_alt, d_perm, perm_alt, (int)n, 0, end_bit,
                                              s));
    QO_TRY(hipMemcpyAsync(d_perm, perm_alt, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    // the host tables of this level are read by the copies above: finish before they are reused
    QO_TRY(hipStreamSynchronize(s));
  }
  return hipSuccess;
}

}  // namespace icp
