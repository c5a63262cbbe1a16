// las_kernels.hip — LAS point records decoded and encoded on the device (include/icp_las.h, the
// icp_hip_*_las calls; host side: ctx_las.cpp). The arithmetic is the host reader's and writers'
// (lasio.cpp) operation by operation: x = X * scale + offset as one multiply and one add,
// X = (int32)((x - offset) / scale) as one subtract, one IEEE division and a truncation. The
// explicit _rn intrinsics are never contracted, whatever the compiler's fp-contract setting.
#include <hip/hip_runtime.h>

#include "las_kernels.h"

namespace icp {

namespace {

constexpr int kBlock = 256;
// Decode, staged path: a block's records span at most 255 * kStageStep + 12 bytes, plus up to 15 in
// front of them (the span starts at a 16-byte boundary) and the 16-byte granule's tail behind.
constexpr int kStageStep = 128;  // stride * record_length up to which a block stages its whole span
constexpr int kStageBytes = 255 * kStageStep + 12 + 15 + 16;
constexpr int kStageWords = (kStageBytes + 3) / 4 + 4;  // + the word pair a 4-byte-aligned record never uses

// Three consecutive little-endian int32 from four consecutive words, starting sh bits into w0.
__device__ __forceinline__ void take3(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, unsigned sh, int32_t v[3]) {
  v[0] = (int32_t)__funnelshift_r(w0, w1, sh);
  v[1] = (int32_t)__funnelshift_r(w1, w2, sh);
  v[2] = (int32_t)__funnelshift_r(w2, w3, sh);
}

__device__ __forceinline__ void store_point(double* out, int64_t s, const int32_t v[3], const LasAxes& ax) {
  double* p = out + 3 * s;
  for (int a = 0; a < 3; a++) p[a] = __dadd_rn(__dmul_rn((double)v[a], ax.scale[a]), ax.offset[a]);
}

// Record j0 + s * stride of the chunk becomes point s of `out`, s < sel. raw is the chunk's first
// record, at any byte address; its allocation ends on a 16-byte boundary at or after the last byte.
__global__ __launch_bounds__(kBlock) void k_las_decode_staged(const uint8_t* raw, int64_t step, int64_t first_byte,
                                                               int64_t sel, double* out, LasAxes ax) {
  __shared__ uint4 stage4[(kStageWords + 3) / 4];
  uint32_t* stage = reinterpret_cast<uint32_t*>(stage4);
  const int64_t s0 = (int64_t)blockIdx.x * kBlock;
  const int64_t cnt = sel - s0 < kBlock ? sel - s0 : kBlock;  // > 0: the grid covers sel exactly
  // the block's bytes: from its first record's first byte to its last record's twelfth
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(raw) + (uintptr_t)(first_byte + s0 * step);
  const uintptr_t a1 = a0 + (uintptr_t)((cnt - 1) * step + 12);
  const uintptr_t lo = a0 & ~(uintptr_t)15;
  const int n16 = (int)((a1 - lo + 15) / 16);  // every granule holds a byte of [a0, a1)
  const uint4* src = reinterpret_cast<const uint4*>(lo);
  for (int k = threadIdx.x; k < n16; k += kBlock) stage4[k] = src[k];
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= cnt) return;
  const unsigned o = (unsigned)(a0 - lo) + (unsigned)(t * step);
  const unsigned w = o >> 2, sh = (o & 3u) * 8u;
  int32_t v[3];
  take3(stage[w], stage[w + 1], stage[w + 2], stage[w + 3], sh, v);  // sh = 0 ignores the fourth word
  store_point(out, s0 + t, v, ax);
}

// The same for steps too long to stage: each thread loads the aligned words that hold its record's
// twelve bytes, and nothing else of the span.
__global__ __launch_bounds__(kBlock) void k_las_decode_direct(const uint8_t* raw, int64_t step, int64_t first_byte,
                                                               int64_t sel, double* out, LasAxes ax) {
  const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= sel) return;
  const uintptr_t a = reinterpret_cast<uintptr_t>(raw) + (uintptr_t)(first_byte + s * step);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const unsigned sh = (unsigned)(a & 3u) * 8u;
  const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
  const uint32_t w3 = sh ? q[3] : 0u;  // an aligned record ends with its third word
  int32_t v[3];
  take3(w0, w1, w2, w3, sh, v);
  store_point(out, s, v, ax);
}

// "Keep the left value unless the right one is strictly smaller / greater": the host loops' update
// (lasio.cpp), associative on ordered values, so partials combined in index order give the
// sequential result, the survivor of -0.0 and +0.0 included.
struct Bounds6 {
  double mn[3], mx[3];
};

__device__ __forceinline__ void fold(Bounds6& l, const Bounds6& r) {
  for (int a = 0; a < 3; a++) {
    if (r.mn[a] < l.mn[a]) l.mn[a] = r.mn[a];
    if (r.mx[a] > l.mx[a]) l.mx[a] = r.mx[a];
  }
}

// One wave per kBoundsRun consecutive points, 64 at a time: a shuffle tree in lane order, then lane
// 0 folds the tile into its running bounds. parts[wave] = {min xyz, max xyz}; the host folds the
// parts in order. Lanes past the cloud's end repeat its last point (a repeat changes nothing).
__global__ __launch_bounds__(kBlock) void k_las_bounds(const double* xyz, int64_t n, double* parts) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
  const int64_t p0 = wave * kBoundsRun;
  if (p0 >= n) return;  // whole waves only: no lane of a live wave leaves before the shuffles
  Bounds6 acc;
  for (int64_t t = p0; t < p0 + kBoundsRun && t < n; t += 64) {
    const int64_t i = t + lane < n ? t + lane : n - 1;
    Bounds6 b;
    for (int a = 0; a < 3; a++) b.mn[a] = b.mx[a] = xyz[3 * i + a];
    for (int off = 1; off < 64; off <<= 1) {
      Bounds6 r;
      for (int a = 0; a < 3; a++) {
        r.mn[a] = __shfl_down(b.mn[a], off, 64);
        r.mx[a] = __shfl_down(b.mx[a], off, 64);
      }
      if (lane + off < 64) fold(b, r);  // left: lanes [lane, lane + off), right: the next off lanes
    }
    if (t == p0) acc = b;
    else fold(acc, b);
  }
  if (lane == 0)
    for (int a = 0; a < 3; a++) {
      parts[6 * wave + a] = acc.mn[a];
      parts[6 * wave + 3 + a] = acc.mx[a];
    }
}

__device__ __forceinline__ double quotient(double v, double off, double scale) {
  return __ddiv_rn(__dsub_rn(v, off), scale);
}

// Coordinates the device must not encode: non-finite ones and quotients outside int32, where the
// host's cast gives what x86's conversion gives and the device's saturates. One add per wave.
__global__ __launch_bounds__(kBlock) void k_las_count_unencodable(const double* xyz, int64_t n, LasAxes ax,
                                                                   unsigned long long* count) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int bad = 0;
  if (i < n)
    for (int a = 0; a < 3; a++) {
      const double q = quotient(xyz[3 * i + a], ax.offset[a], ax.scale[a]);
      bad += !(q > -2147483649.0 && q < 2147483648.0);  // NaN and the infinities fail both
    }
  for (int off = 32; off > 0; off >>= 1) bad += __shfl_down(bad, off, 64);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(count, (unsigned long long)bad);
}

// Points [0, n) of xyz as 20-byte records: X, Y, Z, then 8 zero bytes (point format 0's other fields).
__global__ __launch_bounds__(kBlock) void k_las_encode(const double* xyz, int64_t n, LasAxes ax, uint32_t* rec) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t* r = rec + 5 * i;
  for (int a = 0; a < 3; a++) r[a] = (uint32_t)(int32_t)quotient(xyz[3 * i + a], ax.offset[a], ax.scale[a]);
  r[3] = 0u;
  r[4] = 0u;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

hipError_t launch_las_decode(const uint8_t* raw, int record_length, int64_t stride, int64_t j0, int64_t sel, double* out,
                             const LasAxes& ax, hipStream_t s) {
  if (sel <= 0) return hipSuccess;
  const int64_t step = stride * record_length;
  const int64_t first_byte = j0 * record_length;
  if (step <= kStageStep)
    hipLaunchKernelGGL(k_las_decode_staged, dim3(blocks_for(sel)), dim3(kBlock), 0, s, raw, step, first_byte, sel, out, ax);
  else
    hipLaunchKernelGGL(k_las_decode_direct, dim3(blocks_for(sel)), dim3(kBlock), 0, s, raw, step, first_byte, sel, out, ax);
  return hipGetLastError();
}

int64_t las_bounds_parts(int64_t n) { return (n + kBoundsRun - 1) / kBoundsRun; }

hipError_t launch_las_bounds(const double* xyz, int64_t n, double* parts, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_las_bounds, dim3(blocks_for(las_bounds_parts(n) * 64)), dim3(kBlock), 0, s, xyz, n, parts);
  return hipGetLastError();
}

hipError_t launch_las_count_unencodable(const double* xyz, int64_t n, const LasAxes& ax, unsigned long long* count,
                                        hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_las_count_unencodable, dim3(blocks_for(n)), dim3(kBlock), 0, s, xyz, n, ax, count);
  return hipGetLastError();
}

hipError_t launch_las_encode(const double* xyz, int64_t n, const LasAxes& ax, uint32_t* rec, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_las_encode, dim3(blocks_for(n)), dim3(kBlock), 0, s, xyz, n, ax, rec);
  return hipGetLastError();
}

}  // namespace icp
