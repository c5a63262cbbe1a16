// las_kernels.h — launches of las_kernels.hip (LAS records decoded / encoded on the device).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace icp {

struct LasAxes {
  double scale[3];
  double offset[3];
};

constexpr int64_t kBoundsRun = 1024;  // consecutive points per wave of the bounds reduction

// Records j0, j0 + stride, ... (sel of them) of a chunk whose first record is at raw become points
// [0, sel) of out (AoS xyz fp64): X * scale + offset from the int32 at record bytes 0, 4, 8. raw
// may have any alignment; the 16-byte granules that hold the records' bytes must be readable.
hipError_t launch_las_decode(const uint8_t* raw, int record_length, int64_t stride, int64_t j0, int64_t sel, double* out,
                             const LasAxes& ax, hipStream_t s);

// Min and max per axis of consecutive runs of kBoundsRun points, in index order:
// parts[6 k] = {min x, y, z, max x, y, z} of run k, las_bounds_parts(n) runs.
int64_t las_bounds_parts(int64_t n);
hipError_t launch_las_bounds(const double* xyz, int64_t n, double* parts, hipStream_t s);

// Adds to *count the coordinates whose (v - offset) / scale is not a finite value inside int32.
hipError_t launch_las_count_unencodable(const double* xyz, int64_t n, const LasAxes& ax, unsigned long long* count,
                                        hipStream_t s);

// n points as 20-byte records (5 words each): (int32)((v - offset) / scale) x 3, then zeros.
hipError_t launch_las_encode(const double* xyz, int64_t n, const LasAxes& ax, uint32_t* rec, hipStream_t s);

}  // namespace icp
