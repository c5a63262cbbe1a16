/*
 * icp_las.h — LAS 1.2 point I/O of the two reference front-ends. The host calls (no GPU):
 *   icp_las_read        LASIO::readLAS (core/lasio.cpp:7-125; signature check, maxPoints
 *                       truncation) and readLASFile (icp_registration.cpp:248-378; rejects 0 or
 *                       > 1e8 points) — x = X * scale + offset per axis
 *   icp_las_write_core  LASIO::writeLAS (core/lasio.cpp:127-210): scale 0.001, offset = min
 *   icp_las_write_cli   saveResultAsLAS (icp_registration.cpp:698-815): caller's scale/offset
 *   icp_write_transform_report  saveTransformation (icp_registration.cpp:625-695), same text
 * Integer conversion truncates toward zero, as the reference's casts do.
 * The icp_hip_*_las calls at the end do the same between files and clouds resident on a context's
 * device: records decoded and encoded by kernels, the same points and the same file bytes.
 */
#ifndef ICP_LAS_H
#define ICP_LAS_H

#include <stddef.h>
#include <stdint.h>

#include "icp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ICP_LAS_CORE 0 /* LASIO::readLAS rules   */
#define ICP_LAS_CLI 1  /* readLASFile rules      */

typedef struct icp_las_header {
  uint32_t offset_to_points;
  uint32_t num_points;
  uint16_t record_length;
  double scale[3];
  double offset[3];
  double max[3];
  double min[3];
} icp_las_header;

/* Header only. Returns 0 on success, -1 if the file cannot be opened/read, -2 bad signature
 * (core rules) or bad point count (CLI rules). */
int icp_las_read_header(const char* path, int rules, icp_las_header* hdr);

/* Points (AoS xyz). xyz_out must hold min(num_points, max_points) points (max_points 0 = all;
 * with CLI rules, whose reader has no limit, max_points only bounds the output buffer).
 * Returns the number of points read (>= 0) or a negative error as above. */
int64_t icp_las_read(const char* path, int rules, int64_t max_points, double* xyz_out, icp_las_header* hdr);

/* LASIO::writeLAS with the bounds of the given points (PointCloud::computeBounds first). */
int icp_las_write_core(const char* path, const double* xyz, int64_t n);
/* LASIO::writeLAS with the caller's PointCloud bounds as they stand (minX, maxX, minY, maxY, minZ,
 * maxZ): the writer's offset is minX/minY/minZ whatever the points are now. The reference service
 * saves the registered source with the bounds computed when it was loaded
 * (registrationservice.cpp:98, :156), so its coordinates can fall below the offset. */
int icp_las_write_core_bounds(const char* path, const double* xyz, int64_t n, const double bounds[6]);
int icp_las_write_cli(const char* path, const double* xyz, int64_t n, const double scale[3], const double offset[3]);

/* R row-major 3x3, t[3]; transforms: n_transforms cumulative 4x4 (row-major) or null. */
int icp_write_transform_report(const char* path, const double R[9], const double t[3], const double* transforms,
                               int32_t n_transforms);

/* --- Files to and from clouds resident on the device (needs a GPU). The raw records cross PCIe
 * through two pinned staging buffers of the context (a chunk is read from the file while the
 * previous one is copied and decoded; written while the next one is encoded and copied) and are
 * decoded / encoded by kernels: 12 to record_length bytes per point up instead of 24, 20 down.
 * Points and file bytes are those of icp_las_read / icp_las_write_* exactly. Errors as in
 * icp_hip.h (ICP_HIP_EINVAL for a file that cannot be opened, read or written, or that
 * icp_las_read_header rejects); a multi-device context does the device work on its first member.
 *
 * Reading: las_rules as icp_las_read_header; the span is n = min(num_points, max_points) records
 * (core rules; max_points 0 = all) or num_points (CLI rules, max_points ignored); stride >= 1
 * keeps records 0, stride, 2 stride, ... of it (the CLI's `i += sample_rate` loop), so a call
 * yields (n - 1) / stride + 1 points. hdr (may be null) gets the file's header, *n_out the points.
 * Files the kernels would not reproduce go through icp_las_read and one upload instead: a file
 * shorter than its header claims (the host reader then parses what its batch buffer held) and
 * record_length < 12 (no room for three coordinates; 0 included).
 * Writing: flavour ICP_LAS_CLI = icp_las_write_cli (scale, offset required; bounds ignored),
 * ICP_LAS_CORE = icp_las_write_core_bounds with bounds (minX, maxX, minY, maxY, minZ, maxZ), or
 * icp_las_write_core when bounds is null (scale, offset ignored). A cloud with a non-finite
 * coordinate, or one whose (v - offset) / scale lies outside int32 (where the host's cast and the
 * device's conversion differ), is downloaded and written by the host writer. */

/* Decode into the caller's device buffer (contract of the *_device calls, icp_hip.h), which holds
 * the points the header promises: d_xyz_out = null only reports hdr and *n_out for sizing it. */
int icp_hip_read_las_device(icp_hip_ctx* ctx, const char* path, int las_rules, int64_t max_points, int64_t stride,
                            double* d_xyz_out, icp_las_header* hdr, int64_t* n_out);
/* icp_hip_set_target / icp_hip_set_source from a file: decoded into a scratch buffer in HBM that
 * the builders read in place. n_out may be null. */
int icp_hip_set_target_las(icp_hip_ctx* ctx, const char* path, int las_rules, int64_t max_points, int64_t stride,
                           int max_tree_points, int max_depth, int rules, icp_las_header* hdr, int64_t* n_out);
int icp_hip_set_source_las(icp_hip_ctx* ctx, const char* path, int las_rules, int64_t max_points, int64_t stride,
                           icp_las_header* hdr, int64_t* n_out);
/* Encode a device cloud (n >= 1 points), or the context's resident (moved) source. */
int icp_hip_write_las_device(icp_hip_ctx* ctx, const char* path, const double* d_xyz, int64_t n, int flavour,
                             const double scale[3], const double offset[3], const double bounds[6]);
int icp_hip_write_source_las(icp_hip_ctx* ctx, const char* path, int flavour, const double scale[3],
                             const double offset[3], const double bounds[6]);
/* Testing hook: whether the context's last LAS call that moved points went through the kernels (1)
 * or the host reader / writer (0). ICP_HIP_ENOTREADY before the first such call. */
int icp_hip_last_las_path(icp_hip_ctx* ctx, int32_t* device_path);
/* Tuning / testing: bytes of each of the two staging buffers, in [64 KiB, 256 MiB] (default
 * 8 MiB). The buffers are made at the first LAS call and remade after a change. */
int icp_hip_set_las_chunk_bytes(icp_hip_ctx* ctx, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
