// las_format.h — the 227-byte LAS 1.2 headers of the two reference writers (lasio.cpp), shared by
// the host writers and the device encode (ctx_las.cpp). Private to libicp_hip.so.
#pragma once

#include <cstdint>

namespace icp {

// LASIO::writeLAS: scale 0.001, offset = mn, 20-byte records (format 0).
void las_header_core(char h[227], uint32_t n, const double mn[3], const double mx[3]);
// saveResultAsLAS: the caller's scale and offset, the points' min and max.
void las_header_cli(char h[227], uint32_t n, const double scale[3], const double offset[3], const double mn[3],
                    const double mx[3]);

}  // namespace icp
