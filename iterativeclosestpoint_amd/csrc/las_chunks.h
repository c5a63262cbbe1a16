// las_chunks.h — the chunked reader of a LAS file's point records (host only, no HIP calls): the
// device decode's file side (ctx_las.cpp), which hands it its pinned staging buffers as plain
// pointers. Private to libicp_hip.so; tests/cpp/las_chunks_sanitize.cpp links it under ASan/UBSan.
#pragma once

#include <cstdint>
#include <cstdio>

#include "../../include/icp_las.h"

namespace icp {

// The span of point records of an open file: n records of hdr.record_length bytes from
// hdr.offset_to_points. well_formed: the file holds all of the span and a record holds its three
// coordinates (record_length >= 12); only then do the raw bytes alone give the host reader's
// points (a short file makes icp_las_read parse stale batch-buffer bytes, lasio.cpp).
struct LasSpan {
  std::FILE* f = nullptr;
  icp_las_header hdr{};
  int64_t n = 0;         // records of the span: min(num_points, max_points) (core), num_points (CLI)
  int64_t next = 0;      // first record of the next chunk
  int64_t file_bytes = 0;
  bool well_formed = false;
};

// Opens the file and reads its header by the rules of icp_las_read_header. Returns 0, or that
// call's error (-1 cannot open / read, -2 bad signature or point count). max_points <= 0: no limit.
int las_span_open(const char* path, int rules, int64_t max_points, LasSpan* s);
void las_span_close(LasSpan* s);

// Reads the next chunk of whole records into buf (cap bytes, at least one record). Returns the
// records read (their bytes start at buf[0]), 0 after the last record, -1 when the file ends or
// fails inside the span (never the case for a well-formed span that nobody truncates meanwhile),
// -2 when cap holds no record. *first_record gets the span index of the chunk's first record.
int64_t las_span_read(LasSpan* s, void* buf, size_t cap, int64_t* first_record);

// The records of a chunk that a stride keeps (span indices 0, stride, 2 stride, ...): the chunk
// holds records [first, first + count). Returns how many; *j0 gets the chunk index of the first
// kept record and *out0 its index among the kept records of the whole span.
int64_t las_chunk_selection(int64_t first, int64_t count, int64_t stride, int64_t* j0, int64_t* out0);

}  // namespace icp
