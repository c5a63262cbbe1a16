// las_chunks.cpp — see las_chunks.h. Host code only: no HIP calls, buffers are plain pointers.
#include "las_chunks.h"

#include <sys/stat.h>

namespace icp {

int las_span_open(const char* path, int rules, int64_t max_points, LasSpan* s) {
  *s = LasSpan{};
  const int rc = icp_las_read_header(path, rules, &s->hdr);
  if (rc != 0) return rc;
  s->f = std::fopen(path, "rb");
  if (!s->f) return -1;
  struct stat st;
  if (fstat(fileno(s->f), &st) != 0) {
    las_span_close(s);
    return -1;
  }
  s->file_bytes = (int64_t)st.st_size;
  s->n = s->hdr.num_points;
  if (rules == ICP_LAS_CORE && max_points > 0 && max_points < s->n) s->n = max_points;  // lasio.cpp:60-63
  const int64_t rl = s->hdr.record_length;
  const int64_t end = (int64_t)s->hdr.offset_to_points + s->n * rl;  // < 2^32 + 2^32 * 2^16: no overflow
  s->well_formed = rl >= 12 && end <= s->file_bytes;
  if (std::fseek(s->f, (long)s->hdr.offset_to_points, SEEK_SET) != 0) {
    las_span_close(s);
    return -1;
  }
  return 0;
}

void las_span_close(LasSpan* s) {
  if (s->f) std::fclose(s->f);
  s->f = nullptr;
}

int64_t las_span_read(LasSpan* s, void* buf, size_t cap, int64_t* first_record) {
  if (first_record) *first_record = s->next;
  if (s->next >= s->n) return 0;
  const int64_t rl = s->hdr.record_length;
  if (rl <= 0 || (int64_t)cap < rl) return -2;
  int64_t cnt = (int64_t)cap / rl;
  if (cnt > s->n - s->next) cnt = s->n - s->next;
  const size_t bytes = (size_t)(cnt * rl);
  if (std::fread(buf, 1, bytes, s->f) != bytes) return -1;
  s->next += cnt;
  return cnt;
}

int64_t las_chunk_selection(int64_t first, int64_t count, int64_t stride, int64_t* j0, int64_t* out0) {
  if (stride < 1) stride = 1;
  const int64_t g0 = (first + stride - 1) / stride * stride;  // first kept record at or after `first`
  *j0 = g0 - first;
  *out0 = g0 / stride;
  if (g0 >= first + count) return 0;
  return (first + count - 1 - g0) / stride + 1;
}

}  // namespace icp
