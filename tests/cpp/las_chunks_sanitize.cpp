// CPU self-test of the chunked LAS record reader (iterativeclosestpoint_amd/csrc/las_chunks.cpp:
// the file side of the device decode, host code without a HIP call), built with AddressSanitizer +
// UndefinedBehaviorSanitizer (csrc/Makefile target las_asan) and run by tests/test_las_chunks.py.
// Every chunk buffer is a heap block of exactly the capacity handed to the reader, so a byte
// written past it is a finding. For each file, both header rules, several point limits and
// several chunk capacities: a well-formed span comes back complete, in order and equal to the
// file's bytes; any other span ends with a short count or an error, never an overrun.
// One line per file: "<path> rc=<open status> n=<records> well_formed=<0|1>" (CLI rules, no
// limit), then "ok". Exit status 0 when every check passed; the sanitizers abort on findings.
//
// usage: las_chunks_sanitize [las files...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <vector>

#include "../../iterativeclosestpoint_amd/csrc/las_chunks.h"

static int g_fail = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                             \
    }                                                                       \
  } while (0)

static void one_span(const char* path, const std::vector<char>& file, int rules, int64_t max_points, size_t cap) {
  icp::LasSpan sp;
  if (icp::las_span_open(path, rules, max_points, &sp) != 0) {
    CHECK(sp.f == nullptr);
    return;
  }
  const int64_t rl = sp.hdr.record_length;
  CHECK(sp.file_bytes == (int64_t)file.size());
  CHECK(sp.n <= (int64_t)sp.hdr.num_points);
  if (rules == ICP_LAS_CORE && max_points > 0) CHECK(sp.n <= max_points);
  const int64_t end = (int64_t)sp.hdr.offset_to_points + sp.n * rl;
  CHECK(sp.well_formed == (rl >= 12 && end <= (int64_t)file.size()));
  std::unique_ptr<char[]> buf(new char[cap ? cap : 1]);  // exactly cap bytes: ASan guards the rest
  int64_t total = 0, expect_first = 0;
  for (int guard = 0; guard < 1 << 22; guard++) {
    int64_t first = -1;
    const int64_t cnt = icp::las_span_read(&sp, buf.get(), cap, &first);
    CHECK(first == expect_first);
    if (cnt <= 0) {
      if (cnt == -2) CHECK(rl <= 0 || (int64_t)cap < rl);
      if (cnt == 0) CHECK(total == sp.n);
      if (sp.well_formed && rl > 0 && (int64_t)cap >= rl) CHECK(cnt == 0);  // a whole span never fails
      break;
    }
    CHECK(cnt * rl <= (int64_t)cap && total + cnt <= sp.n);
    const int64_t at = (int64_t)sp.hdr.offset_to_points + total * rl;
    CHECK(at + cnt * rl <= (int64_t)file.size());
    if (at + cnt * rl <= (int64_t)file.size()) CHECK(std::memcmp(buf.get(), file.data() + at, (size_t)(cnt * rl)) == 0);
    total += cnt;
    expect_first = total;
  }
  icp::las_span_close(&sp);
  CHECK(sp.f == nullptr);
}

static void selections() {
  for (int64_t stride : {1, 2, 3, 7, 50, 1000})
    for (int64_t first : {0, 1, 6, 7, 49, 50, 51, 999, 1000, 123457})
      for (int64_t count : {1, 2, 7, 64, 3277}) {
        int64_t j0 = -1, out0 = -1;
        const int64_t sel = icp::las_chunk_selection(first, count, stride, &j0, &out0);
        int64_t want = 0, want_j0 = -1;
        for (int64_t g = first; g < first + count; g++)
          if (g % stride == 0) {
            if (want == 0) want_j0 = g - first;
            want++;
          }
        CHECK(sel == want);
        if (want > 0) {
          CHECK(j0 == want_j0 && out0 == (first + j0) / stride);
          CHECK(j0 + (sel - 1) * stride < count);  // the last kept record lies inside the chunk
        }
      }
}

int main(int argc, char** argv) {
  selections();
  for (int k = 1; k < argc; k++) {
    std::ifstream in(argv[k], std::ios::binary);
    std::vector<char> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    for (int rules : {ICP_LAS_CORE, ICP_LAS_CLI})
      for (int64_t max_points : {(int64_t)0, (int64_t)1, (int64_t)77, (int64_t)1 << 40})
        for (size_t cap : {(size_t)0, (size_t)11, (size_t)12, (size_t)20, (size_t)61, (size_t)4096, (size_t)65536})
          one_span(argv[k], file, rules, max_points, cap);
    icp::LasSpan sp;
    const int rc = icp::las_span_open(argv[k], ICP_LAS_CLI, 0, &sp);
    std::printf("%s rc=%d n=%lld well_formed=%d\n", argv[k], rc, (long long)(rc == 0 ? sp.n : 0),
                rc == 0 && sp.well_formed ? 1 : 0);
    if (rc == 0) icp::las_span_close(&sp);
  }
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
