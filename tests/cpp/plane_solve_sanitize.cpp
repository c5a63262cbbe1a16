// plane_solve_sanitize.cpp — the point-to-plane solve (iterativeclosestpoint_amd/csrc/plane_solve.h,
// host only) under AddressSanitizer + UndefinedBehaviorSanitizer (`make plane_asan`, run by
// tests/test_plane_host.py). argv[1]: a file of cases the host tests wrote, each an icp_plane_sums
// followed by an int64 (the expected ok flag). Every case is solved; a case that solves must give an
// orthonormal rotation and a T whose last row is (0, 0, 0, 1); a case that refuses must leave T
// untouched. Prints one line per case and "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../iterativeclosestpoint_amd/csrc/plane_solve.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<unsigned char> bytes;
  unsigned char buf[4096];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) bytes.insert(bytes.end(), buf, buf + got);
  std::fclose(f);
  const size_t rec = sizeof(icp_plane_sums) + sizeof(int64_t);
  if (bytes.empty() || bytes.size() % rec != 0) {
    std::fprintf(stderr, "%s: %zu bytes is not a whole number of %zu-byte cases\n", argv[1], bytes.size(), rec);
    return 2;
  }
  int bad = 0;
  for (size_t k = 0; k < bytes.size() / rec; k++) {
    icp_plane_sums s;
    int64_t want = 0;
    std::memcpy(&s, bytes.data() + k * rec, sizeof(s));
    std::memcpy(&want, bytes.data() + k * rec + sizeof(s), sizeof(want));
    double T[16];
    for (int i = 0; i < 16; i++) T[i] = -7.0 - i;  // a pattern a refusing solve must leave alone
    int32_t ok = -1;
    icp::plane_solve(&s, T, &ok);
    bool fine = ok == (int32_t)want;
    if (ok == 1) {
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
          double dot = 0.0;
          for (int i = 0; i < 3; i++) dot += T[4 * r + i] * T[4 * c + i];
          if (!(std::fabs(dot - (r == c ? 1.0 : 0.0)) <= 1e-14)) fine = false;
        }
      if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) fine = false;
      for (int i = 0; i < 12; i++)
        if (!std::isfinite(T[i])) fine = false;
    } else {
      for (int i = 0; i < 16; i++)
        if (T[i] != -7.0 - i) fine = false;
    }
    std::printf("case %zu ok=%d want=%d %s\n", k, (int)ok, (int)want, fine ? "fine" : "BAD");
    if (!fine) bad++;
  }
  // null arguments are ignored, not dereferenced
  icp_plane_sums z;
  std::memset(&z, 0, sizeof(z));
  int32_t ok = 5;
  icp::plane_solve(&z, nullptr, &ok);
  if (ok != 0) bad++;
  icp::plane_solve(nullptr, nullptr, nullptr);
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}
