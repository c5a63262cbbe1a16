// voxel_host_sanitize.cpp — voxel-grid down-sampling on the host
// (iterativeclosestpoint_amd/csrc/voxel_host.h, header only) under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make voxel_asan`, run by tests/test_voxel_host.py). The run-length
// cases (one voxel of 1, 63, 64, 65, 128, 129 and 4097 points; a run of 17 beside a run of 16), the
// rejected inputs and the capacity cases, each with its outputs sized exactly (a write past m
// entries is the sanitizer's to find) and checked for what needs no second implementation: counts,
// first indices, the centroid inside its cell, FIRST mode's bits. Prints one line per case and "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../iterativeclosestpoint_amd/csrc/voxel_host.h"

namespace {

int g_bad = 0;

void report(const char* name, bool fine) {
  std::printf("%s %s\n", name, fine ? "fine" : "BAD");
  if (!fine) g_bad++;
}

// a deterministic value in [0, 1)
double unit(uint64_t k) {
  k = (k ^ (k >> 30)) * 0xbf58476d1ce4e5b9ull;
  k = (k ^ (k >> 27)) * 0x94d049bb133111ebull;
  return (double)((k ^ (k >> 31)) >> 11) * (1.0 / 9007199254740992.0);
}

struct Out {
  std::vector<double> xyz;
  std::vector<int32_t> first, count;
  int64_t m = 0;
  double origin[3] = {0, 0, 0};
  int rc = 0;
  std::string why;
};

// sized by a count-only call first, then the exact capacity
Out run(const std::vector<double>& p, double h, const double* origin, int mode) {
  Out o;
  const int64_t n = (int64_t)p.size() / 3;
  o.rc = icp::voxel_downsample_host(p.data(), n, h, origin, mode, 0, nullptr, nullptr, nullptr, &o.m, o.origin, &o.why);
  if (o.rc != ICP_HIP_OK) return o;
  o.xyz.resize(3 * (size_t)o.m);
  o.first.resize((size_t)o.m);
  o.count.resize((size_t)o.m);
  int64_t m2 = 0;
  o.rc = icp::voxel_downsample_host(p.data(), n, h, origin, mode, o.m, o.xyz.data(), o.first.data(), o.count.data(), &m2,
                                    o.origin, &o.why);
  if (m2 != o.m) o.rc = -100;
  return o;
}

// n points inside the cell [base, base + 1) of a grid of edge 1 from the origin (0, 0, 0)
void fill_cell(std::vector<double>* p, int n, double base, uint64_t seed) {
  for (int i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) p->push_back((a == 0 ? base : 0.0) + 0.01 + 0.98 * unit(seed + 3 * (uint64_t)i + a));
}

bool check_runs(const Out& o, const std::vector<double>& p, const std::vector<int>& lens, int mode) {
  if (o.rc != ICP_HIP_OK || o.m != (int64_t)lens.size()) return false;
  int32_t at = 0;
  for (size_t r = 0; r < lens.size(); r++) {
    if (o.count[r] != lens[r] || o.first[r] != at) return false;
    for (int a = 0; a < 3; a++) {
      const double v = o.xyz[3 * r + a];
      if (mode == ICP_VOXEL_FIRST) {
        if (std::memcmp(&v, &p[3 * (size_t)at + a], sizeof(double)) != 0) return false;
      } else {
        const double lo = a == 0 ? (double)r : 0.0;
        if (!(v > lo && v < lo + 1.0)) return false;
      }
    }
    at += lens[r];
  }
  return true;
}

}  // namespace

int main() {
  const double zero[3] = {0.0, 0.0, 0.0};
  for (int n : {1, 63, 64, 65, 128, 129, 4097})
    for (int mode : {ICP_VOXEL_CENTROID, ICP_VOXEL_FIRST}) {
      std::vector<double> p;
      fill_cell(&p, n, 0.0, (uint64_t)n);
      const Out o = run(p, 1.0, zero, mode);
      report(("run " + std::to_string(n) + (mode ? " first" : " centroid")).c_str(), check_runs(o, p, {n}, mode));
    }
  {
    std::vector<double> p;
    fill_cell(&p, 17, 0.0, 1000);
    fill_cell(&p, 16, 1.0, 2000);
    report("runs 17 + 16", check_runs(run(p, 1.0, zero, ICP_VOXEL_CENTROID), p, {17, 16}, ICP_VOXEL_CENTROID));
    // the cloud's own minimum as the origin: reported, and no point below it
    const Out o = run(p, 4.0, nullptr, ICP_VOXEL_CENTROID);
    bool fine = o.rc == ICP_HIP_OK && o.m == 1 && o.count[0] == 33;
    for (int a = 0; a < 3; a++) {
      double lo = p[a];
      for (size_t i = 0; i < p.size() / 3; i++) lo = p[3 * i + a] < lo ? p[3 * i + a] : lo;
      fine = fine && o.origin[a] == lo;
    }
    report("origin at the minimum", fine);
  }

  // rejected inputs: EINVAL, a reason, nothing written
  std::vector<double> p;
  fill_cell(&p, 40, 0.0, 7);
  const int64_t n = 40;
  double px[3] = {-7.0, -7.0, -7.0};
  int32_t pf = -7, pc = -7;
  int64_t m = -1;
  std::string why;
  auto refused = [&](int rc) { return rc == ICP_HIP_EINVAL && !why.empty() && px[0] == -7.0 && pf == -7 && pc == -7; };
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (double h : {0.0, -1.0, nan, inf}) {
    why.clear();
    report("bad edge", refused(icp::voxel_downsample_host(p.data(), n, h, zero, 0, 1, px, &pf, &pc, &m, nullptr, &why)));
  }
  why.clear();
  report("n = 0", refused(icp::voxel_downsample_host(p.data(), 0, 1.0, zero, 0, 1, px, &pf, &pc, &m, nullptr, &why)));
  why.clear();
  report("bad mode", refused(icp::voxel_downsample_host(p.data(), n, 1.0, zero, 2, 1, px, &pf, &pc, &m, nullptr, &why)));
  {
    std::vector<double> q = p;
    q[10] = nan;
    q[20] = inf;
    why.clear();
    const bool fine = refused(icp::voxel_downsample_host(q.data(), n, 1.0, nullptr, 0, 1, px, &pf, &pc, &m, nullptr, &why));
    report("non-finite coordinates", fine && why.find("2 non-finite") != std::string::npos);
  }
  {
    const double above[3] = {0.5, 0.0, 0.0};
    why.clear();
    const bool fine = refused(icp::voxel_downsample_host(p.data(), n, 1.0, above, 0, 1, px, &pf, &pc, &m, nullptr, &why));
    report("below the origin", fine && why.find("below") != std::string::npos);
  }
  {
    const double h = 0.5;
    std::vector<double> q = {0.0, 0.0, 0.0, 2097152.0 * h, 0.0, 0.0};
    why.clear();
    const bool fine = refused(icp::voxel_downsample_host(q.data(), 2, h, nullptr, 0, 1, px, &pf, &pc, &m, nullptr, &why));
    report("extent 2^21 h", fine && why.find("too fine") != std::string::npos);
    q[3] = 2097151.0 * h;
    const Out o = run(q, h, nullptr, ICP_VOXEL_FIRST);
    report("extent (2^21 - 1) h", o.rc == ICP_HIP_OK && o.m == 2 && o.first[1] == 1);
  }
  {
    std::vector<double> q;
    fill_cell(&q, 5, 0.0, 1);
    fill_cell(&q, 5, 1.0, 2);
    fill_cell(&q, 5, 2.0, 3);
    why.clear();
    std::vector<double> two(6, -7.0);
    const int rc = icp::voxel_downsample_host(q.data(), 15, 1.0, zero, 0, 2, two.data(), nullptr, nullptr, &m, nullptr, &why);
    bool fine = rc == ICP_HIP_EINVAL && m == 3 && !why.empty();
    for (double v : two) fine = fine && v == -7.0;
    report("cap = m - 1", fine);
    m = -1;
    const int rc2 = icp::voxel_downsample_host(q.data(), 15, 1.0, zero, 0, 0, nullptr, nullptr, nullptr, &m, nullptr, &why);
    report("count only", rc2 == ICP_HIP_OK && m == 3);
    std::vector<int32_t> cnt(3, -7);
    const int rc3 = icp::voxel_downsample_host(q.data(), 15, 1.0, zero, 0, 3, nullptr, nullptr, cnt.data(), &m, nullptr, &why);
    report("one output", rc3 == ICP_HIP_OK && m == 3 && cnt[0] == 5 && cnt[1] == 5 && cnt[2] == 5);
  }
  if (g_bad) return 1;
  std::printf("ok\n");
  return 0;
}
