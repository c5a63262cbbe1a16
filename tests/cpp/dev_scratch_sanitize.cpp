// dev_scratch_sanitize.cpp — DevScratch's ownership under ASan + UBSan, without a device: this
// program defines hipMalloc / hipFree itself (malloc behind a set of live pointers, a switch that
// fails the k-th allocation, an abort on a free of a pointer that is not live) and runs scopes
// shaped like the library's calls for k = none, 0, 1, ..., one past the last allocation.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <set>

#include "../../iterativeclosestpoint_amd/csrc/dev_scratch.h"

namespace {

std::set<void*> live;
int n_alloc = 0, n_free = 0;
int fail_at = -1;  // the allocation (counted from 0) that fails; -1: none

void check(bool ok, const char* what, int k) {
  if (ok) return;
  std::fprintf(stderr, "FAILED (fail_at = %d): %s\n", k, what);
  std::exit(1);
}

}  // namespace

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
  if (n_alloc++ == fail_at) return hipErrorOutOfMemory;
  if (bytes == 0) std::abort();  // the owner never asks for an empty buffer
  *p = std::malloc(bytes);
  if (!*p) std::abort();
  live.insert(*p);
  return hipSuccess;
}

extern "C" hipError_t hipFree(void* p) {
  if (!live.erase(p)) {
    std::fprintf(stderr, "hipFree of a pointer that is not live\n");
    std::abort();
  }
  n_free++;
  std::free(p);
  return hipSuccess;
}

extern "C" const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "ok" : "error"; }

namespace {

// A call's shape: three buffers (one of a count of 0), one grown twice, one kept on success.
// Returns the kept buffer (null: the scope failed); *made = the allocations that succeeded.
double* scope(int* made, void** grown_first) {
  DevScratch S;
  static double stale[1];  // what a failed alloc must not leave in *p
  double *a = stale, *kept = stale;
  int* b = reinterpret_cast<int*>(stale);
  unsigned char* g = nullptr;
  *made = 0;
  *grown_first = nullptr;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t err, const void* p) {
    if (err != hipSuccess) {
      check(p == nullptr, "*p is null after a failed alloc", fail_at);
      return false;
    }
    check(p != nullptr, "a successful alloc yields a pointer", fail_at);
    (*made)++;
    return true;
  };
  e = S.alloc(&a, 100);
  if (!ok(e, a)) return nullptr;
  a[99] = 1.0;
  e = S.alloc(&b, 0);
  if (!ok(e, b)) return nullptr;  // a count of 0: one element
  b[0] = 7;
  e = S.regrow(&g, 16);
  if (!ok(e, g)) return nullptr;  // from null: a plain alloc
  *grown_first = g;
  g[15] = 1;
  e = S.regrow(&g, 64);
  if (!ok(e, g)) return nullptr;
  check(live.count(*grown_first) == 0, "the grown buffer's predecessor is freed at once", fail_at);
  g[63] = 1;
  e = S.alloc(&kept, 10);
  if (!ok(e, kept)) return nullptr;
  kept[9] = 2.0;
  return S.keep(kept);
}

}  // namespace

int main() {
  const int kAllocs = 5;
  for (int k = -1; k <= kAllocs; k++) {
    fail_at = k;
    n_alloc = n_free = 0;
    int made = 0;
    void* first = nullptr;
    double* kept = scope(&made, &first);
    const bool whole = k < 0 || k >= kAllocs;
    const int owner_frees = n_free;  // before this test releases the kept buffer itself
    check(made == (whole ? kAllocs : k), "the scope stops at the failed allocation", k);
    check((kept != nullptr) == whole, "the kept buffer is returned only by a whole scope", k);
    if (kept) {
      check(live.size() == 1 && live.count(kept) == 1, "only the kept buffer outlives the scope", k);
      check(kept[9] == 2.0, "the kept buffer is intact", k);
      check(owner_frees == made - 1, "every other buffer is freed exactly once", k);
      (void)hipFree(kept);
    } else {
      check(owner_frees == made, "every buffer of a failed scope is freed exactly once", k);
    }
    check(live.empty(), "nothing is left live", k);
    std::printf("fail_at %2d: %d allocations, %d frees, fine\n", k, made, owner_frees);
  }
  {  // keep of a pointer the owner does not hold changes nothing
    fail_at = -1;
    DevScratch S;
    int* a = nullptr;
    int other = 0;
    check(S.alloc(&a, 4) == hipSuccess, "alloc", -1);
    check(S.keep(&other) == &other, "keep returns its argument", -1);
    check(live.size() == 1, "the owner still holds its buffer", -1);
  }
  check(live.empty(), "the last scope freed its buffer", -1);
  std::printf("ok\n");
  return 0;
}
