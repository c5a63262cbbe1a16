// call_io_sanitize.cpp — a call's input upload and optional outputs (csrc/call_io.h) under ASan +
// UBSan, without a device: this program defines hipMalloc / hipFree / hipMemcpyAsync itself (malloc
// behind a table of live buffers and their sizes, a switch that fails the k-th allocation, an abort
// on a free of a pointer that is not live, and a copy that aborts unless each side lies inside a live
// "device" buffer or a registered host buffer, as its kind says) and runs the output type through
// both forms, a null pointer, and a call-shaped scope with every allocation failed in turn.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../iterativeclosestpoint_amd/csrc/call_io.h"

namespace {

std::map<const char*, size_t> live;  // "device" buffers: start -> bytes
std::map<const char*, size_t> host;  // the host buffers a copy may touch
int n_alloc = 0, n_free = 0, n_copy = 0;
size_t last_alloc_bytes = 0, last_copy_bytes = 0;
int fail_at = -1;  // the allocation (counted from 0) that fails; -1: none

void check(bool ok, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "FAILED (fail_at = %d): %s\n", fail_at, what);
  std::exit(1);
}

bool inside(const std::map<const char*, size_t>& m, const void* p, size_t bytes) {
  const char* c = static_cast<const char*>(p);
  for (const auto& b : m)
    if (c >= b.first && c + bytes <= b.first + b.second) return true;
  return false;
}

template <class T>
T* host_buffer(T* p, size_t count) {
  host[reinterpret_cast<const char*>(p)] = count * sizeof(T);
  return p;
}

}  // namespace

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
  if (n_alloc++ == fail_at) return hipErrorOutOfMemory;
  if (bytes == 0) std::abort();  // the owner never asks for an empty buffer
  *p = std::malloc(bytes);
  if (!*p) std::abort();
  live[static_cast<const char*>(*p)] = bytes;
  last_alloc_bytes = bytes;
  return hipSuccess;
}

extern "C" hipError_t hipFree(void* p) {
  if (!live.erase(static_cast<const char*>(p))) {
    std::fprintf(stderr, "hipFree of a pointer that is not live\n");
    std::abort();
  }
  n_free++;
  std::free(p);
  return hipSuccess;
}

extern "C" hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  const bool dst_dev = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice;
  const bool src_dev = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
  if (!inside(dst_dev ? live : host, dst, bytes) || !inside(src_dev ? live : host, src, bytes)) {
    std::fprintf(stderr, "copy of %zu bytes (kind %d) outside a live or host buffer\n", bytes, (int)kind);
    std::abort();
  }
  std::memcpy(dst, src, bytes);
  n_copy++;
  last_copy_bytes = bytes;
  return hipSuccess;
}

extern "C" const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "ok" : "error"; }

namespace {

// The device form: the caller's buffer is what the kernel writes; nothing is allocated or copied.
void device_form() {
  DevScratch S;
  double* d = nullptr;
  check(S.alloc(&d, 8) == hipSuccess, "the caller's device buffer");
  const int allocs = n_alloc, copies = n_copy;
  CallOut<double> o(d, false);
  check(o.prepare(S, 8) == hipSuccess && n_alloc == allocs, "device form: prepare allocates nothing");
  check(o.dev() == d && o.dev(3) == d + 3, "device form: dev() is the caller's pointer, a slice's at its offset");
  check(o.download(8, nullptr) == hipSuccess && n_copy == copies, "device form: download copies nothing");
  double* own = nullptr;  // an output the call holds itself: device to device
  check(S.alloc(&own, 8) == hipSuccess, "the call's own buffer");
  for (int i = 0; i < 8; i++) own[i] = 10.0 + i;
  check(o.copy_from(own, 8, nullptr) == hipSuccess && n_copy == copies + 1 && last_copy_bytes == 8 * sizeof(double),
        "device form: copy_from copies count elements");
  check(d[7] == 17.0, "device form: copy_from lands in the caller's buffer");
}

// A null pointer in either form: nothing allocated, dev() null, nothing copied.
void null_output(bool to_host) {
  DevScratch S;
  const int allocs = n_alloc, copies = n_copy;
  CallOut<int32_t> o(nullptr, to_host);
  check(o.prepare(S, 8) == hipSuccess && n_alloc == allocs, "null output: prepare allocates nothing");
  check(o.dev() == nullptr && o.dev(5) == nullptr, "null output: dev() is null at every offset");
  int32_t own[8] = {0};
  check(o.download(8, nullptr) == hipSuccess && o.download(8, nullptr, 4) == hipSuccess &&
            o.copy_from(own, 8, nullptr) == hipSuccess && n_copy == copies,
        "null output: nothing is copied");
}

// The host form: one allocation of max(count, 1) elements; download copies exactly count elements.
void host_form(size_t count) {
  DevScratch S;
  int32_t out[16 + 2];
  for (int32_t& v : out) v = -7;
  host_buffer(out + 1, count);  // a copy of one element more, or one earlier, aborts
  const int allocs = n_alloc, copies = n_copy;
  CallOut<int32_t> o(out + 1, true);
  check(o.dev() == nullptr, "host form: no buffer before prepare");
  check(o.prepare(S, count) == hipSuccess && n_alloc == allocs + 1, "host form: prepare allocates once");
  check(last_alloc_bytes == (count ? count : 1) * sizeof(int32_t), "host form: max(count, 1) elements");
  int32_t* d = o.dev();
  check(d != nullptr && d != out + 1 && o.dev(5) == d, "host form: dev() is the scratch buffer, whatever the slice");
  for (size_t i = 0; i < count; i++) d[i] = (int32_t)(100 + i);
  check(o.download(count, nullptr) == hipSuccess && n_copy == copies + 1, "host form: download copies once");
  check(last_copy_bytes == count * sizeof(int32_t), "host form: download copies exactly count elements");
  check(out[0] == -7 && out[count + 1] == -7, "host form: nothing is written outside the caller's count elements");
  for (size_t i = 0; i < count; i++) check(out[1 + i] == (int32_t)(100 + i), "host form: the elements arrive");
  if (count >= 4) {  // a slice: the buffer's first elements to the caller's, from the offset on
    d[0] = 900;
    d[1] = 901;
    check(o.download(2, nullptr, count - 2) == hipSuccess && last_copy_bytes == 2 * sizeof(int32_t), "host form: a slice");
    check(out[1 + count - 2] == 900 && out[1 + count - 1] == 901 && out[count + 1] == -7, "host form: a slice lands at its offset");
  }
  int32_t* own = nullptr;  // an output the call holds itself: device to host
  check(S.alloc(&own, count) == hipSuccess, "the call's own buffer");
  for (size_t i = 0; i < count; i++) own[i] = (int32_t)(200 + i);
  check(o.copy_from(own, count, nullptr) == hipSuccess && last_copy_bytes == count * sizeof(int32_t), "host form: copy_from");
  for (size_t i = 0; i < count; i++) check(out[1 + i] == (int32_t)(200 + i), "host form: copy_from's elements arrive");
  host.clear();
}

// A call's shape in the host form: the input uploaded, three outputs (one not asked for), all
// downloaded. Returns whether it ran whole; *made = the allocations that succeeded.
bool scope(int* made) {
  double in[30], xyz_out[30];
  int32_t idx_out[10];
  for (int i = 0; i < 30; i++) in[i] = 0.5 * i;
  host_buffer(in, 30);
  host_buffer(xyz_out, 30);
  host_buffer(idx_out, 10);
  *made = 0;
  DevScratch S;
  CallOut<double> xyz(xyz_out, true), none(nullptr, true);
  CallOut<int32_t> idx(idx_out, true);
  double* up = nullptr;
  if (call_upload(S, &up, in, 30, nullptr) != hipSuccess) {
    check(up == nullptr, "a failed upload leaves no pointer");
    return false;
  }
  (*made)++;
  check(up[29] == 14.5, "the upload's elements arrive");
  if (xyz.prepare(S, 30) != hipSuccess) {
    check(xyz.dev() == nullptr, "a failed prepare leaves no buffer");
    return false;
  }
  (*made)++;
  check(none.prepare(S, 30) == hipSuccess && none.dev() == nullptr, "an output not asked for costs no allocation");
  if (idx.prepare(S, 10) != hipSuccess) {
    check(idx.dev() == nullptr, "a failed prepare leaves no buffer");
    return false;
  }
  (*made)++;
  for (int i = 0; i < 30; i++) xyz.dev()[i] = up[i] + 1.0;
  for (int i = 0; i < 10; i++) idx.dev()[i] = i;
  check(xyz.download(30, nullptr) == hipSuccess && none.download(30, nullptr) == hipSuccess &&
            idx.download(10, nullptr) == hipSuccess,
        "the downloads");
  check(xyz_out[29] == 15.5 && idx_out[9] == 9, "the outputs arrive");
  return true;
}

}  // namespace

int main() {
  device_form();
  null_output(false);
  null_output(true);
  for (size_t count : {(size_t)0, (size_t)1, (size_t)16}) host_form(count);
  check(live.empty(), "the forms' scopes freed their buffers");
  std::printf("forms fine\n");
  const int kAllocs = 3;
  for (int k = -1; k <= kAllocs; k++) {
    fail_at = k;
    n_alloc = n_free = 0;
    int made = 0;
    const bool whole = scope(&made);
    host.clear();
    check(whole == (k < 0 || k >= kAllocs), "the scope runs whole only without a failed allocation");
    check(made == (whole ? kAllocs : k), "the scope stops at the failed allocation");
    check(n_free == made, "every buffer is freed exactly once at the scope's end");
    check(live.empty(), "nothing is left live");
    std::printf("fail_at %2d: %d allocations, %d frees, fine\n", k, made, n_free);
  }
  std::printf("ok\n");
  return 0;
}
