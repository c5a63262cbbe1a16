// ctx_util.h — what every unit of the C-ABI context shares: the error string's setter, the
// HIP / RCCL call checks and the device allocation helpers (private to libicp_hip.so).
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <string>
#include <utility>

#include "../../include/icp_hip.h"
#include "dev_scratch.h"

// The calling thread's error text, read back by icp_hip_last_error (the string: icp_ctx.hip).
void icp_ctx_set_error(const char* msg);

static inline int fail(int code, const std::string& msg) {
  icp_ctx_set_error(msg.c_str());
  return code;
}

// The one mapping from a HIP error to the C ABI: out of memory is ENOMEM, anything else EDEVICE.
static inline int fail_hip(const char* what, hipError_t e) {
  return fail(e == hipErrorOutOfMemory ? ICP_HIP_ENOMEM : ICP_HIP_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail_hip(#expr, e_);                                          \
  } while (0)

#define RCCL_TRY(expr)                                                                         \
  do {                                                                                         \
    ncclResult_t r_ = (expr);                                                                  \
    if (r_ != ncclSuccess) return fail(ICP_HIP_ERCCL, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
  } while (0)

// Context-lifetime buffers (a call's own scratch: DevScratch).
template <typename T>
hipError_t dalloc(T** p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  return hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
}

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

// Runs `f` when the scope ends, unless dismissed: the undo of a call that installs state in steps.
template <class F>
class ScopeExit {
 public:
  explicit ScopeExit(F f) : f_(std::move(f)) {}
  ScopeExit(const ScopeExit&) = delete;
  ScopeExit& operator=(const ScopeExit&) = delete;
  ~ScopeExit() {
    if (armed_) f_();
  }
  void dismiss() { armed_ = false; }

 private:
  F f_;
  bool armed_ = true;
};
