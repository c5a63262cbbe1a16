// call_io.h — the input and the optional outputs of a call that exists in two forms (DESIGN.md
// §3.8): the host form takes host buffers and goes through buffers of the call's DevScratch, the
// device form reads and writes the caller's device buffers in place. Needs the HIP runtime and
// dev_scratch.h alone. The ordering rules are dev_scratch.h's: the copies enqueued here are
// followed by the caller's synchronise before a successful return.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "dev_scratch.h"

// The host form's input: count elements of `host` in a buffer of S, the copy enqueued on s.
template <class T>
hipError_t call_upload(DevScratch& S, T** d, const T* host, size_t count, hipStream_t s) {
  const hipError_t e = S.alloc(d, count);
  return e != hipSuccess ? e : hipMemcpyAsync(*d, host, count * sizeof(T), hipMemcpyHostToDevice, s);
}

// One optional output: the caller's pointer (null: not asked for) and the call's form.
template <class T>
class CallOut {
 public:
  CallOut(T* out, bool to_host) : out_(out), dev_(to_host ? nullptr : out), to_host_(to_host) {}

  // The host form of an output asked for: a buffer of S of count elements. Otherwise nothing.
  hipError_t prepare(DevScratch& S, size_t count) { return to_host_ && out_ ? S.alloc(&dev_, count) : hipSuccess; }

  // What the kernel writes; null when the output was not asked for. A call that runs in slices
  // passes the slice's first element: the device form writes there in the caller's buffer, the
  // host form's buffer holds one slice.
  T* dev(size_t off = 0) const { return to_host_ || !dev_ ? dev_ : dev_ + off; }

  // The host form: the buffer's first count elements to the caller's, from element off on.
  hipError_t download(size_t count, hipStream_t s, size_t off = 0) const {
    if (!to_host_ || !out_) return hipSuccess;
    return hipMemcpyAsync(out_ + off, dev_, count * sizeof(T), hipMemcpyDeviceToHost, s);
  }

  // An output the call holds in a device buffer of its own (src): copied to the caller in either form.
  hipError_t copy_from(const T* src, size_t count, hipStream_t s) const {
    if (!out_) return hipSuccess;
    return hipMemcpyAsync(out_, src, count * sizeof(T), to_host_ ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s);
  }

 private:
  T* out_;
  T* dev_;
  bool to_host_;
};
