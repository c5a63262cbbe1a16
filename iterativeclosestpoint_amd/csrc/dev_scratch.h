// dev_scratch.h — the one owner of device memory that lives for a single call (needs the HIP
// runtime alone, so the .hip units use it without the context's headers).
//
// Ordering, as every user keeps it: a function that has enqueued work reading or writing one of
// these buffers synchronises its stream before it returns successfully. On a failure path the
// destructor's hipFree does the waiting (it returns only once the device is done with the
// memory). A host buffer of the caller is never the destination of a copy still in flight at
// return: such a copy is followed by a synchronise on the success path, and a failed call's output
// is unspecified but its copies have ended with the hipFree.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

class DevScratch {
 public:
  DevScratch() = default;
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() {
    for (void* p : ptrs_) (void)hipFree(p);
  }

  // count elements (one for a count of 0: never a null buffer); *p is null on failure.
  template <class T>
  hipError_t alloc(T** p, size_t count) {
    *p = nullptr;
    void* v = nullptr;
    const hipError_t e = hipMalloc(&v, (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) return e;
    ptrs_.push_back(v);
    *p = static_cast<T*>(v);
    return hipSuccess;
  }

  // *p (one of this owner's buffers, or null) replaced by a buffer of count elements; the old
  // one is freed first and its contents are not carried over.
  template <class T>
  hipError_t regrow(T** p, size_t count) {
    if (*p && drop(*p)) (void)hipFree(*p);
    return alloc(p, count);
  }

  // p leaves the owner (a buffer that outlives the call) and is returned.
  template <class T>
  T* keep(T* p) {
    drop(p);
    return p;
  }

 private:
  bool drop(const void* p) {
    for (size_t k = 0; k < ptrs_.size(); k++)
      if (ptrs_[k] == p) {
        ptrs_.erase(ptrs_.begin() + (std::ptrdiff_t)k);
        return true;
      }
    return false;
  }
  std::vector<void*> ptrs_;
};
