// phase_events.h — start / end HIP events of the N phases of one call (the voxel and the outlier
// calls time their phases with it; read-backs between phases stay outside the intervals).
#pragma once

#include <hip/hip_runtime.h>

template <int N>
struct PhaseEvents {
  hipEvent_t ev[2 * N] = {};
  bool ran[N] = {};
  PhaseEvents() = default;
  PhaseEvents(const PhaseEvents&) = delete;
  PhaseEvents& operator=(const PhaseEvents&) = delete;
  ~PhaseEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  // k = 2 p: phase p starts; k = 2 p + 1: it ends
  hipError_t mark(int k, hipStream_t s) {
    if (!ev[k]) {
      const hipError_t e = hipEventCreate(&ev[k]);
      if (e != hipSuccess) return e;
    }
    if (k & 1) ran[k >> 1] = true;
    return hipEventRecord(ev[k], s);
  }
  // after the stream is synchronised; a phase that did not run: 0
  hipError_t read(double ms[N]) const {
    for (int p = 0; p < N; p++) {
      float f = 0.0f;
      if (ran[p]) {
        const hipError_t e = hipEventElapsedTime(&f, ev[2 * p], ev[2 * p + 1]);
        if (e != hipSuccess) return e;
      }
      ms[p] = f;
    }
    return hipSuccess;
  }
};
