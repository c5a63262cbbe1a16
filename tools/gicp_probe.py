#!/usr/bin/env python3
"""Timings of the generalized-ICP calls on the LiDAR-like scene (icp.synth_scene, bench.py --scene),
one GPU process, one JSON line per size (DESIGN.md §3.13 quotes them; profiles/gicp/ keeps them).
Each call is written next to its yardstick on the same context and the same iterate:

  sums      icp_hip_gicp_sums_at against icp_hip_plane_sums_at, both at the iterate's own threshold
            about its centroid_src: the same reads (per pair the residual, the match, the moved source
            point, two 32-byte target lines) plus, for the generalized sums, the 24-byte stream of the
            source's normals.
  normals   icp_hip_estimate_source_normals against icp_hip_estimate_target_normals of the same cloud
            (the source, set as the target of the same context), the same k: the same kernel plus the
            un-permute, the private octree build and two gathers.

One warm call of each, then --reps calls of each, interleaved; the host clock around the call (every
one ends in a stream synchronise). Reported: the medians, every repetition, and the ratio of the
medians.

  gicp_probe.py [--points 100000,1000000,10000000] [--reps 9] [--k 16] [--out FILE]

Every step raises on a failing call; the process then exits non-zero and nothing further runs.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def wall_ms(fn, *a, **kw):
    t0 = time.perf_counter()
    out = fn(*a, **kw)
    return (time.perf_counter() - t0) * 1e3, out


def interleaved(reps, *calls):
    """One warm call of each, then reps rounds of all of them in turn: a list of times per call."""
    for c in calls:
        c()
    times = [[] for _ in calls]
    for _ in range(reps):
        for t, c in zip(times, calls):
            t.append(wall_ms(c)[0])
    return times


def probe_size(icp, n, reps, k, emit):
    tgt, src, _ = icp.synth_scene(n)
    eye = np.eye(3)
    with icp.Context(0) as ctx:
        # the normals' yardstick first: the source as the context's target
        ctx.set_target(src)
        ctx.set_source(src)
        t_src, t_tgt = interleaved(reps, lambda: ctx.estimate_source_normals(k), lambda: ctx.estimate_target_normals(k))
        same = ctx.get_source_normals().tobytes() == ctx.get_target_normals().tobytes()
        # the sums on one iterate of the scene pair
        ctx.set_target(tgt)
        ctx.estimate_target_normals(k)
        ctx.estimate_source_normals(k)
        st = ctx.iterate()
        o, thr = np.array(st.centroid_src[:]), st.threshold
        t_gicp, t_plane = interleaved(reps, lambda: ctx.gicp_sums_at(o, eye, 1e-3, thr), lambda: ctx.plane_sums_at(o, thr))
        s = ctx.gicp_sums_at(o, eye, 1e-3, thr)
    r3 = lambda v: [round(x, 3) for x in v]
    med = statistics.median
    emit({"figure": "gicp", "points": n, "k": k, "reps": reps, "valid_pairs": s.n,
          "gicp_sums_at_ms_median": round(med(t_gicp), 3), "gicp_sums_at_ms_runs": r3(t_gicp),
          "plane_sums_at_ms_median": round(med(t_plane), 3), "plane_sums_at_ms_runs": r3(t_plane),
          "gicp_over_plane": round(med(t_gicp) / med(t_plane), 3),
          "estimate_source_normals_ms_median": round(med(t_src), 3), "estimate_source_normals_ms_runs": r3(t_src),
          "estimate_target_normals_ms_median": round(med(t_tgt), 3), "estimate_target_normals_ms_runs": r3(t_tgt),
          "source_over_target_normals": round(med(t_src) / med(t_tgt), 3), "normals_bytes_equal": same,
          "clock": "host around each call (each ends in a stream synchronise), calls interleaved"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="100000,1000000,10000000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import iterativeclosestpoint_amd as icp

    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        if a.out:  # kept up to date: a later step that fails loses nothing measured before it
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))

    for n in [int(x) for x in a.points.split(",") if x]:
        probe_size(icp, n, a.reps, a.k, emit)


if __name__ == "__main__":
    main()
