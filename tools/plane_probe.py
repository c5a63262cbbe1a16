#!/usr/bin/env python3
"""Timings of the point-to-plane path on the LiDAR-like scene (icp.synth_scene), one GPU process,
one JSON line per figure (DESIGN.md §3.9 quotes them; profiles/plane/ keeps them):

  normals       icp_hip_estimate_target_normals at k neighbours: host clock around the call (it ends
                in a stream synchronise), the first call apart, then the median of --reps calls.
  plane_sums    icp_hip_plane_sums after each iterate of a plane session: host clock around the call
                (launch, merge, 256-B copy, synchronise), beside the iterate's own device time
                (icp_hip_last_timing, timing_stride 1) and the step's compulsory bytes per query:
                streamed source 24 B + pos 4 B + dist 8 B, gathered at 64-B line granularity a 32-B
                target record and a 24-B normal = 164 B.
  registration  both metrics with early stops on: iterations and host wall time until t_rmse against
                T_true first falls to each of --targets, and where the session stopped.

  plane_probe.py [--points 1000000,10000000] [--k 16] [--reps 3] [--iterates 10]
                 [--registration-points 1000000] [--targets 1e-2,3e-3,1e-3,3e-4] [--out FILE]

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

BYTES_PER_QUERY = 24 + 4 + 8 + 64 + 64


def t_rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


def wall_ms(fn, *a, **kw):
    t0 = time.perf_counter()
    out = fn(*a, **kw)
    return (time.perf_counter() - t0) * 1e3, out


def probe_size(icp, n, k, reps, iterates, emit):
    tgt, src, _ = icp.synth_scene(n)
    with icp.Context(0, cfg={"timing_stride": 1}) as ctx:
        ms, _ = wall_ms(ctx.set_target, tgt)
        emit({"figure": "set_target", "points": n, "ms": round(ms, 3), "info": ctx.target_info()})
        first, _ = wall_ms(ctx.estimate_target_normals, k)
        runs = [wall_ms(ctx.estimate_target_normals, k)[0] for _ in range(reps)]
        nrm = ctx.get_target_normals()
        emit({"figure": "normals", "points": n, "k": k, "first_call_ms": round(first, 3),
              "median_ms": round(statistics.median(runs), 3), "runs_ms": [round(r, 3) for r in runs],
              "zero_normals": int((~nrm.any(1)).sum()), "clock": "host, the call ends in a stream synchronise"})
        del nrm
        ctx.set_source(src)
        sums_ms, it_ms, nn_ms, used = [], [], [], []
        T = None
        for it in range(iterates):
            # a plane session's step, by hand, so that the sums are timed alone
            st = ctx.iterate(T, it, icp.RULES_ENGINE, 3.0)
            a, b = ctx.last_timing()
            ms, s = wall_ms(ctx.plane_sums, st.centroid_src)
            T, ok = icp.plane_solve(s)
            if not ok:
                T = icp.best_fit_from_stats(st)
            sums_ms.append(ms)
            nn_ms.append(a)
            it_ms.append(b)
            used.append(int(ok))
        med = statistics.median(sums_ms[1:])  # the first call makes the part buffer
        emit({"figure": "plane_sums", "points": n, "iterates": iterates, "first_call_ms": round(sums_ms[0], 4),
              "median_ms": round(med, 4), "runs_ms": [round(r, 4) for r in sums_ms],
              "iterate_device_ms_median": round(statistics.median(it_ms[1:]), 4),
              "search_kernel_ms_median": round(statistics.median(nn_ms[1:]), 4),
              "used_plane": used, "bytes_per_query": BYTES_PER_QUERY,
              "compulsory_GB_per_s_at_median": round(n * BYTES_PER_QUERY / (med * 1e-3) / 1e9, 1),
              "clock": "host around the call: two launches, a 256-B copy, one synchronise"})


def probe_registration(icp, n, k, targets, emit):
    tgt, src, T_true = icp.synth_scene(n)
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        ctx.estimate_target_normals(k)
        for metric, name in ((icp.METRIC_POINT, "point"), (icp.METRIC_PLANE, "plane")):
            for rep in range(2):  # the second run of each metric is reported (first launches done)
                ctx.set_source(src)
                ses = ctx.session(icp.params_default(max_iterations=200), metric=metric)
                wall, errs, walls = 0.0, [], []
                while not ses.done:
                    ms, rec = wall_ms(ses.step)
                    wall += ms
                    if rec is not None:
                        errs.append(t_rmse(np.array(rec.transform[:]).reshape(4, 4), T_true))
                        walls.append(wall)
                rc, res = ses.finish()
                ses.close()
            reached = {}
            for t in targets:
                hit = next((i for i, e in enumerate(errs) if e <= t), None)
                reached[f"{t:g}"] = None if hit is None else {"iterations": hit + 1, "wall_ms": round(walls[hit], 2)}
            emit({"figure": "registration", "points": n, "metric": name, "k": k, "rc": rc, "status": res.status,
                  "iterations": len(errs), "wall_ms": round(wall, 2), "final_t_rmse": errs[-1] if errs else None,
                  "best_t_rmse": min(errs) if errs else None, "reached": reached,
                  "clock": "host wall over icp_session_step calls (each ends with its record on the host)"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1000000,10000000")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iterates", type=int, default=10)
    ap.add_argument("--registration-points", type=int, default=1_000_000)
    ap.add_argument("--targets", default="1e-2,3e-3,1e-3,3e-4")
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
        probe_size(icp, n, a.k, a.reps, a.iterates, emit)
    if a.registration_points > 0:
        probe_registration(icp, a.registration_points, a.k, [float(x) for x in a.targets.split(",")], emit)


if __name__ == "__main__":
    main()
