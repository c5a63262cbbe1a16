#!/usr/bin/env python3
"""Timings of voxel-grid down-sampling on the LiDAR-like scene (icp.synth_scene), one GPU process,
one JSON line per figure (DESIGN.md §3.10 quotes them; profiles/voxel/ keeps them):

  voxel         icp_hip_voxel_downsample_device on the scene's target, resident in HBM, all three
                outputs, at two voxel edges found on the spot by bisection on the count-only call
                (reductions of about 1/4 and about 1/50): one warm call, then the medians over
                --reps calls of the host clock around the call (it ends in a stream synchronise) and
                of the five phases' device times (icp_hip_voxel_last_timing). Compulsory bytes:
                24 n read + 32 m written; their rate over the reduce kernel and over the call. The
                sort's own traffic per pass, 8-B keys and 4-B indices read and written, is listed
                apart. The yardstick is icp_voxel_downsample (the host function, one core, same box).
  registration  the 1M scene thinned by the record stride 50 against a voxel edge that leaves about
                as many points, both metrics with early stops on: iterations, host wall over the
                session's steps and t_rmse against T_true at the stop.

  voxel_probe.py [--points 1000000,10000000] [--reps 5] [--registration-points 1000000]
                 [--stride 50] [--k 16] [--out FILE]

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

PHASES = ("bounds", "keys", "sort", "runs", "reduce")


def t_rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


def wall_ms(fn, *a, **kw):
    t0 = time.perf_counter()
    out = fn(*a, **kw)
    return (time.perf_counter() - t0) * 1e3, out


def edge_for(count, n, want, lo=1e-3, hi=50.0, steps=24):
    """The voxel edge whose voxel count is nearest n * want: bisection in log h (the count falls
    with h). count(h) -> m."""
    for _ in range(steps):
        mid = (lo * hi) ** 0.5
        if count(mid) > n * want:
            lo = mid
        else:
            hi = mid
    return float(f"{(lo * hi) ** 0.5:.3g}")


def probe_size(icp, n, reps, emit):
    tgt = icp.synth_scene(n, 0)[0]
    with icp.Context(0) as ctx:
        buf = ctx.to_device(tgt)
        dp, df, dk = ctx.device_buffer(24 * n), ctx.device_buffer(4 * n), ctx.device_buffer(4 * n)
        count = lambda h: ctx.voxel_downsample_device(buf, n, h)[0]  # noqa: E731
        for want in (1 / 4, 1 / 50):
            h = edge_for(count, n, want)
            call = lambda: ctx.voxel_downsample_device(buf, n, h, cap=n, d_xyz_out=dp, d_first_out=df,  # noqa: E731
                                                       d_count_out=dk)
            first, (m, _) = wall_ms(call)
            walls, phases = [], []
            for _ in range(reps):
                walls.append(wall_ms(call)[0])
                phases.append(ctx.voxel_last_timing())
            med = statistics.median(walls)
            ph = np.median(np.array(phases), axis=0)
            nbytes = 24 * n + 32 * m
            cells = np.floor((tgt.max(0) - tgt.min(0)) / h).astype(np.int64)  # the largest cell per axis
            top = max(a for a in range(3) if cells[a] > 0 or a == 0)
            key_bits = 21 * top + max(1, int(cells[top]).bit_length())  # the sort's end bit
            host_ms, (hp, hf, hk, _) = wall_ms(icp.voxel_downsample, tgt, h)
            same = (hp.tobytes() == dp.download(np.float64, (n, 3))[:m].tobytes()
                    and hf.tobytes() == df.download(np.int32)[:m].tobytes()
                    and hk.tobytes() == dk.download(np.int32)[:m].tobytes())
            emit({"figure": "voxel", "points": n, "edge_m": h, "voxels": m, "reduction": round(m / n, 4),
                  "largest_voxel": int(hk.max()), "first_call_ms": round(first, 3), "median_ms": round(med, 3),
                  "runs_ms": [round(w, 3) for w in walls],
                  "phase_ms_median": {p: round(float(v), 4) for p, v in zip(PHASES, ph)},
                  "compulsory_bytes": nbytes,
                  "reduce_GB_per_s": round(nbytes / (float(ph[4]) * 1e-3) / 1e9, 1),
                  "call_GB_per_s": round(nbytes / (med * 1e-3) / 1e9, 1),
                  "sort_bytes_per_pass": 2 * 12 * n, "sort_key_bits": key_bits,
                  "host_one_core_ms": round(host_ms, 1), "host_over_device": round(host_ms / med, 1),
                  "same_bits_as_host": bool(same),
                  "clock": "host around the call (two small read-backs, one final synchronise); phases: HIP events"})
        for b in (buf, dp, df, dk):
            b.free()


def register(icp, tgt, src, T_true, k, label, emit):
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        ctx.estimate_target_normals(k)
        for metric, name in ((icp.METRIC_POINT, "point"), (icp.METRIC_PLANE, "plane")):
            for rep in range(2):  # the second run of each metric is reported (first launches done)
                ctx.set_source(src)
                ses = ctx.session(icp.params_default(max_iterations=200), metric=metric)
                wall, errs = 0.0, []
                while not ses.done:
                    ms, rec = wall_ms(ses.step)
                    wall += ms
                    if rec is not None:
                        errs.append(t_rmse(np.array(rec.transform[:]).reshape(4, 4), T_true))
                rc, res = ses.finish()
                ses.close()
            emit({"figure": "registration", "thinning": label, "target_points": len(tgt), "source_points": len(src),
                  "metric": name, "k": k, "rc": rc, "status": res.status, "iterations": len(errs),
                  "wall_ms": round(wall, 2), "final_t_rmse": errs[-1] if errs else None,
                  "best_t_rmse": min(errs) if errs else None,
                  "clock": "host wall over icp_session_step calls (each ends with its record on the host)"})


def probe_registration(icp, n, stride, k, emit):
    tgt, src, T_true = icp.synth_scene(n)
    st, ss = tgt[::stride], src[::stride]
    register(icp, st, ss, T_true, k, f"stride {stride}", emit)
    with icp.Context(0) as ctx:
        buf = ctx.to_device(tgt)
        h = edge_for(lambda e: ctx.voxel_downsample_device(buf, n, e)[0], n, 1.0 / stride)
        buf.free()
        ms_t, (vt, _, kt, _) = wall_ms(ctx.voxel_downsample, tgt, h)
        ms_s, (vs, _, ks, _) = wall_ms(ctx.voxel_downsample, src, h)
    emit({"figure": "registration_thinning", "points": n, "stride": stride, "edge_m": h, "stride_points": [len(st), len(ss)],
          "voxel_points": [len(vt), len(vs)], "voxels_of_one_point": [int((kt == 1).sum()), int((ks == 1).sum())],
          "voxel_calls_ms": [round(ms_t, 2), round(ms_s, 2)],
          "clock": "host around icp_hip_voxel_downsample (upload, core, download)"})
    register(icp, vt, vs, T_true, k, f"voxel {h} m", emit)
    # the scene's source carries isolated outliers: each keeps a voxel of its own, so the grid raises
    # their share; the count output is what a caller filters them with
    register(icp, vt[kt >= 2], vs[ks >= 2], T_true, k, f"voxel {h} m, voxels of >= 2 points", emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--registration-points", type=int, default=1_000_000)
    ap.add_argument("--stride", type=int, default=50)
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
        probe_size(icp, n, a.reps, emit)
    if a.registration_points > 0:
        probe_registration(icp, a.registration_points, a.stride, a.k, emit)


if __name__ == "__main__":
    main()
