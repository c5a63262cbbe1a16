#!/usr/bin/env python3
"""Timings of outlier removal on the LiDAR-like scene (icp.synth_scene), one GPU process, one JSON
line per figure (DESIGN.md §3.11 quotes them; profiles/outlier/ keeps them):

  outlier       icp_hip_outlier_filter_device on the scene's target, resident in HBM, all three
                outputs: statistical at k = 16 and k = 8 (std_ratio 1), and radius with a minimum of
                8 neighbours and a radius found on the spot by bisection so that the median
                unsaturated count is about 8. One warm call, then over --reps calls the medians of
                the host clock around the call (it ends in a stream synchronise) and of the four
                phases' device times (icp_hip_outlier_last_timing). Compulsory bytes of the scores
                kernel: the 32-B record read and the 8-B score stored per point, 40 n. The
                yardstick of the statistical scores is icp_hip_estimate_target_normals at the same k
                on the same cloud in the same process (the same walk, a heavier epilogue), host
                clock around the call, interleaved with the outlier calls; both are reported with
                the spread of their repetitions.
  registration  the 1M scene thinned by a voxel grid (--edge), then filtered, both metrics with early
                stops on: iterations, host wall over the session's steps and t_rmse against T_true
                at the stop; beside the bare grid and the grid without its one-point voxels. The
                share of the source's injected outliers that survive each thinning.

  outlier_probe.py [--points 1000000,10000000] [--reps 5] [--registration-points 1000000]
                   [--edge 0.425] [--k 16] [--out FILE]

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

PHASES = ("build", "scores", "statistics", "compaction")


def t_rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


def wall_ms(fn, *a, **kw):
    t0 = time.perf_counter()
    out = fn(*a, **kw)
    return (time.perf_counter() - t0) * 1e3, out


def radius_for(median_count, want, lo=1e-3, hi=5.0, steps=14):
    """The radius whose median unsaturated neighbour count is nearest `want`: bisection in log r
    (the count grows with r). median_count(r) -> float."""
    for _ in range(steps):
        mid = (lo * hi) ** 0.5
        if median_count(mid) < want:
            lo = mid
        else:
            hi = mid
    return float(f"{(lo * hi) ** 0.5:.3g}")


def probe_size(icp, n, reps, emit):
    tgt = icp.synth_scene(n, 0)[0]
    with icp.Context(0) as ctx:
        buf = ctx.to_device(tgt)
        dp, di, ds = ctx.device_buffer(24 * n), ctx.device_buffer(4 * n), ctx.device_buffer(8 * n)
        ctx.set_target(tgt)  # the yardstick's octree: the same shape as the call's private one

        def median_count(r):
            ctx.outlier_filter_device(buf, n, icp.OUTLIER_RADIUS, 64, r, d_score_out=ds)
            return float(np.median(ds.download(np.float64)))

        radius = radius_for(median_count, 8.0)
        cases = [("statistical", icp.OUTLIER_STATISTICAL, 16, 1.0), ("statistical", icp.OUTLIER_STATISTICAL, 8, 1.0),
                 ("radius", icp.OUTLIER_RADIUS, 8, radius)]
        for name, mode, k, param in cases:
            call = lambda: ctx.outlier_filter_device(buf, n, mode, k, param, cap=n, d_xyz_out=dp, d_index_out=di,  # noqa: E731
                                                     d_score_out=ds)
            yard = mode == icp.OUTLIER_STATISTICAL and k >= 3
            first, (m, st) = wall_ms(call)
            if yard:
                wall_ms(ctx.estimate_target_normals, k)
            walls, phases, normals = [], [], []
            for _ in range(reps):  # interleaved
                walls.append(wall_ms(call)[0])
                phases.append(ctx.outlier_last_timing())
                if yard:
                    normals.append(wall_ms(ctx.estimate_target_normals, k)[0])
            med = statistics.median(walls)
            ph = np.array(phases)
            phm = np.median(ph, axis=0)
            line = {"figure": "outlier", "points": n, "mode": name, "k": k, "param": param, "kept": m,
                    "mean": st.mean, "std": st.std, "threshold": st.threshold,
                    "first_call_ms": round(first, 3), "median_ms": round(med, 3), "runs_ms": [round(w, 3) for w in walls],
                    "phase_ms_median": {p: round(float(v), 4) for p, v in zip(PHASES, phm)},
                    "scores_ms_runs": [round(float(v), 4) for v in ph[:, 1]],
                    "scores_ms_spread": [round(float(ph[:, 1].min()), 4), round(float(ph[:, 1].max()), 4)],
                    "compulsory_bytes_scores": 40 * n,
                    "scores_GB_per_s": round(40 * n / (float(phm[1]) * 1e-3) / 1e9, 1),
                    "clock": "host around the call (two small read-backs, one final synchronise); phases: HIP events"}
            if yard:
                line.update({"normals_ms_median": round(statistics.median(normals), 3),
                             "normals_ms_runs": [round(w, 3) for w in normals],
                             "normals_ms_spread": [round(min(normals), 3), round(max(normals), 3)],
                             "scores_over_normals": round(float(phm[1]) / statistics.median(normals), 3),
                             "normals_clock": "host around icp_hip_estimate_target_normals (ends in a synchronise)"})
            if mode == icp.OUTLIER_RADIUS:
                line["median_unsaturated_count"] = median_count(param)
            emit(line)
        for b in (buf, dp, di, ds):
            b.free()


def register(icp, tgt, src, T_true, k, label, emit, extra=None):
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
            line = {"figure": "registration", "thinning": label, "target_points": len(tgt), "source_points": len(src),
                    "metric": name, "k": k, "rc": rc, "status": res.status, "iterations": len(errs),
                    "wall_ms": round(wall, 2), "final_t_rmse": errs[-1] if errs else None,
                    "best_t_rmse": min(errs) if errs else None,
                    "clock": "host wall over icp_session_step calls (each ends with its record on the host)"}
            line.update(extra or {})
            emit(line)


def probe_registration(icp, n, edge, k, emit):
    tgt, src, T_true = icp.synth_scene(n)
    clean = icp.synth_scene(n, outlier_fraction=0.0)[1]
    injected = (src != clean).any(1)  # the rows the scene replaced by uniform strays
    del clean
    with icp.Context(0) as ctx:
        vt, _, kt, _ = ctx.voxel_downsample(tgt, edge)
        vs, fs, ks, _ = ctx.voxel_downsample(src, edge)
        stray = injected[fs] & (ks == 1)  # voxels that hold one injected point and nothing else
        n_stray = int(stray.sum())

        def share(mask):
            return {"source_stray_voxels": n_stray, "source_stray_voxels_kept": int((stray & mask).sum()),
                    "stray_share_surviving": round(float((stray & mask).sum()) / max(n_stray, 1), 4),
                    "source_surface_voxels_dropped": int((~stray & ~mask).sum())}

        emit({"figure": "registration_thinning", "points": n, "edge_m": edge, "injected_source_points": int(injected.sum()),
              "voxel_points": [len(vt), len(vs)], "source_stray_voxels": n_stray,
              "voxels_of_one_point": [int((kt == 1).sum()), int((ks == 1).sum())]})
        all_s = np.ones(len(vs), bool)
        register(icp, vt, vs, T_true, k, f"voxel {edge} m", emit, share(all_s))
        register(icp, vt[kt >= 2], vs[ks >= 2], T_true, k, f"voxel {edge} m, voxels of >= 2 points", emit, share(ks >= 2))
        for sk, ratio in ((8, 1.0), (16, 1.0), (8, 2.0)):
            ms_t, (ft, _, _, st_t) = wall_ms(ctx.outlier_filter, vt, icp.OUTLIER_STATISTICAL, sk, ratio)
            ms_s, (fsrc, ix, _, st_s) = wall_ms(ctx.outlier_filter, vs, icp.OUTLIER_STATISTICAL, sk, ratio)
            mask = np.zeros(len(vs), bool)
            mask[ix] = True
            extra = share(mask)
            extra.update({"filter_calls_ms": [round(ms_t, 2), round(ms_s, 2)],
                          "thresholds": [st_t.threshold, st_s.threshold]})
            register(icp, ft, fsrc, T_true, k, f"voxel {edge} m, sor k={sk} ratio={ratio:g}", emit, extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--registration-points", type=int, default=1_000_000)
    ap.add_argument("--edge", type=float, default=0.425)
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
        probe_registration(icp, a.registration_points, a.edge, a.k, emit)


if __name__ == "__main__":
    main()
