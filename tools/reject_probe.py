#!/usr/bin/env python3
"""Timings of the rejectors on the LiDAR-like scene (icp.synth_scene), one GPU process, one JSON
line per figure (DESIGN.md §3.12 quotes them; profiles/reject/ keeps them). After each iterate of a
trimmed plane session stepped by hand, the host clock around each call (every one ends in a stream
synchronise), beside the iterate's own device time (icp_hip_last_timing, timing_stride 1):

  residual_select  icp_hip_residual_select(0.5): a memset, the digit passes, a 64-B copy, one
                   synchronise. It reads the residuals `full_reads` times: 8 full_reads bytes per query.
  pair_sums        icp_hip_pair_sums at the selected threshold. Compulsory bytes per query: dist 8 B for
                   the first-pair pass, then dist 8 B and for a valid pair the source 24 B, pos 4 B and
                   the gathered target record at 64-B line granularity.
  plane_sums_at    icp_hip_plane_sums_at at the same threshold, with icp_hip_plane_sums beside it (the
                   iterate's own threshold: about twice the pairs at a fraction of 0.5).

  reject_probe.py [--points 100000,1000000,10000000] [--k 16] [--iterates 10] [--fraction 0.5] [--out FILE]

Every step raises on a failing call; the process then exits non-zero and nothing further runs.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FULL_READS = 6  # reject_kernels.hip kSelectPasses: every digit pass reads all of dist


def wall_ms(fn, *a, **kw):
    t0 = time.perf_counter()
    out = fn(*a, **kw)
    return (time.perf_counter() - t0) * 1e3, out


def med(v):
    return round(statistics.median(v[1:]), 4)  # the first call makes the call's buffers


def probe_size(icp, n, k, iterates, fraction, emit):
    tgt, src, _ = icp.synth_scene(n)
    with icp.Context(0, cfg={"timing_stride": 1}) as ctx:
        ctx.set_target(tgt)
        ctx.estimate_target_normals(k)
        ctx.set_source(src)
        t = {name: [] for name in ("select", "pair", "plane_at", "plane", "iterate", "search")}
        valid, valid_sigma = [], []
        T = None
        for it in range(iterates):
            st = ctx.iterate(T, it, icp.RULES_ENGINE, 3.0)
            a, b = ctx.last_timing()
            ms_sel, sel = wall_ms(ctx.residual_select, fraction)
            ms_pair, ps = wall_ms(ctx.pair_sums, sel.value)
            ms_at, s = wall_ms(ctx.plane_sums_at, ps.centroid_src, sel.value)
            ms_pl, _ = wall_ms(ctx.plane_sums, st.centroid_src)
            T, ok = icp.plane_solve(s)
            if not ok:
                st.centroid_src[:], st.centroid_tgt[:], st.H[:] = ps.centroid_src[:], ps.centroid_tgt[:], ps.H[:]
                T = icp.best_fit_from_stats(st)
            for name, ms in (("select", ms_sel), ("pair", ms_pair), ("plane_at", ms_at), ("plane", ms_pl),
                             ("iterate", b), ("search", a)):
                t[name].append(ms)
            valid.append(ps.valid)
            valid_sigma.append(st.valid)
        sel_ms = med(t["select"])
        pair_bytes = 8 + 8 + fraction * (24 + 4 + 64)
        emit({"figure": "residual_select", "points": n, "fraction": fraction, "iterates": iterates,
              "first_call_ms": round(t["select"][0], 4), "median_ms": sel_ms,
              "runs_ms": [round(r, 4) for r in t["select"]], "full_reads": FULL_READS,
              "bytes_per_query": 8 * FULL_READS,
              "GB_per_s_at_median": round(n * 8 * FULL_READS / (sel_ms * 1e-3) / 1e9, 1),
              "clock": "host around the call: a memset, seven launches, a 64-B copy, one synchronise"})
        emit({"figure": "pair_sums", "points": n, "first_call_ms": round(t["pair"][0], 4), "median_ms": med(t["pair"]),
              "runs_ms": [round(r, 4) for r in t["pair"]], "valid_median": int(statistics.median(valid)),
              "bytes_per_query": round(pair_bytes, 1),
              "compulsory_GB_per_s_at_median": round(n * pair_bytes / (med(t["pair"]) * 1e-3) / 1e9, 1),
              "clock": "host around the call: a memset, three launches, a 168-B copy, one synchronise"})
        emit({"figure": "plane_sums_at", "points": n, "first_call_ms": round(t["plane_at"][0], 4),
              "median_ms": med(t["plane_at"]), "runs_ms": [round(r, 4) for r in t["plane_at"]],
              "plane_sums_median_ms": med(t["plane"]), "valid_median": int(statistics.median(valid)),
              "valid_sigma_median": int(statistics.median(valid_sigma)),
              "clock": "host around the call: two launches, a 256-B copy, one synchronise"})
        emit({"figure": "iterate", "points": n, "iterate_device_ms_median": med(t["iterate"]),
              "search_kernel_ms_median": med(t["search"]),
              "rejector_step_ms_median": round(sel_ms + med(t["pair"]) + med(t["plane_at"]), 4),
              "clock": "HIP events of the iterate (timing_stride 1)"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="100000,1000000,10000000")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--iterates", type=int, default=10)
    ap.add_argument("--fraction", type=float, default=0.5)
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
        probe_size(icp, n, a.k, a.iterates, a.fraction, emit)


if __name__ == "__main__":
    main()
