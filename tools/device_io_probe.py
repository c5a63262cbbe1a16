#!/usr/bin/env python3
"""Host-timed phases around a registration: the host route (LAS read on the host, stride, LAS
written on the host, clouds uploaded, source downloaded) against the device route (--device-io:
records decoded / encoded by kernels, clouds resident). DESIGN.md §3.8 holds the table.

One child process per configuration and repetition (a fresh process: no warm caches of the other
route); the parent interleaves the routes and prints one JSON line per configuration with the
medians. Library phases are timed around the C calls the CLI itself makes; `cli_*` is the wall time
of bin/icp_registration as a whole.

  device_io_probe.py [--points 10000000] [--reps 5] [--sample-rates 1,50] [--record-lengths 20,34]
                     [--workdir DIR] [--out FILE]

ICP_HIP_LIB selects another build of the library for the host route (a parent commit's, which has
no device route: its device phases are skipped).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
EXE = ROOT / "iterativeclosestpoint_amd" / "bin" / "icp_registration"


class Clock:
    def __init__(self):
        self.ms = {}

    def __call__(self, name, fn, *a, **kw):
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        self.ms[name] = self.ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
        return out


def make_pair(workdir: Path, points: int, record_length: int):
    """A synthetic LAS pair; record_length > 20 pads the writer's records (the header patched)."""
    import iterativeclosestpoint_amd as icp

    src_p, tgt_p = workdir / f"src_{points}_{record_length}.las", workdir / f"tgt_{points}_{record_length}.las"
    if src_p.exists() and tgt_p.exists():
        return src_p, tgt_p
    tgt, src, _ = icp.synth_pair(points, yaw_deg=3.0)
    for path, xyz in ((src_p, src), (tgt_p, tgt)):
        icp.las_write_cli(path, xyz, (0.001,) * 3, (0.0,) * 3)
        if record_length != 20:
            blob = path.read_bytes()
            head = bytearray(blob[:227])
            head[105:107] = int(record_length).to_bytes(2, "little")
            rec = np.zeros((points, record_length), np.uint8)
            rec[:, :20] = np.frombuffer(blob, np.uint8, offset=227).reshape(points, 20)
            path.write_bytes(bytes(head) + rec.tobytes())
    return src_p, tgt_p


def child_host(src_p, tgt_p, rate, outdir):
    """The default CLI flow's phases through the same library calls."""
    import iterativeclosestpoint_amd as icp

    clk = Clock()
    src, hs = clk("read", icp.las_read, src_p)
    tgt, _ = clk("read", icp.las_read, tgt_p)
    ss = clk("sample", lambda: np.ascontiguousarray(src[::rate]))
    ts = clk("sample", lambda: np.ascontiguousarray(tgt[::rate]))
    sc, of = tuple(hs.scale), tuple(hs.offset)
    clk("write_sampled", icp.las_write_cli, outdir / "sampled_source.las", ss, sc, of)
    clk("write_sampled", icp.las_write_cli, outdir / "sampled_target.las", ts, sc, of)
    with icp.Context(0) as ctx:
        clk("set_target", ctx.set_target, ts, 10, 20, icp.RULES_CLI)
        clk("set_source", ctx.set_source, ss)
        p = icp.params_default(max_iterations=20, tolerance=1e-2, rules=icp.RULES_CLI)
        clk("registration", ctx.run, p, 20)
        moved = clk("get_source", ctx.get_source)
    clk("write_registered", icp.las_write_cli, outdir / "registered_source.las", moved, sc, of)
    clk("write_registered", icp.las_write_cli, outdir / "registered_target.las", ts, sc, of)
    return clk.ms


def child_device(src_p, tgt_p, rate, outdir):
    """--device-io's phases through the same library calls."""
    import iterativeclosestpoint_amd as icp

    clk = Clock()
    with icp.Context(0) as ctx:
        _, hs = clk("read+sample+set_source", ctx.set_source_las, src_p, icp.LAS_CLI, 0, rate)
        d_tgt, nt, _ = clk("read+sample", ctx.read_las_device, tgt_p, icp.LAS_CLI, 0, rate)
        sc, of = tuple(hs.scale), tuple(hs.offset)
        clk("write_sampled", ctx.write_source_las, outdir / "sampled_source.las", icp.LAS_CLI, sc, of)
        clk("write_sampled", ctx.write_las_device, outdir / "sampled_target.las", d_tgt, nt, icp.LAS_CLI, sc, of)
        clk("set_target", ctx.set_target_device, d_tgt, nt, 10, 20, icp.RULES_CLI)
        p = icp.params_default(max_iterations=20, tolerance=1e-2, rules=icp.RULES_CLI)
        clk("registration", ctx.run, p, 20)
        clk("write_registered", ctx.write_source_las, outdir / "registered_source.las", icp.LAS_CLI, sc, of)
        clk("write_registered", ctx.write_las_device, outdir / "registered_target.las", d_tgt, nt, icp.LAS_CLI, sc, of)
        paths = ctx.last_las_path()
        d_tgt.free()
    clk.ms["device_path"] = paths
    return clk.ms


def child_clouds(points):
    """set_source / get_source against their device variants, and the raw copies, at `points`."""
    import iterativeclosestpoint_amd as icp

    clk = Clock()
    _, src, _ = icp.synth_pair(points, yaw_deg=3.0)
    with icp.Context(0) as ctx:
        ctx.set_source(src[:4096])  # first-launch costs out of the way
        with ctx.device_buffer(src.nbytes) as d:
            clk("h2d_copy", d.upload, src)
            clk("set_source", ctx.set_source, src)
            clk("set_source_device", ctx.set_source_device, d, points)
            clk("get_source", ctx.get_source)
            clk("get_source_device", ctx.get_source_device, d)
            clk("d2h_copy", d.download, np.float64)
    return clk.ms


def child_codec(path, points):
    """Decode and encode of a whole file against the plain copies of the same bytes (file cached)."""
    import iterativeclosestpoint_amd as icp

    clk = Clock()
    raw = np.fromfile(path, np.uint8)
    with icp.Context(0) as ctx:
        ctx.read_las_device(path)[0].free()  # buffers made, file in the page cache
        with ctx.device_buffer(raw.nbytes) as d:
            clk("h2d_copy_raw_pageable", d.upload, raw)
        buf, n, hdr = clk("read_las_device", ctx.read_las_device, path)
        out = Path(str(path) + ".probe_out")
        clk("write_las_device", ctx.write_las_device, out, buf, n, icp.LAS_CLI, tuple(hdr.scale), tuple(hdr.offset))
        clk("d2h_copy_fp64", buf.download, np.float64)
        buf.free()
        out.unlink()
    return clk.ms


def run_cli(src_p, tgt_p, rate, outdir, device_io):
    t0 = time.perf_counter()
    r = subprocess.run([str(EXE), "--source", str(src_p), "--target", str(tgt_p), "--sample-rate", str(rate),
                        "--outdir", str(outdir)] + (["--device-io"] if device_io else []),
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stdout[-1000:] + r.stderr[-1000:])
    return (time.perf_counter() - t0) * 1e3


def spawn(spec: dict) -> dict:
    r = subprocess.run([sys.executable, __file__, "--child", json.dumps(spec)], capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"child {spec} failed:\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def medians(rows):
    keys = sorted({k for r in rows for k in r})
    return {k: round(statistics.median(r[k] for r in rows if k in r), 2) for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample-rates", default="1,50")
    ap.add_argument("--record-lengths", default="20,34")
    ap.add_argument("--workdir", default="/tmp/icp_device_io_probe")
    ap.add_argument("--out", default="")
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()

    if a.child:
        s = json.loads(a.child)
        outdir = Path(s.get("outdir", "."))
        kind = s["kind"]
        if kind == "host":
            ms = child_host(Path(s["src"]), Path(s["tgt"]), s["rate"], outdir)
        elif kind == "device":
            ms = child_device(Path(s["src"]), Path(s["tgt"]), s["rate"], outdir)
        elif kind == "clouds":
            ms = child_clouds(s["points"])
        else:
            ms = child_codec(Path(s["src"]), s["points"])
        print(json.dumps(ms))
        return

    work = Path(a.workdir)
    work.mkdir(parents=True, exist_ok=True)
    have_device = "ICP_HIP_LIB" not in os.environ
    lines = []
    for rl in [int(x) for x in a.record_lengths.split(",")]:
        src_p, tgt_p = make_pair(work, a.points, rl)
        for rate in [int(x) for x in a.sample_rates.split(",")]:
            rows = {"host": [], "device": [], "cli_host": [], "cli_device": []}
            for rep in range(a.reps):  # interleaved: host, device, host, device, ...
                for kind in ("host", "device"):
                    if kind == "device" and not have_device:
                        continue
                    out = work / f"out_{kind}"
                    out.mkdir(exist_ok=True)
                    rows[kind].append(spawn({"kind": kind, "src": str(src_p), "tgt": str(tgt_p), "rate": rate,
                                             "outdir": str(out)}))
                    if not a.no_cli:
                        rows[f"cli_{kind}"].append({"wall": run_cli(src_p, tgt_p, rate, out, kind == "device")})
            line = {"points": a.points, "record_length": rl, "sample_rate": rate, "reps": a.reps,
                    **{k: medians(v) for k, v in rows.items() if v}}
            lines.append(line)
            print(json.dumps(line), flush=True)
        if have_device:
            line = {"points": a.points, "record_length": rl,
                    "codec": medians([spawn({"kind": "codec", "src": str(src_p), "points": a.points})
                                      for _ in range(a.reps)])}
            lines.append(line)
            print(json.dumps(line), flush=True)
    if have_device:
        line = {"points": a.points,
                "clouds": medians([spawn({"kind": "clouds", "points": a.points}) for _ in range(a.reps)])}
        lines.append(line)
        print(json.dumps(line), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
