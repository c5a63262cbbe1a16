"""The chunked LAS record reader of the device decode (iterativeclosestpoint_amd/csrc/las_chunks.cpp:
host code, no HIP call) under AddressSanitizer + UndefinedBehaviorSanitizer: the Makefile target
`las_asan` builds tests/cpp/las_chunks_sanitize.cpp with it, and the program reads five files
(well-formed, cut five records short, cut in the middle of a record, with a gap of variable-length
records in front of the points, zero-length) with chunk buffers of exactly the capacity it states.
CPU only."""
import os
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "iterativeclosestpoint_amd" / "csrc"
EXE = ROOT / "build" / "sanitize" / "las_chunks_asan"


def _files(icp, tmp_path):
    rng = np.random.default_rng(11)
    n = 1000
    xyz = rng.uniform(-50.0, 50.0, (n, 3))
    good = tmp_path / "good.las"
    icp.las_write_cli(good, xyz, (0.001,) * 3, (0.0,) * 3)
    blob = good.read_bytes()
    assert len(blob) == 227 + 20 * n
    short = tmp_path / "short5.las"
    short.write_bytes(blob[:-5 * 20])
    mid = tmp_path / "midrecord.las"
    mid.write_bytes(blob[:-7])
    # 148 bytes of variable-length records between header and points, 34-byte records
    head = bytearray(blob[:227])
    head[96:100] = (375).to_bytes(4, "little")
    head[105:107] = (34).to_bytes(2, "little")
    rec = np.zeros((n, 34), np.uint8)
    rec[:, :20] = np.frombuffer(blob[227:], np.uint8).reshape(n, 20)
    rec[:, 20:] = rng.integers(0, 256, (n, 14), dtype=np.uint8)
    gap = tmp_path / "vlr_gap.las"
    gap.write_bytes(bytes(head) + rng.integers(0, 256, 148, dtype=np.uint8).tobytes() + rec.tobytes())
    empty = tmp_path / "empty.las"
    empty.write_bytes(b"")
    return {good: (0, n, 1), short: (0, n, 0), mid: (0, n, 0), gap: (0, n, 1), empty: (-1, 0, 0)}


def test_chunk_reader_under_sanitizer(icp, tmp_path):
    r = subprocess.run(["make", "-C", str(CSRC), "las_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    files = _files(icp, tmp_path)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    run = subprocess.run([str(EXE), *map(str, files)], capture_output=True, text=True, timeout=300, env=env)
    report = run.stdout[-2000:] + run.stderr[-6000:]
    assert run.returncode == 0, report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, report
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok", report
    # what the reader made of each file (CLI rules, no point limit)
    for line, (path, (rc, n, well)) in zip(lines, files.items()):
        assert line == f"{path} rc={rc} n={n} well_formed={well}", report
