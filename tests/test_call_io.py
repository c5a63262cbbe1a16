"""A call's input upload and optional outputs in its host and device forms (csrc/call_io.h), without
a GPU: the stand-alone program tests/cpp/call_io_sanitize.cpp under ASan + UBSan, with its own
hipMalloc / hipFree / hipMemcpyAsync (a copy outside a live or host buffer aborts) and every
allocation of a call-shaped scope failed in turn."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "iterativeclosestpoint_amd" / "csrc"
EXE = ROOT / "build" / "sanitize" / "call_io_asan"
ALLOCS = 3  # of the program's scope: the upload and two outputs asked for


def test_outputs_and_upload_under_sanitizer():
    r = subprocess.run(["make", "-C", str(CSRC), "call_io_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    run = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300, env=env)
    report = run.stdout[-2000:] + run.stderr[-6000:]
    assert run.returncode == 0, report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, report
    lines = run.stdout.strip().splitlines()
    # the forms, then no failure, each allocation failed in turn, one past the last
    assert lines[0] == "forms fine" and lines[-1] == "ok" and len(lines) == 1 + ALLOCS + 2 + 1, report
    for k, line in zip(range(-1, ALLOCS + 1), lines[1:-1]):
        made = ALLOCS if k < 0 or k >= ALLOCS else k
        assert line == f"fail_at {k:2d}: {made} allocations, {made} frees, fine", report
