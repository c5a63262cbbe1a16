"""DevScratch, the owner of call-lifetime device memory (csrc/dev_scratch.h), without a GPU: the
stand-alone program tests/cpp/dev_scratch_sanitize.cpp under ASan + UBSan, with its own hipMalloc /
hipFree and every allocation of a call-shaped scope failed in turn."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "iterativeclosestpoint_amd" / "csrc"
EXE = ROOT / "build" / "sanitize" / "dev_scratch_asan"
ALLOCS = 5  # of the program's scope


def test_ownership_under_sanitizer():
    r = subprocess.run(["make", "-C", str(CSRC), "scratch_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    run = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300, env=env)
    report = run.stdout[-2000:] + run.stderr[-6000:]
    assert run.returncode == 0, report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, report
    lines = run.stdout.strip().splitlines()
    # no failure, each allocation failed in turn, one past the last
    assert lines[-1] == "ok" and len(lines) == ALLOCS + 2 + 1, report
    assert all(line.endswith("fine") for line in lines[:-1]), report
    for k, line in zip(range(-1, ALLOCS + 1), lines):
        made = ALLOCS if k < 0 or k >= ALLOCS else k
        kept = 1 if made == ALLOCS else 0
        assert line == f"fail_at {k:2d}: {made} allocations, {made - kept} frees, fine", report
