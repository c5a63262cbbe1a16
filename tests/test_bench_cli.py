"""bench.py's command line: --dump-outputs (what the timed path's last step left, as .npy) and the
plain line against --full (the legs beside the headline figure run only there)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
DUMPED = ("transform", "sample_rows", "source_moved", "correspondence_index", "correspondence_distance")
FULL_ONLY = ("search_paths", "reference_work", "cpu_baseline", "cpu_allcores", "parity", "timed_state_parity",
             "registration")


class _FakeCtx:
    def __init__(self, n):
        self.moved = np.arange(3 * n, dtype=np.float64).reshape(n, 3)

    def get_source(self):
        return self.moved

    def get_correspondences(self):
        n = len(self.moved)
        return np.arange(n, dtype=np.int32)[::-1].copy(), np.linspace(0.0, 1.0, n)


class _FakeSession:
    def transform(self):
        return np.eye(4)


def _load(d):
    return {k: np.load(d / f"{k}.npy") for k in DUMPED}


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    import bench

    n = bench.DUMP_SAMPLE + 12345  # above the sample size: a seeded sample of rows, the same every time
    ctx = _FakeCtx(n)
    bench.dump_outputs(str(tmp_path / "a"), ctx, _FakeSession())
    bench.dump_outputs(str(tmp_path / "b"), ctx, _FakeSession())
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(f"{k}.npy" for k in DUMPED)
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    for k in DUMPED:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
    rows = a["sample_rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_SAMPLE and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert np.array_equal(a["source_moved"], ctx.moved[rows])
    assert np.array_equal(a["correspondence_index"], (n - 1 - rows).astype(np.float64))
    assert np.array_equal(a["correspondence_distance"], np.linspace(0.0, 1.0, n)[rows])


def test_dump_outputs_small_cloud_is_whole(tmp_path):
    import bench

    ctx = _FakeCtx(1000)
    bench.dump_outputs(str(tmp_path), ctx, _FakeSession())
    a = _load(tmp_path)
    assert np.array_equal(a["sample_rows"], np.arange(1000.0)) and np.array_equal(a["source_moved"], ctx.moved)


def _bench(*args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--points", "20000", *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout  # one JSON line
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dump(icp, tmp_path):
    j = _bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / "d1"))
    assert j["steps"] == 7 and j["warmup"] == 2 and j["unit"] == "Mcorr/s" and j["dtype"] == "f64"
    assert j["higher_is_better"] is True and j["ms_per_step"] > 0 and j["first_iteration"] is not None
    assert j["value"] == pytest.approx(20000 / j["ms_per_step"] / 1e3, rel=1e-2)  # both rounded in the line
    for k in FULL_ONLY:
        assert j[k] is None, k
    a = _load(tmp_path / "d1")
    assert a["source_moved"].shape == (20000, 3) and a["transform"].shape == (4, 4)
    assert all(v.dtype == np.float64 for v in a.values())
    # the dumped arrays belong together: each residual is the distance from the moved point to the
    # target point its index names (same fp64 differences; a few ulp from the sum and the root)
    tgt, src, _ = icp.synth_pair(20000)
    idx = a["correspondence_index"].astype(np.int64)
    d = np.linalg.norm(a["source_moved"] - tgt[idx], axis=1)
    np.testing.assert_allclose(d, a["correspondence_distance"], rtol=1e-12, atol=1e-15)
    # and that target point is the nearest one: brute force over all targets for 300 seeded rows
    rows = np.random.default_rng(7).choice(20000, size=300, replace=False)
    d2 = sum((a["source_moved"][rows, k, None] - tgt[None, :, k]) ** 2 for k in range(3))
    assert np.array_equal(d2.argmin(axis=1), idx[rows])
    np.testing.assert_allclose(np.sqrt(d2.min(axis=1)), a["correspondence_distance"][rows], rtol=1e-12, atol=1e-15)
    # the same arguments give the same inputs and outputs
    _bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / "d2"))
    b = _load(tmp_path / "d2")
    for k in DUMPED:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_full_bench_line_has_the_legs(icp):
    # --warmup 0: no untimed step, so the line has no first iteration beside the timed ones
    j = _bench("--steps", "3", "--warmup", "0", "--full", "--cpu-sample", "5000")
    assert j["steps"] == 3 and j["warmup"] == 0 and j["first_iteration"] is None and j["ms_per_step"] > 0
    assert j["timed_state_parity"]["iterate"] == 3
    for k in FULL_ONLY:
        assert j[k] is not None, k
    assert j["timed_state_parity"]["idx_mismatch"] == 0 and j["timed_state_parity"]["dist_mismatch"] == 0
    assert j["parity"]["final_transform_rmse_vs_cpu"] <= 1e-6
    assert j["search_paths"]["queries"] == 20000
