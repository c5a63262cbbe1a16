"""CPU checks of the rejectors (no GPU): icp_trim_rank against its formula, the new entry points in
the headers, the library and the binding, and the premises of the GPU tests on the partial-overlap
fixture by a numpy loop (reject_fixtures.numpy_icp): the reference's cull ends worse than it started,
the trimmed rule better, with either metric."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import reject_fixtures as rf

ROOT = Path(__file__).resolve().parents[1]


def _formula(f, n):
    return max(min(3, n), min(n, int(np.float64(f) * np.float64(n))))  # one fp64 product, one truncation


SIZES = [1, 2, 3, 4, 10, 2 ** 29]
FRACTIONS = [1e-9, 0.1, 0.5, 1.0 - 2.0 ** -53, 1.0]


@pytest.mark.parametrize("n", SIZES)
def test_trim_rank_is_the_formula(icp, n):
    for f in FRACTIONS:
        assert icp.trim_rank(f, n) == _formula(f, n), (f, n)
    assert icp.trim_rank(1.0, n) == n and icp.trim_rank(1e-9, n) == min(3, n)
    assert 1 <= icp.trim_rank(0.5, n) <= n


def test_trim_rank_on_either_side_of_an_integer(icp):
    """f n just below, on and just above an integer k: the truncation gives k - 1, k, k."""
    for n, k in ((10, 7), (1000, 333), (4193, 2096), (2 ** 29, 2 ** 28 + 12345)):
        on = k / n
        f_lo, f_hi = on, on
        while np.float64(f_lo) * np.float64(n) >= k:
            f_lo = np.nextafter(f_lo, 0.0)
        while np.float64(f_hi) * np.float64(n) < k:
            f_hi = np.nextafter(f_hi, 1.0)
        assert icp.trim_rank(float(f_lo), n) == k - 1 == _formula(f_lo, n), (n, k)
        assert icp.trim_rank(float(f_hi), n) == k == _formula(f_hi, n), (n, k)
        assert icp.trim_rank(float(np.nextafter(f_hi, 1.0)), n) == _formula(np.nextafter(f_hi, 1.0), n)


def test_trim_rank_refuses_a_bad_fraction(icp):
    for f in (0.0, -0.5, 1.0 + 2.0 ** -52, float("nan"), float("inf")):
        assert icp.trim_rank(f, 100) == 0
    assert icp.trim_rank(0.5, -1) == 0 and icp.trim_rank(0.5, 0) == 0


def test_symbols_and_constants(icp):
    hip = (ROOT / "include" / "icp_hip.h").read_text()
    eng = (ROOT / "include" / "icp_engine.h").read_text()
    host = (ROOT / "include" / "icp_host.h").read_text()
    lib = ctypes.CDLL(str(icp.LIB_PATH))
    for name, text in (("icp_hip_residual_select", hip), ("icp_hip_pair_sums", hip), ("icp_hip_plane_sums_at", hip),
                       ("icp_session_set_rejection", eng), ("icp_engine_run_options", eng),
                       ("icp_run_options_default", eng), ("icp_trim_rank", host)):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in icp._lib.SIGNATURES
    for k, name in enumerate(("SIGMA", "TRIM", "MAX_DIST")):
        assert re.search(r"#define\s+ICP_REJECT_" + name + r"\s+" + str(k) + r"\b", eng)
        assert getattr(icp, "REJECT_" + name) == k
    assert re.search(r"#define\s+ICP_RUN_OPTIONS_VERSION\s+1u?\b", eng) and icp.RUN_OPTIONS_VERSION == 1
    o = icp.run_options()
    assert (o.version, o.metric, o.reject, o.reject_param) == (1, icp.METRIC_POINT, icp.REJECT_SIGMA, 0.0)
    assert ctypes.sizeof(icp.SelectResult) == 40 and ctypes.sizeof(icp.PairSums) == 160
    assert ctypes.sizeof(icp.RunOptions) == 24


def test_fixture_is_the_stated_one():
    tgt, src, T, overlap = rf.overlap_pair()
    assert (len(tgt), len(src)) == (4178, 4193) and abs(overlap - 0.568) < 5e-4
    assert abs(rf.t_rmse(np.eye(4), T) - 0.0280) < 5e-5


def test_premises_point_to_point():
    """After 20 iterations the cull is above the initial error and at least 5 times the trimmed
    rule, which is below it."""
    tgt, src, T, _ = rf.overlap_pair()
    e0 = rf.t_rmse(np.eye(4), T)
    sigma = rf.numpy_icp(tgt, src, T, 20)
    trim = rf.numpy_icp(tgt, src, T, 20, trim=0.5)
    print(f"point: initial {e0:.3e}; 3 sigma {sigma[4]:.3e} / {sigma[19]:.3e}; trim 0.5 {trim[4]:.3e} / {trim[19]:.3e}")
    assert trim[19] < e0 < sigma[19] and sigma[19] >= 5 * trim[19]


@pytest.mark.parametrize("grid", [0.0, 1e-3])
def test_premises_point_to_plane(grid):
    """After 5 iterations on 12-neighbour normals: the trimmed rule at most 1e-3, the cull at
    least 1e-2; the same on the 1 mm grid of a LAS file after 20."""
    tgt, src, T, _ = rf.overlap_pair(grid=grid)
    iters = 20 if grid else 5
    sigma = rf.numpy_icp(tgt, src, T, iters, plane_k=12)
    trim = rf.numpy_icp(tgt, src, T, iters, trim=0.5, plane_k=12)
    print(f"plane, grid {grid}: 3 sigma {sigma[-1]:.3e}; trim 0.5 {trim[-1]:.3e}")
    assert trim[-1] <= 1e-3 and sigma[-1] >= 1e-2


def test_constructed_sets_fit_the_lattice():
    for name, r in rf.select_sets().items():
        assert len(r) == 4913 and np.isfinite(r).all() and (r > 0).all() and r.max() < 4.0, name  # half the lattice spacing
        assert len(rf.boundary_ranks(r)) >= 4, name
    assert len(np.unique(np.frexp(rf.select_sets()["binades"])[1])) == 41
