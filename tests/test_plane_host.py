"""The host side of point-to-plane ICP (no GPU): icp_plane_solve against numpy on the sums of the
corner fixture, the sanitizer build of plane_solve.h, and the device calls' refusal without a GPU."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import plane_fixtures as pf

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "iterativeclosestpoint_amd" / "csrc"
EXE = ROOT / "build" / "sanitize" / "plane_solve_asan"
N = 6000


@pytest.fixture(scope="module")
def pairs():
    """Every source point of the 6000-point pair with its brute-force nearest target point and that
    point's plane normal (the fixture's planes are the coordinate planes)."""
    tgt, src, T_true = pf.pair(N)
    j = pf.nn_brute(src, tgt)
    nrm = np.zeros((N, 3))
    nrm[np.arange(N), j // (N // 3)] = 1.0
    return src, tgt[j], nrm


def _sums(icp, pairs, origin):
    a, b, nrm = pairs
    A, g, r2, *_ = pf.plane_sums_numpy(a, b, nrm, np.asarray(origin, np.float64))
    return pf.sums_struct(icp, A, g, r2, len(a), origin), A, g


def _x_of(T, c):
    """(w, t') of a step T about the origin c: the rotation's log and T's translation undone."""
    R = T[:3, :3]
    vee = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])  # (sin t / t) w
    s = np.linalg.norm(vee)
    w = vee * (np.arcsin(s) / s) if s > 0 else vee
    return np.concatenate([w, T[:3, 3] - c + R @ c])


def test_solve_matches_numpy(icp, pairs):
    c = pairs[0].mean(0)
    s, A, g = _sums(icp, pairs, c)
    T, ok = icp.plane_solve(s)
    assert ok == 1
    want = np.linalg.solve(A, -g)
    got = _x_of(T, c)
    cond = np.linalg.cond(A)
    for part in (slice(0, 3), slice(3, 6)):  # radians and metres apart
        err = np.linalg.norm(got[part] - want[part]) / np.linalg.norm(want[part])
        assert err <= 1e-10, f"relative error {err:.3e}, cond(A) = {cond:.3e}"


def test_rotation_is_orthonormal(icp, pairs):
    s, _, _ = _sums(icp, pairs, pairs[0].mean(0))
    T, ok = icp.plane_solve(s)
    assert ok == 1
    R = T[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14
    assert abs(np.linalg.det(R) - 1.0) <= 1e-14
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])


def _origin_gap(icp, pairs):
    """Largest distance between the images of the pairs' source points under the step solved about
    their centroid c and the step solved about 0, with |c| and the step's angle."""
    a = pairs[0]
    c = a.mean(0)
    Tc, okc = icp.plane_solve(_sums(icp, pairs, c)[0])
    T0, ok0 = icp.plane_solve(_sums(icp, pairs, (0.0, 0.0, 0.0))[0])
    assert okc == 1 and ok0 == 1
    pc = a @ Tc[:3, :3].T + Tc[:3, 3]
    p0 = a @ T0[:3, :3].T + T0[:3, 3]
    xc, x0 = _x_of(Tc, c), _x_of(T0, np.zeros(3))
    lin = np.abs((np.cross(xc[:3], a - c) + xc[3:]) - (np.cross(x0[:3], a) + x0[3:])).max()
    return lin, np.abs(pc - p0).max(), np.linalg.norm(c), np.linalg.norm(xc[:3])


def test_origin_does_not_change_the_map(icp, pairs):
    """The normal equations about c and about 0 describe one least-squares problem: their solutions
    move every point by the same w x (a - c) + t'_c = w x a + t'_0, held to 1e-9 on the fixture's
    points (the figure tests/test_gpu_scene.py uses for transforms). The rigid maps built from them,
    R (x - c) + c + t'_c and R x + t'_0, then differ by (R - I - [w]x) c, at most |c| theta^2 / 2:
    1e-3 on the unaligned pair (theta = 0.035, |c| = 2.6), 7e-9 with the source placed by T_true
    (theta = 8e-5); both are held to that bound plus the 1e-9."""
    tgt, src, T_true = pf.pair(N)
    w = src @ T_true[:3, :3].T + T_true[:3, 3]
    j = pf.nn_brute(w, tgt)
    nrm = np.zeros((N, 3))
    nrm[np.arange(N), j // (N // 3)] = 1.0
    for case in (pairs, (w, tgt[j], nrm)):
        lin, gap, cn, theta = _origin_gap(icp, case)
        assert lin <= 1e-9, (lin, cn, theta)
        assert gap <= cn * theta ** 2 / 2 + 1e-9, (gap, cn, theta)


def test_singular_input_is_refused(icp, pairs):
    a, b, _ = pairs
    nrm = np.zeros_like(a)
    nrm[:, 2] = 1.0  # J = (a'y, -a'x, 0, 0, 0, 1): three columns exactly zero
    A, g, r2, *_ = pf.plane_sums_numpy(a, b, nrm, np.zeros(3))
    assert np.count_nonzero(np.diag(A)) == 3
    T, ok = icp.plane_solve(pf.sums_struct(icp, A, g, r2, len(a)))
    assert ok == 0
    assert np.isnan(T).all()  # untouched


def test_too_few_pairs_is_refused(icp, pairs):
    five = tuple(p[:5] for p in pairs)
    s, _, _ = _sums(icp, five, (0.0, 0.0, 0.0))
    assert s.n == 5
    T, ok = icp.plane_solve(s)
    assert ok == 0 and np.isnan(T).all()
    # the same matrix with a pair count of 6 is judged on its pivots, not on the count
    s.n = 6
    assert icp.plane_solve(s)[1] == 0  # five pairs: rank <= 5


def test_solver_under_sanitizer(icp, pairs, tmp_path):
    r = subprocess.run(["make", "-C", str(CSRC), "plane_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a, b, _ = pairs
    flat = np.zeros_like(a)
    flat[:, 2] = 1.0
    As, gs, r2s, *_ = pf.plane_sums_numpy(a, b, flat, np.zeros(3))
    cases = [(_sums(icp, pairs, a.mean(0))[0], 1), (_sums(icp, pairs, (0.0, 0.0, 0.0))[0], 1),
             (pf.sums_struct(icp, As, gs, r2s, len(a)), 0),
             (_sums(icp, tuple(p[:5] for p in pairs), (0.0, 0.0, 0.0))[0], 0)]
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for s, want in cases:
            f.write(bytes(s))
            f.write(np.int64(want).tobytes())
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    run = subprocess.run([str(EXE), str(path)], capture_output=True, text=True, timeout=300, env=env)
    report = run.stdout[-2000:] + run.stderr[-6000:]
    assert run.returncode == 0, report
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, report
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == len(cases) + 1, report
    assert all(line.endswith("fine") for line in lines[:-1]), report


def test_device_calls_fail_loudly_without_a_context(icp):
    """The k-NN, normals and plane-sums calls refuse with IcpError where there is no device context
    (without a GPU none can be made: no CPU fallback exists)."""
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(icp.IcpError):
            icp.Context(0)
    ctx = object.__new__(icp.Context)  # what a caller is left with: no handle
    ctx._h = C.c_void_p()
    ctx._n_tgt = 4
    ctx.n_src = 0
    q = np.zeros((4, 3))
    for call in (lambda: ctx.knn(q, 2), lambda: ctx.knn_device(0, 4, 2), lambda: ctx.estimate_target_normals(8),
                 lambda: ctx.set_target_normals(q), lambda: ctx.get_target_normals(), lambda: ctx.plane_sums()):
        with pytest.raises(icp.IcpError):
            call()
