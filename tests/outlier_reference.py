"""The numpy statement of the outlier filters' definition (include/icp_hip.h), the
bounds of the device's statistics and the fixture cloud of the outlier tests (a helper module, not
a conftest; validated on the CPU by tests/test_outlier_reference.py).

Statistical (k, std_ratio): the neighbours of point i are the k points j != i smallest under
(fl(d2_ij), j); score_i = (sqrt(d2_0) + ... + sqrt(d2_{k-1})) / k added in neighbour order;
mean and var of the scores (population form) from stats_reference.moments_ref;
threshold = mean + std_ratio * sqrt(var); kept iff score_i <= threshold.
Radius (k = minimum neighbours, radius): r2 = fl(radius * radius),
score_i = min(k, #{j != i : fl(d2_ij) <= r2}); kept iff score_i == k.

Bounds of the device's mean and std (u = 2^-53; W = max score - min score). The device sums
d_i = fl(score_i - c), c = score_0, and fl(d_i^2) over a fixed tree (|d_i| <= W (1 + u)), then
mean = fl(c + fl(S1 / n)), var = fl(fl(S2 / n) - fl(m1 m1)), std = fl(sqrt(var)). Any summation
order of n terms errs by at most (n - 1) u times the sum of the magnitudes, so to first order
  |mean_gpu - mean| <= (n + 2) u W + u |mean|,
  |std_gpu^2 - var| <= (3n + 7) u W^2 + 2 u var,
and the tests assert the rounder statements of stats_reference.py that contain them:
  |dmean| <= 2^-52 ((n + 4) W + |mean|),   |std_gpu^2 - var| <= 2^-52 (2n + 16) W^2 + 2^-51 var
(W = 0 forces std == 0.0: every d_i is then zero). The radius mode's sums are sums of small
integers and exact.
"""
import functools
from fractions import Fraction

import numpy as np

import plane_fixtures as pf
import stats_reference as sr

STATISTICAL, RADIUS = 0, 1  # icp_hip.h ICP_OUTLIER_*


def neighbours(xyz, k):
    """(idx (n, k), d2 (n, k)): the k nearest other points of every point under (fl(d2), index):
    the k + 1 nearest with the row's own index dropped if present, else the last entry."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    idx1, d21 = pf.knn_brute(xyz, xyz, k + 1)
    idx, d2 = np.empty((n, k), np.int32), np.empty((n, k))
    for i in range(n):
        own = np.flatnonzero(idx1[i] == i)
        keep = np.ones(k + 1, bool)
        keep[own[0] if len(own) else k] = False
        idx[i], d2[i] = idx1[i][keep], d21[i][keep]
    return idx, d2


def knn_scores(xyz, k):
    _, d2 = neighbours(xyz, k)
    r = np.sqrt(d2)
    s = r[:, 0].copy()
    for j in range(1, k):  # neighbour order, one rounded addition each
        s = s + r[:, j]
    return s / k


def radius_scores(xyz, radius, k, chunk=256):
    xyz = np.ascontiguousarray(xyz, np.float64)
    r2 = np.float64(radius) * np.float64(radius)
    cnt = np.empty(len(xyz), np.int64)
    for lo in range(0, len(xyz), chunk):
        D = pf.d2_rows(xyz[lo:lo + chunk], xyz)
        inside = D <= r2
        inside[np.arange(D.shape[0]), lo + np.arange(D.shape[0])] = False  # the point itself, by index
        cnt[lo:lo + chunk] = inside.sum(1)
    return np.minimum(cnt, k).astype(np.float64)


def reference(xyz, mode, k, param):
    """dict: score (n,), mean, var, sd, thr (Fractions), threshold (float), kept (bool mask),
    gap (the smallest relative distance of a score from the threshold; statistical mode)."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    score = knn_scores(xyz, k) if mode == STATISTICAL else radius_scores(xyz, param, k)
    mean, var = sr.moments_ref(score)
    sd = sr._sqrt(var)
    if mode == STATISTICAL:
        thr = mean + Fraction(float(param)) * sd
        threshold = float(thr)
        kept = score <= threshold
        gap = float(np.abs(score - threshold).min() / abs(threshold)) if threshold != 0 else 0.0
    else:
        thr, threshold = Fraction(k), float(k)
        kept = score == threshold
        gap = 1.0 / k  # counts are integers
    return dict(score=score, mean=mean, var=var, sd=sd, thr=thr, threshold=threshold, kept=kept, gap=gap)


def stats_bounds(score):
    """(bound of the mean, bound of std^2) for the scores' device statistics (the module docstring)."""
    score = np.asarray(score, np.float64)
    n = len(score)
    mean, var = sr.moments_ref(score)
    W = Fraction(float(score.max())) - Fraction(float(score.min()))
    return sr.E52 * ((n + 4) * W + abs(mean)), sr.E52 * (2 * n + 16) * W * W + sr.E51 * var


def check_stats(st, ref, label=""):
    """The device's record st against the reference: n, mean and std within their bounds, the
    threshold the rule's own arithmetic on the reported mean and std."""
    score = ref["score"]
    assert st.n == len(score), label
    b_mean, b_var = stats_bounds(score)
    e_mean = abs(Fraction(float(st.mean)) - ref["mean"])
    e_var = abs(Fraction(float(st.std)) ** 2 - ref["var"])
    print(f"[outlier stats] {label}: mean error {float(e_mean):.3e} (bound {float(b_mean):.3e}), "
          f"var error {float(e_var):.3e} (bound {float(b_var):.3e})")
    assert e_mean <= b_mean, f"{label}: mean {st.mean!r}, error {float(e_mean):.3e} > {float(b_mean):.3e}"
    assert e_var <= b_var, f"{label}: std {st.std!r}, error {float(e_var):.3e} > {float(b_var):.3e}"
    if score.max() == score.min():
        assert st.std == 0.0, label


N_SURFACE, N_INJECTED = 6000, 150


@functools.lru_cache(maxsize=None)
def fixture_cloud():
    """(cloud (6150, 3), injected (6150,) bool): the corner fixture plus 150 uniform strays in
    [-0.5, 4.5]^3, the rows permuted. Shared: read only."""
    rng = np.random.default_rng(21)
    stray = rng.uniform(-0.5, 4.5, (N_INJECTED, 3))
    perm = rng.permutation(N_SURFACE + N_INJECTED)
    cloud = np.ascontiguousarray(np.concatenate([pf.corner(N_SURFACE, 11), stray])[perm])
    injected = perm >= N_SURFACE
    cloud.setflags(write=False)
    injected.setflags(write=False)
    return cloud, injected


@functools.lru_cache(maxsize=None)
def fixture_reference(mode, k, param):
    """reference() of the fixture cloud, computed once per case. Shared: read only."""
    ref = reference(fixture_cloud()[0], mode, k, param)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def lattice8():
    """The 8^3 integer lattice in a fixed shuffled order, and the mask of its 6^3 interior."""
    g = np.arange(8.0)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    p = np.ascontiguousarray(p[np.random.default_rng(7).permutation(len(p))])
    interior = ((p >= 1) & (p <= 6)).all(1)
    return p, interior
