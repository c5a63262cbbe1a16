"""Shared inputs and references of the rejector tests (a helper module, not a conftest): the
partial-overlap fixture, a numpy ICP loop with the engine's rules (the CPU statement of what the GPU
tests assert), the constructed residual sets of the rank select, and the derived bounds of the pair
sums.

The partial-overlap fixture. surface(n, seed): (x, y) uniform in [0, 4]^2 from default_rng(seed),
z = 0.30 sin(1.7 x) cos(1.3 y) + 0.20 sin(2.9 y + 0.5) + 0.15 cos(2.3 x - 0.7 y) + N(0, 1e-3) drawn
from the same generator after the (x, y). The target is the rows of surface(n, 21) with x <= 2.8, the
world source w the rows of surface(n, 22) with x >= 1.2, the source (w - t) @ R with
plane_fixtures.pair's R and t. At n = 6000: 4178 target points, 4193 source points, 56.8 % of the
source inside the target's extent.

Bounds of icp_hip_pair_sums (check_pair_sums). The kernel sums as the iterate's cull does: plain sums
of values shifted by a valid pair of this iterate (the first one), a fixed tree over fixed parts, the
parts added in index order, then means = shift + sum / m and H = sum (a - s)(b - t)^T - m da db^T. Each
term is at most the valid set's spread, 2 Ra_k (Ra_k = max over the valid set of |a_ik - ca_k|), so
stats_reference's bounds for the iterate's record hold as they stand, with members = 1 and without the
displacement term (the shift is a pair of this iterate, not of an earlier one):
  rmse       |drmse| <= (m + 8) 2^-53 rmse
  centroid   |dca_k| <= 2^-52 ((m + 4) 2 Ra_k + |ca_k|)
  H          |dH_kl| <= 8 (m + 8 + 4) 2^-52 m Ra_k Rb_l
"""
import functools
from fractions import Fraction

import numpy as np

import plane_fixtures as pf
import stats_reference as R

N_FIXTURE = 6000


def surface(n, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, 4.0, size=(n, 2))
    x, y = xy[:, 0], xy[:, 1]
    z = 0.30 * np.sin(1.7 * x) * np.cos(1.3 * y) + 0.20 * np.sin(2.9 * y + 0.5) + 0.15 * np.cos(2.3 * x - 0.7 * y)
    z = z + rng.normal(0.0, 1e-3, n)
    return np.stack([x, y, z], axis=1)


@functools.lru_cache(maxsize=None)
def overlap_pair(n=N_FIXTURE, grid=0.0):
    """(target, source, T_true, overlap fraction of the source). grid > 0: both clouds rounded to
    that grid (a LAS file's). The arrays are shared: do not write to them."""
    T = pf.pair(3)[2]
    Rm, t = T[:3, :3], T[:3, 3]
    a = surface(n, 21)
    tgt = a[a[:, 0] <= 2.8]
    w = surface(n, 22)
    w = w[w[:, 0] >= 1.2]
    src = (w - t) @ Rm
    if grid > 0.0:
        tgt, src = np.round(tgt / grid) * grid, np.round(src / grid) * grid
    tgt, src = np.ascontiguousarray(tgt), np.ascontiguousarray(src)
    for arr in (tgt, src):
        arr.setflags(write=False)
    return tgt, src, T, float((w[:, 0] <= 2.8).mean())


def with_nan_rows(src):
    out = np.array(src)
    out[[5, len(out) // 2, len(out) - 1]] = np.nan
    return out


def t_rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


# ---- the numpy loop (engine rules, no early stop)

def _nearest(tgt):
    try:
        from scipy.spatial import cKDTree
        tree = cKDTree(tgt)
        return lambda q: tree.query(q)[1]
    except ImportError:
        return lambda q: pf.nn_brute(q, tgt)


def _best_fit(a, b):
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    Rm = Vt.T @ U.T
    if np.linalg.det(Rm) < 0:
        Vt[2] *= -1
        Rm = Vt.T @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, cb - Rm @ ca
    return T


def _normals(tgt, k):
    try:
        from scipy.spatial import cKDTree
        idx = cKDTree(tgt).query(tgt, k)[1]
    except ImportError:
        idx = pf.knn_brute(tgt, tgt, k)[0]
    out = np.empty_like(tgt)
    for i, nb in enumerate(idx):
        p = tgt[nb] - tgt[nb].mean(0)
        out[i] = np.linalg.svd(p, full_matrices=False)[2][2]
    return out


def _plane_step(a, b, nrm, origin):
    A, g = pf.plane_sums_numpy(a, b, nrm, origin)[:2]
    x = np.linalg.solve(A, -g)
    w, tp = x[:3], x[3:]
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Rm = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, origin + tp - Rm @ origin
    return T


def numpy_icp(tgt, src, T_true, iterations, trim=None, plane_k=0, sigma=3.0):
    """t_rmse of the cumulative transform after each iteration. trim None: the engine's cull
    (mean + max(sigma std, mean / 2) at iteration 0, mean + sigma std later); else keep the
    icp_trim_rank smallest residuals. plane_k > 0: the point-to-plane step on k-neighbour normals."""
    nearest = _nearest(tgt)
    nrm = _normals(tgt, plane_k) if plane_k else None
    cur, Tc, errs = np.array(src), np.eye(4), []
    for it in range(iterations):
        idx = nearest(cur)
        d = np.sqrt(((cur - tgt[idx]) ** 2).sum(1))
        if trim is None:
            mean, sd = d.mean(), d.std()
            thr = mean + (max(sigma * sd, 0.5 * mean) if it == 0 else sigma * sd)
        else:
            n = len(d)
            rank = max(min(3, n), min(n, int(trim * float(n))))
            thr = np.partition(d, rank - 1)[rank - 1]
        v = d <= thr
        a, b = cur[v], tgt[idx[v]]
        T = _plane_step(a, b, nrm[idx[v]], a.mean(0)) if plane_k else _best_fit(a, b)
        cur = cur @ T[:3, :3].T + T[:3, 3]
        Tc = T @ Tc
        errs.append(t_rmse(Tc, T_true))
    return errs


# ---- constructed residuals of the rank select (on stats_reference.lattice(17), 4913 points)

def select_sets():
    """name -> residuals (each below 4, half the lattice's spacing: the match is unambiguous)."""
    n = 4913
    i = np.arange(n)
    two = np.full(n, 0.75)
    two[n // 3:] = 1.25
    two[1234] = 0.125
    return {
        "low_bits": 0.5 + 2.0 ** -44 * (i % 4097),
        "binades": (1.0 + (i % 7) / 8.0) * 2.0 ** -(i % 41).astype(np.float64),
        "two_values_and_one": two,
    }


def boundary_ranks(d):
    """Ranks (1-based) on both sides of every boundary between runs of equal values of the sorted
    finite residuals, with 1 and n; at most 64 boundaries, evenly picked."""
    s = np.sort(d[np.isfinite(d)])
    n = len(s)
    cut = np.flatnonzero(s[1:] != s[:-1]) + 1  # s[cut - 1] != s[cut]: ranks cut and cut + 1
    if len(cut) > 64:
        cut = cut[np.linspace(0, len(cut) - 1, 64).astype(int)]
    ranks = {1, n}
    for c in cut:
        ranks.update((int(c), int(c) + 1))
    return sorted(r for r in ranks if 1 <= r <= n)


def select_ref(d, rank):
    """(value, n_finite, n_less, n_equal) by numpy.partition over the finite residuals."""
    f = d[np.isfinite(d)]
    v = np.partition(f, rank - 1)[rank - 1]
    return v, len(f), int((f < v).sum()), int((f == v).sum())


def check_select(got, d, rank, label=""):
    v, n_finite, n_less, n_equal = select_ref(d, rank)
    assert np.float64(got.value).tobytes() == np.float64(v).tobytes(), (label, rank, got.value, v)
    assert (got.rank, got.n_finite, got.n_less, got.n_equal) == (rank, n_finite, n_less, n_equal), (label, rank)


# ---- the pair sums against stats_reference.pairs_ref

def check_pair_sums(ps, d, a, b, threshold, ratios=None, label=""):
    """icp_pair_sums `ps` of the residuals d, moved source a and matches b at `threshold`."""
    d, a, b = np.asarray(d, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(d)
    v = fin & (d <= threshold)
    m = int(v.sum())
    assert ps.threshold == threshold or (np.isinf(threshold) and np.isinf(ps.threshold)), label
    assert ps.n_finite == int(fin.sum()) and ps.valid == m, (label, ps.valid, m)
    if m == 0:
        assert ps.rmse == 0.0 and ps.sum_d2 == 0.0 and not any(ps.centroid_src) and not any(ps.centroid_tgt) \
            and not any(ps.H), label
        return
    p = R.pairs_ref(d[v], a[v], b[v])
    fails = []

    def cmp(field, got, want, bound):
        err = abs(Fraction(float(got)) - want)
        r = 0.0 if err == 0 else (float("inf") if bound == 0 else float(err / bound))
        if ratios is not None:
            ratios[field] = max(ratios.get(field, 0.0), r)
        if r > 1.0:
            fails.append(f"{field}: got {float(got)!r}, reference {float(want)!r}, error {float(err):.3e} > bound "
                         f"{float(bound):.3e}")

    cmp("rmse", ps.rmse, p["rmse"], (m + 8) * R.E53 * p["rmse"])
    Ra = [max(abs(Fraction(float(x)) - p["ca"][k]) for x in (a[v][:, k].min(), a[v][:, k].max())) for k in range(3)]
    Rb = [max(abs(Fraction(float(x)) - p["cb"][k]) for x in (b[v][:, k].min(), b[v][:, k].max())) for k in range(3)]
    for k in range(3):
        cmp("centroid_src", ps.centroid_src[k], p["ca"][k], R.E52 * ((m + 4) * 2 * Ra[k] + abs(p["ca"][k])))
        cmp("centroid_tgt", ps.centroid_tgt[k], p["cb"][k], R.E52 * ((m + 4) * 2 * Rb[k] + abs(p["cb"][k])))
    for k in range(3):
        for l in range(3):
            cmp("H", ps.H[3 * k + l], p["H"][k][l], 8 * (m + 8 + 4) * R.E52 * m * Ra[k] * Rb[l])
    assert not fails, f"{label}: " + "; ".join(fails)
