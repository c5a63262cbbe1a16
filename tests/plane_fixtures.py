"""Shared fixture of the point-to-plane tests (a helper module, not a conftest): three orthogonal
planes sampled twice, the second sampling moved by a known rigid transform, and the numpy
references of the k-NN query and of the plane sums."""
import functools

import numpy as np


def corner(n, seed, noise=1e-3, L=4.0):      # three orthogonal L x L planes, m = n // 3 points each
    rng = np.random.default_rng(seed); out = []
    for ax in range(3):
        uv = rng.uniform(0, L, size=(n // 3, 2)); p = np.zeros((n // 3, 3))
        o = [a for a in range(3) if a != ax]
        p[:, o[0]], p[:, o[1]] = uv[:, 0], uv[:, 1]; p[:, ax] = rng.normal(0, noise, n // 3)
        out.append(p)
    return np.concatenate(out)


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    R = np.eye(3)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R[i, i], R[j, j] = c, c
    if axis == 1:
        R[i, j], R[j, i] = s, -s
    else:
        R[i, j], R[j, i] = -s, s
    return R


@functools.lru_cache(maxsize=None)
def pair(n):
    """(target, source, T_true): target corner(n, 11); source (w - t) @ R with w = corner(n, 12),
    R = Rz(2 deg) Ry(0.5 deg) Rx(-0.5 deg), t = (0.08, -0.05, 0.03); T_true = [R | t] maps the
    source onto the target's surfaces. The arrays are shared: do not write to them."""
    tgt = corner(n, 11)
    w = corner(n, 12)
    R = _rot(2, 2.0) @ _rot(1, 0.5) @ _rot(0, -0.5)
    t = np.array([0.08, -0.05, 0.03])
    src = (w - t) @ R  # rows R^T (w - t)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    for a in (tgt, src, T):
        a.setflags(write=False)
    return tgt, src, T


def d2_rows(q, tgt):
    """fl(d2) of every (query, target) pair with d2_to's arithmetic: dx*dx + dy*dy + dz*dz, left to
    right, each product and sum rounded once (numpy does not fuse)."""
    dx = tgt[None, :, 0] - q[:, None, 0]
    dy = tgt[None, :, 1] - q[:, None, 1]
    dz = tgt[None, :, 2] - q[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def knn_brute(q, tgt, k, chunk=256):
    """The k target points of each query smallest under (fl(d2), index), ascending."""
    q = np.ascontiguousarray(q, np.float64)
    idx = np.empty((len(q), k), np.int32)
    d2 = np.empty((len(q), k), np.float64)
    for lo in range(0, len(q), chunk):
        D = d2_rows(q[lo:lo + chunk], tgt)
        kth = np.partition(D, k - 1, axis=1)[:, k - 1]
        for r in range(D.shape[0]):
            cand = np.flatnonzero(D[r] <= kth[r])  # every point that can be among the k, ties included
            order = cand[np.lexsort((cand, D[r, cand]))][:k]
            idx[lo + r] = order
            d2[lo + r] = D[r, order]
    return idx, d2


def nn_brute(q, tgt, chunk=512):
    """Index of the nearest target point of each query (first minimum of fl(d2))."""
    out = np.empty(len(q), np.int64)
    for lo in range(0, len(q), chunk):
        out[lo:lo + chunk] = np.argmin(d2_rows(q[lo:lo + chunk], tgt), axis=1)
    return out


def plane_terms(a, b, nrm, origin):
    """Per pair: J (m, 6) = (a' x n, n) with a' = a - origin, and r (m,) = n.(a - b), in the
    kernel's operation order."""
    ap = a - origin
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    r = (nx * (a[:, 0] - b[:, 0]) + ny * (a[:, 1] - b[:, 1])) + nz * (a[:, 2] - b[:, 2])
    J = np.stack([ap[:, 1] * nz - ap[:, 2] * ny, ap[:, 2] * nx - ap[:, 0] * nz, ap[:, 0] * ny - ap[:, 1] * nx,
                  nx, ny, nz], axis=1)
    return J, r


def plane_sums_numpy(a, b, nrm, origin):
    """(A (6, 6), g (6,), sum_r2, and the sums of the terms' magnitudes absA, absg, absr2)."""
    J, r = plane_terms(a, b, nrm, origin)
    P = J[:, :, None] * J[:, None, :]
    G = J * r[:, None]
    return (P.sum(0), G.sum(0), float((r * r).sum()), np.abs(P).sum(0), np.abs(G).sum(0), float((r * r).sum()))


def sums_struct(icp, A, g, sum_r2, n, origin=(0.0, 0.0, 0.0), n_skipped=0):
    s = icp.PlaneSums()
    s.A[:] = list(np.asarray(A, np.float64).reshape(36))
    s.g[:] = list(np.asarray(g, np.float64).reshape(6))
    s.sum_r2 = float(sum_r2)
    s.n = int(n)
    s.n_skipped = int(n_skipped)
    s.origin[:] = list(origin)
    return s
