"""References and fixtures of the plane path's exact tests (a helper module, not a conftest):
the numpy model of k_target_normals operation for operation, a plane-sums case whose every term is
a small dyadic number (so every sum is exact in any order), and targets made of separated line and
strip clusters on both sides of the normals' rank rule. tests/test_plane_reference.py proves on the
CPU what the GPU tests rely on."""
import functools
from fractions import Fraction

import numpy as np

import plane_fixtures as pf
from stats_reference import GEO_OFFSET

FAR_OFFSET = np.array([-7.3e6, 2.1e6, -40.0])
OFFSETS = {"origin": np.zeros(3), "geo": GEO_OFFSET, "far": FAR_OFFSET}
RANK_MIN = 2.0 ** -26          # kNormalRankMin (knn_kernels.hip): zero unless S[1] > 2^-26 S[0]


def knn_tier(levels, k):
    """(bytes per thread, block threads) of knn_block_threads (knn_kernels.hip)."""
    per = 8 * levels + 12 * k
    return per, 256 if per * 256 <= 65536 else 128 if per * 128 <= 65536 else 64


def normals_model(tgt, idx, view, icp, with_s=False):
    """k_target_normals in numpy: idx (n, k) the neighbours of every target point in list order
    (knn_brute's), view None or the viewpoint. Every product is rounded before its add (numpy does
    not fuse), the sums run in neighbour order, the eigenvector is the host compile of svd3_impl.h.
    Returns the normals (n, 3) float64, to be compared by bytes; with_s: also S (n, 3)."""
    tgt = np.ascontiguousarray(tgt, np.float64)
    n, k = idx.shape
    p = tgt[idx]                                            # (n, k, 3)
    s = np.zeros((n, 3))
    for r in range(k):
        s = s + p[:, r]
    m = s / float(k)
    c = np.zeros((6, n))
    for r in range(k):
        d = p[:, r] - m
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        for t, prod in enumerate((dx * dx, dx * dy, dx * dz, dy * dy, dy * dz, dz * dz)):
            c[t] = c[t] + prod
    out = np.zeros((n, 3))
    sv = np.zeros((n, 3))
    for j in range(n):
        c00, c01, c02, c11, c12, c22 = c[:, j]
        _, S, V = icp.jacobi_svd3([c00, c01, c02, c01, c11, c12, c02, c12, c22])
        sv[j] = S
        if not S[1] > RANK_MIN * S[0]:
            continue
        v = V[:, 2].copy()
        ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        v = v / ln
        if view is not None:
            q = tgt[j]
            flip = (v[0] * (view[0] - q[0]) + v[1] * (view[1] - q[1])) + v[2] * (view[2] - q[2]) < 0.0
        else:
            flip = v[np.argmax(np.abs(v))] < 0.0            # first maximum: the lowest axis on a tie
        if flip:
            v = -v
        if ln > 0.0:
            out[j] = v
    return (out, sv) if with_s else out


# --- the exact plane-sums case

@functools.lru_cache(maxsize=None)
def exact_plane_case(n_src, seed=1):
    """dict(tgt, nrm, src, j, origin): the shuffled 16^3 integer lattice, one caller-set normal
    +-e_x / +-e_y / +-e_z per point with 200 rows zero, each source row the lattice point tgt[j]
    plus an offset of multiples of 1/64 in [-1/4, 1/4] (every fifth row: no offset), origin
    (8, 8, 8). J, r and their products are multiples of 2^-12 below 2^8. Shared: read only."""
    rng = np.random.default_rng(1000 + seed)
    g = np.arange(16, dtype=np.float64)
    tgt = rng.permutation(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    nrm = np.zeros((4096, 3))
    nrm[np.arange(4096), rng.integers(0, 3, 4096)] = rng.choice([-1.0, 1.0], 4096)
    nrm[rng.choice(4096, 200, replace=False)] = 0.0
    j = rng.integers(0, 4096, n_src)
    off = rng.integers(-16, 17, size=(n_src, 3)) / 64.0
    off[::5] = 0.0
    src = tgt[j] + off
    out = {"tgt": tgt, "nrm": nrm, "src": src, "j": j, "origin": np.array([8.0, 8.0, 8.0])}
    for a in out.values():
        a.setflags(write=False)
    return out


def exact_sums(case, use):
    """(A, g, sum_r2, n, n_skipped) of the case's pairs selected by the mask `use`, as the kernel
    defines them; exact whatever the order (tests/test_plane_reference.py)."""
    nz = case["nrm"][case["j"]].any(1)
    take = use & nz
    a, b, nr = case["src"][take], case["tgt"][case["j"][take]], case["nrm"][case["j"][take]]
    A, g, r2, *_ = pf.plane_sums_numpy(a, b, nr, case["origin"])
    return A, g, r2, int(take.sum()), int((use & ~nz).sum())


# --- line and strip clusters

def _unit(v):
    return v / np.linalg.norm(v)


def _centres(n, spread, offset):
    """n cluster centres on a grid of 128 spreads (a power of two times the spread's own power of
    two where the cluster wants dyadic coordinates), moved by the offset."""
    step = 128.0 * 2.0 ** np.ceil(np.log2(spread))
    ijk = np.stack(np.unravel_index(np.arange(n), (4, 4, 4)), -1).astype(np.float64)
    return ijk * step + offset


@functools.lru_cache(maxsize=None)
def line_clusters(k, where, spread, seed=1):
    """(target (24 k, 3), kind (24,)): 24 clusters of k collinear points each, at most one spread
    long, centres at least 128 spreads apart, at OFFSETS[where]. kind 0: parallel to an axis;
    1: a dyadic oblique line (integer direction, steps of 2^-7 of the spread's power of two);
    2: a random direction with random steps, the coordinates rounded to fp64 as they come."""
    rng = np.random.default_rng(2000 + seed)
    cen = _centres(24, spread, OFFSETS[where])
    u = 2.0 ** np.floor(np.log2(spread)) / 64.0
    pts, kind = [], []
    for ci in range(24):
        kd = 0 if ci < 6 else 1 if ci < 12 else 2
        if kd == 0:
            d = np.eye(3)[ci % 3]
            t = (rng.permutation(np.arange(-16, 17))[:k] * 2.0 + rng.uniform(-0.5, 0.5, k)) * u
        elif kd == 1:
            d = np.array([(1, 1, 0), (1, -1, 1), (2, 1, -1), (0, 1, 2), (-1, 2, 0), (1, 1, 1)][ci - 6], np.float64)
            t = rng.permutation(np.arange(-16, 17))[:k] * (u / 2.0)
        else:
            d = _unit(rng.normal(size=3))
            t = (rng.permutation(np.arange(-16, 17))[:k] + rng.uniform(-0.3, 0.3, k)) * (spread / 34.0)
        pts.append(cen[ci] + t[:, None] * d)
        kind.append(kd)
    tgt = np.concatenate(pts)
    tgt.setflags(write=False)
    return tgt, np.array(kind)


@functools.lru_cache(maxsize=None)
def strip_clusters(k, where, spread, seed=1):
    """(target (24 k, 3), d1 (24, 3), d2 (24, 3)): 24 planar clusters of k points, oblique, one
    spread long along the unit vector d1 and 2^-8 of that wide along d2 (d1 . d2 = 0)."""
    rng = np.random.default_rng(3000 + seed)
    cen = _centres(24, spread, OFFSETS[where])
    pts, D1, D2 = [], [], []
    for ci in range(24):
        d1 = _unit(rng.normal(size=3))
        d2 = _unit(np.cross(d1, rng.normal(size=3)))
        t = (rng.permutation(np.arange(-16, 17))[:k] + rng.uniform(-0.3, 0.3, k)) * (spread / 34.0)
        # the lateral offsets alternate along the strip, so three points already span its width
        w = np.where(np.argsort(np.argsort(t)) % 2 == 0, 1.0, -1.0) * rng.uniform(0.3, 0.5, k) * (spread / 256.0)
        pts.append(cen[ci] + t[:, None] * d1 + w[:, None] * d2)
        D1.append(d1)
        D2.append(d2)
    tgt = np.concatenate(pts)
    tgt.setflags(write=False)
    return tgt, np.array(D1), np.array(D2)


def exact_covariance(p):
    """The covariance sum (p_i - mean)(p_i - mean)^T of the rows of p in exact arithmetic, rounded
    once to fp64 (3, 3), and the sum of its terms' magnitudes (3, 3)."""
    F = [[Fraction(float(x)) for x in row] for row in p]
    k = len(F)
    m = [sum(row[a] for row in F) / k for a in range(3)]
    D = [[row[a] - m[a] for a in range(3)] for row in F]
    Cm = np.array([[float(sum(d[a] * d[b] for d in D)) for b in range(3)] for a in range(3)])
    Ab = np.array([[float(sum(abs(d[a] * d[b]) for d in D)) for b in range(3)] for a in range(3)])
    return Cm, Ab


def deep_copies(seed=7):
    """The target of test_copies_deeper_than_a_leaf: 4000 points, 40 of them copies of one, which
    no subdivision separates, so the tree is as deep as max_depth allows. (target, copy indices)."""
    rng = np.random.default_rng(seed)
    tgt = rng.normal(size=(4000, 3))
    where = rng.choice(4000, 40, replace=False)
    tgt[where] = tgt[where[0]]
    return tgt, where


def tie_plane():
    """Eight dyadic points on the plane x = y, a target of exactly k = 8 points: every sum of the
    normals' arithmetic is exact, the normal is (1, -1, 0) / sqrt(2) up to its sign, and the two
    components of largest magnitude tie. With a viewpoint on the plane n . (v - p) is exactly zero."""
    a = np.arange(8) / 4.0
    b = np.array([0.0, 1.0, 0.5, 0.25, 1.5, 0.0, 0.75, 1.0])
    return np.stack([a, a, b], 1), np.array([5.0, 5.0, 3.0])
