"""Every target normal, bit for bit (k_target_normals, knn_kernels.hip): svd3_impl.h gives the same
bits on the device and on the host, the neighbour lists are the brute-force (fl(d2), index) lists,
so get_target_normals() equals plane_reference.normals_model by bytes at every point, the badly
conditioned ones included. On top of the bytes, by value: collinear clusters get the zero normal
(the rank rule S[1] > 2^-26 S[0]), thin strips a unit normal perpendicular to the strip within the
first-order eigenvector bound, a tie of magnitudes goes to the lowest axis, and a viewpoint in the
plane does not flip."""
import numpy as np
import pytest

import plane_fixtures as pf
import plane_reference as R

pytestmark = pytest.mark.gpu

VIEW = np.array([2.0, 2.0, 2.0])
U = 2.0 ** -53


def _check(icp, ctx, tgt, idx, k, view, what=""):
    ctx.estimate_target_normals(k, view)
    got = ctx.get_target_normals()
    want = R.normals_model(tgt, idx[:, :k], view, icp)
    differ = np.flatnonzero((got.view(np.int64) != want.view(np.int64)).any(1))
    assert len(differ) == 0, (f"{what}: {len(differ)} of {len(tgt)} normals differ, first at {differ[0]}: "
                              f"{got[differ[0]]!r} for {want[differ[0]]!r}")
    return got


@pytest.fixture(scope="module")
def corners(icp):
    """where -> (context, target, brute-force lists at k = 32): the 600-point corner at each offset."""
    made = {}
    try:
        for where, off in R.OFFSETS.items():
            tgt = pf.corner(600, 11) + off
            ctx = icp.Context(0)
            ctx.set_target(tgt)
            made[where] = (ctx, tgt, pf.knn_brute(tgt, tgt, 32)[0])
        yield made
    finally:
        for c, _, _ in made.values():
            c.close()


@pytest.mark.parametrize("view", [False, True], ids=["no_viewpoint", "viewpoint"])
@pytest.mark.parametrize("k", [3, 4, 8, 16, 31, 32])
@pytest.mark.parametrize("where", list(R.OFFSETS))
def test_corner(icp, corners, where, k, view):
    ctx, tgt, idx = corners[where]
    v = VIEW + R.OFFSETS[where] if view else None
    nrm = _check(icp, ctx, tgt, idx, k, v)
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 4 * U  # no degenerate neighbourhood here


@pytest.mark.parametrize("k", [3, 8, 32])
def test_target_of_exactly_k_points(icp, k):
    tgt = np.random.default_rng(40 + k).normal(size=(k, 3))
    idx = pf.knn_brute(tgt, tgt, k)[0]
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        _check(icp, ctx, tgt, idx, k, None)
        _check(icp, ctx, tgt, idx, k, VIEW)


def test_lattice_ties_and_repeated_eigenvalues(icp):
    g = np.arange(8, dtype=np.float64)
    tgt = np.random.default_rng(41).permutation(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    idx, d2 = pf.knn_brute(tgt, tgt, 8)
    assert (d2[:, 6] == d2[:, 7]).mean() > 0.5  # the 7th place ties with the 8th: the index decides
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        _check(icp, ctx, tgt, idx, 7, None)
        _check(icp, ctx, tgt, idx, 7, np.array([3.5, 3.5, 20.0]))


@pytest.mark.parametrize("depth", [20, 40, 60])
def test_deep_copies_in_the_64_thread_tier(icp, depth):
    tgt, where = R.deep_copies()
    idx = _deep_lists()
    with icp.Context(0) as ctx:
        ctx.set_target(tgt, max_depth=depth)
        levels = ctx.target_info()["stack_levels"]
        assert levels == depth and R.knn_tier(levels, 32)[1] == 64
        nrm = _check(icp, ctx, tgt, idx, 32, None, f"depth {depth}")
    # the 32 copies of lowest index are the neighbourhood of every copy: one point, no plane
    assert (nrm[where] == 0.0).all()


_DEEP = []


def _deep_lists():
    if not _DEEP:
        tgt, _ = R.deep_copies()
        _DEEP.append(pf.knn_brute(tgt, tgt, 32)[0])
    return _DEEP[0]


CLUSTERS = [(k, w, s) for k in (3, 8, 32) for w in R.OFFSETS for s in (1.0, 0.01)]
CLUSTER_IDS = [f"k{k}-{w}-{s}" for k, w, s in CLUSTERS]


@pytest.mark.parametrize("k,where,spread", CLUSTERS, ids=CLUSTER_IDS)
def test_line_clusters_get_the_zero_normal(icp, k, where, spread):
    tgt, _ = R.line_clusters(k, where, spread)
    idx = pf.knn_brute(tgt, tgt, k)[0]
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        for view in (None, tgt.mean(0) + 3.0 * spread):
            nrm = _check(icp, ctx, tgt, idx, k, view)
            bad = np.flatnonzero(nrm.any(1))
            assert len(bad) == 0, f"{len(bad)} of {len(tgt)} collinear neighbourhoods got a normal, e.g. {nrm[bad[0]]}"


def _strip_bound(p):
    """(v1, v2, bound): the in-plane eigenvectors of the cluster's exact covariance C and the bound
    on |n . v| for the kernel's normal n. The kernel's matrix differs from C by
      k |e|^2                    the moments are taken about m = mean + e, which adds k e e^T exactly;
                                 |e_a| <= k u max|p_a| (k - 1 adds of partial sums below k max|p_a|,
                                 one division), u = 2^-53
      (k + 2) u 2 (tr C + k |e|^2)  each term's three roundings and the k - 1 adds, on the sum of the
                                 terms' magnitudes about m (Cauchy-Schwarz, in the Frobenius norm)
      160 u tr C                 the Jacobi's stop at off-diagonals of 2 eps max|diag| (sqrt(6) 2^-51),
                                 its rotations' roundings (18 rotations of a few u each), the
                                 reference's own rounding of C and eigh's backward error.
    First-order (Davis-Kahan, with |dC| <= gap / 2): sin(angle) <= 2 |dC| / (lambda1 - lambda2), plus
    4 u for the division by the length."""
    k = len(p)
    Cm, _ = R.exact_covariance(p)
    w, v = np.linalg.eigh(Cm)
    tr = float(np.trace(Cm))
    e2 = float(((k * U * np.abs(p).max(0)) ** 2).sum())
    dC = k * e2 + (k + 2) * U * 2.0 * (tr + k * e2) + 160.0 * U * tr
    gap = w[1] - w[0]
    assert dC <= gap / 2, (dC, gap)
    return v[:, 1], v[:, 2], 2.0 * dC / gap + 4 * U


@pytest.mark.parametrize("k,where,spread", CLUSTERS, ids=CLUSTER_IDS)
def test_strip_clusters_get_their_plane(icp, k, where, spread):
    tgt, d1, d2 = R.strip_clusters(k, where, spread)
    idx = pf.knn_brute(tgt, tgt, k)[0]
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        nrm = _check(icp, ctx, tgt, idx, k, None)
    assert np.abs(np.einsum("ni,ni->n", nrm, nrm) - 1.0).max() <= 8 * U
    worst = 0.0
    for c in range(24):
        v1, v2, bound = _strip_bound(tgt[c * k:(c + 1) * k])
        n = nrm[c * k:(c + 1) * k]
        worst = max(worst, np.abs(n @ v1).max() / bound, np.abs(n @ v2).max() / bound)
        assert np.abs(n @ v1).max() <= bound and np.abs(n @ v2).max() <= bound, (c, bound)
        assert (n[np.arange(k), np.abs(n).argmax(1)] > 0).all()
    print(f"strips k={k} {where} {spread}: worst |n . v| / bound = {worst:.3g}")


def test_tie_goes_to_the_lowest_axis_and_a_zero_dot_product_does_not_flip(icp):
    tgt, view = R.tie_plane()
    idx = pf.knn_brute(tgt, tgt, 8)[0]
    d = tgt - tgt.mean(0)                   # dyadic: exact, as every sum of the kernel's here
    _, S, V = icp.jacobi_svd3(d.T @ d)
    raw = V[:, 2] / np.sqrt((V[0, 2] * V[0, 2] + V[1, 2] * V[1, 2]) + V[2, 2] * V[2, 2])
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        nrm = _check(icp, ctx, tgt, idx, 8, None)
        assert (np.abs(nrm[:, 0]) == np.abs(nrm[:, 1])).all() and (nrm[:, 2] == 0.0).all()
        assert (nrm[:, 0] > 0.0).all() and (nrm[:, 1] < 0.0).all()
        seen = _check(icp, ctx, tgt, idx, 8, view)
        assert (seen == raw).all()          # the Jacobi's own sign: n . (v - p) is exactly zero
