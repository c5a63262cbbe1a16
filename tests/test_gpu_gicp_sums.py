"""The generalized-ICP sums on the GPU (gicp_kernels.hip, icp_hip_gicp_sums / _at): to the last bit
on gicp_reference.exact_gicp_case (every term a small dyadic number, every sum exact in any order)
at source sizes under a wave, over one 4096-query part and over two parts; against numpy with the
textbook summation bound on the corner fixture with estimated normals of both clouds, before and
after a move; the isotropic counts, the determinism, epsilon = 1, NaN source rows and the refusals."""
import ctypes as C

import numpy as np
import pytest

import gicp_reference as G
import plane_fixtures as pf
import reject_fixtures as rf

pytestmark = pytest.mark.gpu

N = 6000
K = 16
EPS = 1e-3


@pytest.fixture(scope="module")
def lattice(icp):
    """The lattice target of the exact case with its caller-set normals."""
    case = G.exact_gicp_case(63)
    with icp.Context(0) as c:
        c.set_target(case["tgt"])
        c.set_target_normals(case["nrm"])
        yield c


@pytest.fixture(scope="module")
def corner(icp):
    """A context holding the 6000-point target with its k = 16 normals."""
    with icp.Context(0) as c:
        c.set_target(pf.pair(N)[0])
        c.estimate_target_normals(K)
        yield c


def _equal(s, want, what):
    A, g, r2, n, iso_src, iso_tgt = want
    gotA = np.array(s.A[:]).reshape(6, 6)
    assert (s.n, s.n_iso_src, s.n_iso_tgt) == (n, iso_src, iso_tgt), what
    assert np.array_equal(gotA, gotA.T), what
    assert np.array_equal(gotA, A), (what, np.abs(gotA - A).max())
    assert np.array_equal(np.array(s.g[:]), g), what
    assert s.sum_r2 == r2, what


@pytest.mark.parametrize("n_src", [63, 4097, 6000])
def test_sums_are_exact(lattice, n_src):
    case = G.exact_gicp_case(n_src)
    o, Rm, eps = case["origin"], case["R"], case["epsilon"]
    lattice.set_source(case["src"])
    lattice.set_source_normals(case["n0"])
    st = lattice.iterate()
    idx, d = lattice.get_correspondences()
    assert np.array_equal(idx, case["j"])  # the nearest lattice point is unique
    valid = d <= st.threshold
    assert valid.sum() == st.valid and valid.sum() >= 0.5 * n_src
    s = lattice.gicp_sums(o, Rm, eps)
    _equal(s, G.exact_sums(case, valid), "the iterate's threshold")
    assert list(s.origin) == list(o) and s.epsilon == eps and s.n == st.valid
    assert s.n_iso_src == s.n_iso_tgt  # the case's zero normals come in pairs
    assert bytes(lattice.gicp_sums(o, Rm, eps)) == bytes(s)
    at = lattice.gicp_sums_at(o, Rm, eps, np.inf)
    _equal(at, G.exact_sums(case, np.ones(n_src, bool)), "every finite pair")
    assert at.n == n_src
    assert bytes(lattice.gicp_sums_at(o, Rm, eps, st.threshold)) == bytes(s)
    at0 = lattice.gicp_sums_at(o, Rm, eps, 0.0)
    _equal(at0, G.exact_sums(case, d == 0.0), "threshold 0")
    assert at0.n >= (n_src + 4) // 5  # every fifth row has no offset


def test_epsilon_one_is_the_point_metric(icp, lattice):
    """C = I for every point: M = I / 2, the translation block is n / 2 I exactly, and the solve is
    the small-angle form of the SVD best fit of the same pairs."""
    case = G.exact_gicp_case(4097)
    lattice.set_source(case["src"])
    lattice.set_source_normals(case["n0"])
    st = lattice.iterate()
    o = np.array(st.centroid_src[:])
    s = lattice.gicp_sums(o, case["R"], 1.0)
    A = np.array(s.A[:]).reshape(6, 6)
    assert s.n == st.valid and np.array_equal(A[3:, 3:], s.n / 2.0 * np.eye(3))
    T, ok = icp.gicp_solve(s)
    assert ok == 1
    Ts = icp.best_fit_from_stats(st)
    # Both minimise sum |R a + t - b|^2 over the same pairs; the solve is one Gauss-Newton step from
    # the identity. With H the step's matrix (the rotation block of sum J^T J = 2 A; about the pairs'
    # centroid the coupling with the translation vanishes) the exact Hessian differs from it by the
    # residuals' term, at most 2 sum |r_i| |a'_i|, and by a relative O(angle): |dw| <= angle (kappa +
    # 4 angle), kappa = 2 sum |r| |a'| / lambda_min(H). The translations of the two transforms then
    # differ by (R - R') c for the centroid c: at most 2 |c| |dw|.
    idx, d = lattice.get_correspondences()
    v = d <= st.threshold
    r, pa = case["src"][v] - case["tgt"][idx[v]], case["src"][v] - o
    kappa = 2.0 * (np.linalg.norm(r, axis=1) * np.linalg.norm(pa, axis=1)).sum() / np.linalg.eigvalsh(2.0 * A[:3, :3]).min()
    vee = lambda Rm: 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    angle = np.linalg.norm(vee(Ts[:3, :3]))
    bound = angle * (kappa + 4.0 * angle)
    dw, dt = np.abs(vee(T[:3, :3]) - vee(Ts[:3, :3])).max(), np.abs(T[:3, 3] - Ts[:3, 3]).max()
    print(f"epsilon = 1: angle {angle:.3e}, kappa {kappa:.3e}, |dw| {dw:.3e} (bound {bound:.3e}), |dt| {dt:.3e}")
    assert 1e-5 < angle < 1e-2 and kappa < 0.2
    assert dw <= bound and dt <= 2.0 * np.linalg.norm(o) * bound


def _numpy_sums(ctx, thr, R_src, origin, nrm_src, nrm_tgt=None):
    """The sums recomputed from what the context reports."""
    tgt = pf.pair(N)[0]
    src = ctx.get_source()
    idx, d = ctx.get_correspondences()
    nrm_tgt = ctx.get_target_normals() if nrm_tgt is None else nrm_tgt
    use = np.isfinite(d) & (d <= thr)
    n0, nb = nrm_src[use], nrm_tgt[idx[use]]
    want = G.gicp_sums_numpy(src[use], tgt[idx[use]], n0, nb, R_src, EPS, origin)
    return want + (int(use.sum()), int((~n0.any(1)).sum()), int((~nb.any(1)).sum()))


def _check_sums(s, want):
    A, g, r2, absA, absg, absr2, n, iso_src, iso_tgt = want
    assert (s.n, s.n_iso_src, s.n_iso_tgt) == (n, iso_src, iso_tgt)
    # any summation order of n terms on the model's own terms: (n + 8) 2^-52 sum |terms|
    f = (n + 8) * 2.0 ** -52
    gotA = np.array(s.A[:]).reshape(6, 6)
    assert np.array_equal(gotA, gotA.T)
    assert (np.abs(gotA - A) <= f * absA).all(), np.abs(gotA - A).max()
    assert (np.abs(np.array(s.g[:]) - g) <= f * absg).all()
    assert abs(s.sum_r2 - r2) <= f * absr2


def test_sums_match_numpy_before_and_after_a_move(icp, corner):
    src = pf.pair(N)[1]
    corner.set_source(src)
    corner.estimate_source_normals(K)
    n0 = corner.get_source_normals()
    assert np.abs(np.einsum("ni,ni->n", n0, n0) - 1.0).max() <= 2.0 ** -50
    st = corner.iterate()
    o = np.array(st.centroid_src[:])
    s = corner.gicp_sums(o, None, EPS)
    _check_sums(s, _numpy_sums(corner, st.threshold, np.eye(3), o, n0))
    assert s.n == st.valid >= 0.9 * N and s.n_iso_src == 0 and s.n_iso_tgt == 0
    # one applied non-trivial transform: the normals stay in the frame they were made in
    T, ok = icp.gicp_solve(s)
    assert ok == 1 and np.abs(T[:3, :3] - np.eye(3)).max() > 1e-3
    st = corner.iterate(T, 1)
    o = np.array(st.centroid_src[:])
    assert corner.get_source_normals().tobytes() == n0.tobytes()
    s = corner.gicp_sums(o, T[:3, :3], EPS)
    _check_sums(s, _numpy_sums(corner, st.threshold, T[:3, :3], o, n0))
    assert s.n == st.valid
    at = corner.gicp_sums_at(o, T[:3, :3], EPS, 0.01)
    want = _numpy_sums(corner, 0.01, T[:3, :3], o, n0)
    _check_sums(at, want)
    assert 0 < at.n < st.valid


def test_isotropic_counts(corner):
    tgt, src, _ = pf.pair(N)
    rng = np.random.default_rng(3)
    nb = corner.get_target_normals()
    holes_t = nb.copy()
    holes_t[rng.choice(N, 100, replace=False)] = 0.0
    try:
        corner.set_target_normals(holes_t)
        corner.set_source(src)
        corner.estimate_source_normals(K)
        holes_s = corner.get_source_normals()
        zeroed = rng.choice(N, 100, replace=False)
        holes_s[zeroed] = 0.0
        corner.set_source_normals(holes_s)
        st = corner.iterate()
        o = np.array(st.centroid_src[:])
        s = corner.gicp_sums(o, None, EPS)
        want = _numpy_sums(corner, st.threshold, np.eye(3), o, holes_s, holes_t)
        _check_sums(s, want)
        _, d = corner.get_correspondences()
        assert s.n == st.valid  # no pair is left out for a zero normal
        assert s.n_iso_src == int((d[zeroed] <= st.threshold).sum()) > 50 and s.n_iso_tgt > 50
    finally:
        corner.set_target_normals(nb)


def test_sums_are_deterministic(icp, corner):
    tgt, src, _ = pf.pair(N)
    Rm = pf._rot(2, 1.0)
    corner.set_source(src)
    corner.estimate_source_normals(K)
    st = corner.iterate()
    first = bytes(corner.gicp_sums(st.centroid_src, Rm, EPS))
    assert bytes(corner.gicp_sums(st.centroid_src, Rm, EPS)) == first
    for cfg in ({"candidate_cache": 0}, {"scan_groups": 1}):
        with icp.Context(0, cfg=cfg) as other:
            other.set_target(tgt)
            other.estimate_target_normals(K)
            other.set_source(src)
            other.estimate_source_normals(K)
            st2 = other.iterate()
            assert list(st2.centroid_src) == list(st.centroid_src)
            assert bytes(other.gicp_sums(st2.centroid_src, Rm, EPS)) == first, cfg


def test_nan_source_rows_change_no_sum(lattice):
    case = G.exact_gicp_case(4097)
    o, Rm, eps = case["origin"], case["R"], case["epsilon"]
    src = rf.with_nan_rows(case["src"])
    keep = np.isfinite(src).all(1)
    assert (~keep).sum() == 3
    lattice.set_source(src)
    lattice.set_source_normals(case["n0"])
    st = lattice.iterate()
    idx, d = lattice.get_correspondences()
    assert np.isnan(d[~keep]).all() and np.array_equal(idx[keep], case["j"][keep])
    valid = d <= st.threshold
    assert valid.sum() == st.valid and not valid[~keep].any()
    _equal(lattice.gicp_sums(o, Rm, eps), G.exact_sums(case, valid), "the iterate's threshold")
    with_nan = {thr: lattice.gicp_sums_at(o, Rm, eps, thr) for thr in (np.inf, 0.25)}
    for thr, s in with_nan.items():
        _equal(s, G.exact_sums(case, keep & (d <= thr)), f"threshold {thr}")
        assert s.n == (keep & (d <= thr)).sum() > 2000
    lattice.set_source(case["src"][keep])
    lattice.set_source_normals(case["n0"][keep])
    lattice.iterate()
    for thr, s in with_nan.items():
        assert bytes(lattice.gicp_sums_at(o, Rm, eps, thr)) == bytes(s)


def test_refusals(icp):
    tgt, src, _ = pf.pair(N)
    eye = np.eye(3)
    with icp.Context(0) as c:
        def code(call):
            with pytest.raises(icp.IcpError) as e:
                call()
            return e.value.code

        assert code(lambda: c.gicp_sums()) == icp.ENOTREADY  # no target
        c.set_target(tgt)
        c.set_source(src[:500])
        assert code(lambda: c.gicp_sums()) == icp.ENOTREADY  # no target normals
        c.estimate_target_normals(K)
        assert code(lambda: c.gicp_sums()) == icp.ENOTREADY  # no source normals
        c.estimate_source_normals(K)
        assert code(lambda: c.gicp_sums()) == icp.ENOTREADY  # no iterate
        c.iterate()
        ok = c.gicp_sums((0.0, 0.0, 0.0), eye, EPS)
        assert ok.n > 0
        skew = eye.copy()
        skew[0, 1] = 1e-8
        nan_R = eye.copy()
        nan_R[2, 2] = np.nan
        for call in (lambda: c.gicp_sums((np.nan, 0.0, 0.0), eye, EPS), lambda: c.gicp_sums((0.0, np.inf, 0.0), eye, EPS),
                     lambda: c.gicp_sums((0, 0, 0), skew, EPS), lambda: c.gicp_sums((0, 0, 0), 2.0 * eye, EPS),
                     lambda: c.gicp_sums((0, 0, 0), nan_R, EPS), lambda: c.gicp_sums((0, 0, 0), eye, 2.0 ** -21),
                     lambda: c.gicp_sums((0, 0, 0), eye, 1.0 + 2.0 ** -52), lambda: c.gicp_sums((0, 0, 0), eye, np.nan),
                     lambda: c.gicp_sums_at((0, 0, 0), eye, EPS, np.nan)):
            assert code(call) == icp.EINVAL
        for eps in (2.0 ** -20, 1.0):
            assert c.gicp_sums((0, 0, 0), eye, eps).epsilon == eps
        null = icp.lib().icp_hip_gicp_sums(c._h, None, eye.ctypes.data_as(C.c_void_p), EPS, C.byref(icp.GicpSums()))
        assert null == icp.EINVAL
        c.set_source(src[:500])  # a new source: its normals and its iterate are gone
        assert code(lambda: c.gicp_sums()) == icp.ENOTREADY
        for bad in (2.0 ** -21, 2.0, np.nan):
            assert code(lambda: c.set_gicp_epsilon(bad)) == icp.EINVAL
        c.set_gicp_epsilon(0.5)
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as g:
        g.set_target(tgt)
        g.estimate_target_normals(K)
        g.set_source(src)
        g.iterate()
        with pytest.raises(icp.IcpError) as e:
            g.gicp_sums()
        assert e.value.code == icp.EINVAL
