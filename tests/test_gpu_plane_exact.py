"""The plane sums to the last bit (plane_kernels.hip, icp_hip_plane_sums / _at): on
plane_reference.exact_plane_case every term is a small dyadic number, so every sum is exact in any
order and one dropped or doubled pair among thousands changes the result; source sizes around a
wave, a 256-thread block, one 4096-query part and two parts. Then the degenerate sums (every normal
zero, fewer than six pairs, NaN source rows) with the session's fallback, and one georeferenced
step: the sums within the summation bound, the solve within the first-order perturbation bound of a
longdouble solve of the same pairs."""
import numpy as np
import pytest

import plane_fixtures as pf
import plane_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EXACT_N = [1, 2, 5, 6, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 8193]


@pytest.fixture(scope="module")
def ctx(icp):
    """The lattice target of the exact case with its caller-set normals."""
    case = R.exact_plane_case(1)
    with icp.Context(0) as c:
        c.set_target(case["tgt"])
        c.set_target_normals(case["nrm"])
        yield c


def _equal(s, want, what):
    A, g, r2, n, skipped = want
    gotA = np.array(s.A[:]).reshape(6, 6)
    assert (s.n, s.n_skipped) == (n, skipped), what
    assert np.array_equal(gotA, gotA.T), what
    assert np.array_equal(gotA, A), (what, np.abs(gotA - A).max())
    assert np.array_equal(np.array(s.g[:]), g), what
    assert s.sum_r2 == r2, what


@pytest.mark.parametrize("n_src", EXACT_N)
def test_sums_are_exact(ctx, n_src):
    case = R.exact_plane_case(n_src)
    o = case["origin"]
    ctx.set_source(case["src"])
    st = ctx.iterate()
    idx, d = ctx.get_correspondences()
    assert np.array_equal(idx, case["j"])  # the nearest lattice point is unique
    valid = d <= st.threshold
    assert valid.sum() == st.valid and valid.sum() >= 0.5 * n_src
    s = ctx.plane_sums(o)
    _equal(s, R.exact_sums(case, valid), "the iterate's threshold")
    assert list(s.origin) == list(o) and s.n + s.n_skipped == st.valid
    assert bytes(ctx.plane_sums(o)) == bytes(s)
    for thr in (np.inf, 0.25, 0.0):
        use = np.isfinite(d) & (d <= thr)
        at = ctx.plane_sums_at(o, thr)
        _equal(at, R.exact_sums(case, use), f"threshold {thr}")
        assert bytes(ctx.plane_sums_at(o, thr)) == bytes(at)
        if thr == 0.0:
            assert at.n + at.n_skipped == (d == 0.0).sum() >= (n_src + 4) // 5  # every fifth row has no offset
        if thr == np.inf:
            assert at.n + at.n_skipped == n_src


def _session(icp, c, metric, steps=3):
    p = icp.params_default(max_iterations=steps, flags=icp.FLAG_NO_EARLY_STOP)
    ses = c.session(p, metric=metric)
    recs, used, sums = [], [], []
    while not ses.done:
        rec = ses.step()
        recs.append(None if rec is None else bytes(rec))
        s, u = ses.last_plane()
        used.append(u)
        sums.append(s)
    rc, _ = ses.finish()
    ses.close()
    return rc, recs, used, sums


def test_every_matched_normal_zero(icp):
    case = R.exact_plane_case(257)
    with icp.Context(0) as c:
        c.set_target(case["tgt"])
        c.set_target_normals(np.zeros((4096, 3)))
        c.set_source(case["src"])
        st = c.iterate()
        for s in (c.plane_sums(case["origin"]), c.plane_sums_at(case["origin"], st.threshold)):
            assert s.n == 0 and s.n_skipped == st.valid and st.valid > 200
            assert not np.array(s.A[:]).any() and not np.array(s.g[:]).any() and s.sum_r2 == 0.0
            T, ok = icp.plane_solve(s)
            assert ok == 0 and np.isnan(T).all()
        c.set_source(case["src"])
        rc, recs, used, sums = _session(icp, c, icp.METRIC_PLANE)
        assert len(recs) >= 1 and recs[0] is not None and used == [0] * len(recs)
        assert all(s.n == 0 for s in sums) and sums[0].n_skipped == st.valid
        c.set_source(case["src"])
        assert (rc, recs) == _session(icp, c, icp.METRIC_POINT)[:2]


@pytest.mark.parametrize("n_src", [3, 5])
def test_fewer_than_six_pairs(icp, ctx, n_src):
    case = R.exact_plane_case(n_src)
    ctx.set_source(case["src"])
    st = ctx.iterate()
    s = ctx.plane_sums_at(case["origin"], np.inf)
    assert s.n + s.n_skipped == n_src and st.valid >= 3
    T, ok = icp.plane_solve(s)
    assert ok == 0 and np.isnan(T).all()
    ctx.set_source(case["src"])
    rc, recs, used, sums = _session(icp, ctx, icp.METRIC_PLANE)
    assert len(recs) >= 1 and recs[0] is not None and used == [0] * len(recs)  # the SVD step, every time
    assert all(s.n < 6 for s in sums) and sums[0].n + sums[0].n_skipped == st.valid
    ctx.set_source(case["src"])
    assert (rc, recs) == _session(icp, ctx, icp.METRIC_POINT)[:2]


def test_nan_source_rows_change_no_sum(ctx):
    case = R.exact_plane_case(257)
    o = case["origin"]
    rows = np.array([3, 100, 256])
    src = case["src"].copy()
    src[rows[0], 0] = src[rows[1], 1] = np.nan
    src[rows[2]] = np.nan
    keep = np.ones(257, bool)
    keep[rows] = False
    ctx.set_source(src)
    st = ctx.iterate()
    idx, d = ctx.get_correspondences()
    assert np.isnan(d[rows]).all() and np.array_equal(idx[keep], case["j"][keep])
    # the iterate's own threshold: the pairs the context reports valid (none when the mean is NaN)
    valid = d <= st.threshold
    assert valid.sum() == st.valid and not valid[rows].any()
    _equal(ctx.plane_sums(o), R.exact_sums(case, valid), "the iterate's threshold")
    with_nan = {thr: ctx.plane_sums_at(o, thr) for thr in (np.inf, 0.25)}
    for thr, s in with_nan.items():
        _equal(s, R.exact_sums(case, keep & (d <= thr)), f"threshold {thr}")
        assert s.n + s.n_skipped == (keep & (d <= thr)).sum() > 100
    ctx.set_source(case["src"][keep])
    ctx.iterate()
    for thr, s in with_nan.items():
        t = ctx.plane_sums_at(o, thr)
        assert (bytes(t.A), bytes(t.g), t.sum_r2, t.n, t.n_skipped) == (bytes(s.A), bytes(s.g), s.sum_r2, s.n, s.n_skipped)


# --- one georeferenced step

def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in np.longdouble."""
    A, b = A.astype(np.longdouble).copy(), b.astype(np.longdouble).copy()
    n = len(b)
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        A[[j, p]], b[[j, p]] = A[[p, j]], b[[p, j]]
        for i in range(j + 1, n):
            f = A[i, j] / A[j, j]
            A[i, j:] -= f * A[j, j:]
            b[i] -= f * b[j]
    x = np.zeros(n, np.longdouble)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def test_georeferenced_single_step(icp):
    """pair(6000) at GEO_OFFSET, one iterate, origin = centroid_src.
    The sums: the existing (n + 8) 2^-52 sum|terms| against numpy's sums of the same fp64 terms.
    The solve, against x = (w, t') of a longdouble solve of the pairs' exact terms: the device sums
    differ from the exact ones by dA <= f absA + sum(|dJ||J| + |J||dJ|), dg likewise, with
    |dJ_rot| <= 3u (|p_a n_b| + |p_b n_a|) (the rounding of a - origin, two products, one
    subtraction), |dr| <= 4u sum|n_c (a_c - b_c)|; the solver adds at most 64u to the scaled matrix
    (the two scalings and a 6 x 6 Cholesky, |L||L^T| <= 6) and 8u |g_s|. With M = D A D of unit
    diagonal, M y = -D g, x = D y: |dy| <= |M^-1| (|dg_s| + |dM| |y|) / (1 - |M^-1| |dM|), and
    |dx_i| <= D_ii |dy| + u |x_i|. w is read back from R with 16u |w| more (Rodrigues and its log)."""
    tgt, src, _ = pf.pair(6000)
    tgt, src = tgt + R.GEO_OFFSET, src + R.GEO_OFFSET
    with icp.Context(0) as c:
        c.set_target(tgt)
        c.estimate_target_normals(16)
        c.set_source(src)
        st = c.iterate()
        o = np.array(st.centroid_src[:])
        s = c.plane_sums(o)
        idx, d = c.get_correspondences()
        nrm = c.get_target_normals()
        assert c.get_source().tobytes() == src.tobytes()
    use = (d <= st.threshold) & nrm[idx].any(1)
    n = int(use.sum())
    assert s.n == n and n >= 5000 and s.n + s.n_skipped == st.valid
    a, b, nr = src[use], tgt[idx[use]], nrm[idx[use]]
    A, g, r2, absA, absg, absr2 = pf.plane_sums_numpy(a, b, nr, o)
    f = (n + 8) * 2.0 ** -52
    gotA, gotg = np.array(s.A[:]).reshape(6, 6), np.array(s.g[:])
    assert np.array_equal(gotA, gotA.T)
    assert (np.abs(gotA - A) <= f * absA).all() and (np.abs(gotg - g) <= f * absg).all()
    assert abs(s.sum_r2 - r2) <= f * absr2

    # the exact terms in longdouble and the bounds of the fp64 terms' own roundings
    L = np.longdouble
    p, nl, ab = a.astype(L) - o.astype(L), nr.astype(L), a.astype(L) - b.astype(L)
    J = np.concatenate([np.cross(p, nl), nl], axis=1)
    r = (nl * ab).sum(1)
    pa, na = np.abs(p).astype(np.float64), np.abs(nr)
    dJ = np.zeros((n, 6))
    dJ[:, 0] = pa[:, 1] * na[:, 2] + pa[:, 2] * na[:, 1]
    dJ[:, 1] = pa[:, 2] * na[:, 0] + pa[:, 0] * na[:, 2]
    dJ[:, 2] = pa[:, 0] * na[:, 1] + pa[:, 1] * na[:, 0]
    dJ *= 3 * U
    dr = 4 * U * (na * np.abs(ab).astype(np.float64)).sum(1)
    Ja, ra = np.abs(J).astype(np.float64), np.abs(r).astype(np.float64)
    dA = f * absA + dJ.T @ Ja + Ja.T @ dJ
    dg = f * absg + dJ.T @ ra + Ja.T @ dr
    A_ld, g_ld = J.T @ J, J.T @ r
    D = 1.0 / np.sqrt(np.diag(A_ld))
    M = A_ld * D[:, None] * D[None, :]
    y = _solve_ld(M, -(D * g_ld))
    x = (D * y).astype(np.float64)
    Minv = np.linalg.norm(np.linalg.inv(M.astype(np.float64)), 2)
    Dd = D.astype(np.float64)
    dM = np.linalg.norm(dA * Dd[:, None] * Dd[None, :]) + 64 * U
    dgs = np.linalg.norm(dg * Dd) + 8 * U * float(np.linalg.norm((D * g_ld).astype(np.float64)))
    assert Minv * dM < 0.5
    dy = Minv * (dgs + dM * float(np.linalg.norm(y.astype(np.float64)))) / (1.0 - Minv * dM)
    bound = Dd * dy + U * np.abs(x)
    print(f"cond(M) = {np.linalg.cond(M.astype(np.float64)):.3g}, |M^-1| = {Minv:.3g}, |dM| = {dM:.3g}, bound = {bound}")

    # plane_solve's x: t' from the same sums about a zero origin (T's translation is then t' itself)
    T, ok = icp.plane_solve(s)
    zero = pf.sums_struct(icp, gotA, gotg, s.sum_r2, s.n, (0.0, 0.0, 0.0), s.n_skipped)
    T0, ok0 = icp.plane_solve(zero)
    assert ok == 1 and ok0 == 1 and T0[:3, :3].tobytes() == T[:3, :3].tobytes()
    Rm, tp = T[:3, :3], T0[:3, 3]
    vee = 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    sn = np.linalg.norm(vee)
    w = vee * (np.arcsin(sn) / sn)
    print(f"w error {np.abs(w - x[:3])}, t' error {np.abs(tp - x[3:])}")
    assert (np.abs(w - x[:3]) <= bound[:3] + 16 * U * np.linalg.norm(x[:3])).all()
    assert (np.abs(tp - x[3:]) <= bound[3:]).all()
    # T's translation: t' + c - R c
    want_t = tp.astype(L) + o.astype(L) - Rm.astype(L) @ o.astype(L)
    err_t = np.abs((T[:3, 3].astype(L) - want_t).astype(np.float64))
    print(f"translation error {err_t}, ulp {np.spacing(np.abs(o).max())}")
    assert (err_t <= 4 * np.spacing(np.abs(o).max())).all()
