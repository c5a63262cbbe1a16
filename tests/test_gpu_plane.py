"""The point-to-plane step on the GPU (plane_kernels.hip, engine.cpp): the sums against numpy with
the textbook summation bound, their determinism, skipped pairs, the registration against the
point-to-point metric on the corner fixture, the session against the low-level calls, the fallback
to the SVD step, and the default metric left as it was."""
import ctypes as C

import numpy as np
import pytest

import plane_fixtures as pf
from conftest import t_rmse

pytestmark = pytest.mark.gpu

N = 6000
K = 16


def _mat4_mul(icp, A, B):
    out = np.empty(16)
    a, b = np.ascontiguousarray(A, np.float64).reshape(16), np.ascontiguousarray(B, np.float64).reshape(16)
    icp.lib().icp_mat4_mul(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out.reshape(4, 4)


def _mat(rec_field):
    return np.array(rec_field[:], np.float64).reshape(4, 4)


@pytest.fixture(scope="module")
def ctx(icp):
    """A context holding the 6000-point target with its k = 16 normals."""
    with icp.Context(0) as c:
        c.set_target(pf.pair(N)[0])
        c.estimate_target_normals(K)
        yield c


def _numpy_sums(ctx, st, nrm=None):
    """The sums recomputed from what the context reports: (A, g, r2, bound arrays, n, n_skipped)."""
    tgt = pf.pair(N)[0]
    src = ctx.get_source()
    idx, d = ctx.get_correspondences()
    nrm = ctx.get_target_normals() if nrm is None else nrm
    valid = d <= st.threshold
    nz = nrm[idx].any(1)
    use = valid & nz
    origin = np.array(st.centroid_src[:])
    A, g, r2, absA, absg, absr2 = pf.plane_sums_numpy(src[use], tgt[idx[use]], nrm[idx[use]], origin)
    return A, g, r2, absA, absg, absr2, int(use.sum()), int((valid & ~nz).sum())


def _check_sums(s, want):
    A, g, r2, absA, absg, absr2, n, n_skipped = want
    assert s.n == n and s.n_skipped == n_skipped
    # any summation order of n terms, plus the terms' own roundings: (n + 8) 2^-52 sum |terms|
    f = (n + 8) * 2.0 ** -52
    gotA = np.array(s.A[:]).reshape(6, 6)
    assert np.array_equal(gotA, gotA.T)
    assert (np.abs(gotA - A) <= f * absA).all(), np.abs(gotA - A).max()
    assert (np.abs(np.array(s.g[:]) - g) <= f * absg).all()
    assert abs(s.sum_r2 - r2) <= f * absr2


@pytest.mark.parametrize("n_src", [63, 4097, 6000])  # under a wave, over one 4096-query part, two parts
def test_sums_match_numpy(icp, ctx, n_src):
    ctx.set_source(pf.pair(N)[1][:n_src])
    st = ctx.iterate()
    s = ctx.plane_sums(st.centroid_src)
    assert list(s.origin) == list(st.centroid_src)
    _check_sums(s, _numpy_sums(ctx, st))
    assert s.n_skipped == 0 and s.n + s.n_skipped == st.valid
    assert s.n >= 0.9 * n_src  # the case exercises the sums, not an empty set


def test_sums_are_deterministic(icp, ctx):
    tgt, src, _ = pf.pair(N)
    ctx.set_source(src)
    st = ctx.iterate()
    first = bytes(ctx.plane_sums(st.centroid_src))
    assert bytes(ctx.plane_sums(st.centroid_src)) == first
    for cfg in ({"candidate_cache": 0}, {"scan_groups": 1}):
        with icp.Context(0, cfg=cfg) as other:
            other.set_target(tgt)
            other.estimate_target_normals(K)
            other.set_source(src)
            st2 = other.iterate()
            assert list(st2.centroid_src) == list(st.centroid_src)
            assert bytes(other.plane_sums(st2.centroid_src)) == first, cfg


def test_pairs_with_a_zero_normal_are_skipped(icp, ctx):
    tgt, src, _ = pf.pair(N)
    nrm = ctx.get_target_normals()
    holes = nrm.copy()
    zeroed = np.random.default_rng(3).choice(N, 100, replace=False)
    holes[zeroed] = 0.0
    try:
        ctx.set_target_normals(holes)
        ctx.set_source(src)
        st = ctx.iterate()
        s = ctx.plane_sums(st.centroid_src)
        want = _numpy_sums(ctx, st, holes)
        idx, d = ctx.get_correspondences()
        assert want[-1] == int((np.isin(idx, zeroed) & (d <= st.threshold)).sum()) and want[-1] > 0
        _check_sums(s, want)
        assert s.n + s.n_skipped == st.valid
    finally:
        ctx.set_target_normals(nrm)


def _plane_session(icp, c, iterations):
    """A plane session of `iterations` steps with no early stop: (records, used_plane flags, sums)."""
    p = icp.params_default(max_iterations=iterations, flags=icp.FLAG_NO_EARLY_STOP)
    ses = c.session(p, metric=icp.METRIC_PLANE)
    recs, used, sums = [], [], []
    while not ses.done:
        recs.append(ses.step())
        s, u = ses.last_plane()
        used.append(u)
        sums.append(bytes(s))
    rc, res = ses.finish()
    assert rc == 0
    ses.close()
    return recs, used, sums, res


@pytest.mark.parametrize("n", [6000, 20000])
def test_registration_beats_point_to_point(icp, n):
    tgt, src, T_true = pf.pair(n)
    with icp.Context(0) as c:
        c.set_target(tgt)
        c.estimate_target_normals(K)
        c.set_source(src)
        recs, used, _, _ = _plane_session(icp, c, 5)
        assert len(recs) == 5 and used == [1] * 5
        plane_err = t_rmse(_mat(recs[-1].transform), T_true)
        c.set_source(src)
        ses = c.session(icp.params_default(max_iterations=30, flags=icp.FLAG_NO_EARLY_STOP))
        point_errs = []
        while not ses.done:
            point_errs.append(t_rmse(_mat(ses.step().transform), T_true))
        ses.close()
    assert len(point_errs) == 30
    print(f"n={n}: plane after 5 iterations {plane_err:.3e}; point best of 30 {min(point_errs):.3e} "
          f"at iteration {int(np.argmin(point_errs)) + 1}")
    assert plane_err < min(point_errs)


def test_session_equals_the_low_level_loop(icp, ctx):
    src = pf.pair(N)[1]
    ctx.set_source(src)
    recs, used, sums, _ = _plane_session(icp, ctx, 5)
    moved = ctx.get_source()
    assert used == [1] * 5
    ctx.set_source(src)
    T, Tc = None, np.eye(4)
    for it in range(5):
        st = ctx.iterate(T, it, icp.RULES_ENGINE, 3.0)
        s = ctx.plane_sums(st.centroid_src)
        assert bytes(s) == sums[it]
        T, ok = icp.plane_solve(s)
        assert ok == 1
        Tc = _mat4_mul(icp, T, Tc)
        assert T.tobytes() == _mat(recs[it].increment).tobytes()
        assert Tc.tobytes() == _mat(recs[it].transform).tobytes()
    ctx.apply(T)
    assert ctx.get_source().tobytes() == moved.tobytes()


def test_refused_solve_falls_back_to_the_svd_step(icp, ctx):
    src = pf.pair(N)[1]
    nrm = ctx.get_target_normals()
    flat = np.zeros_like(nrm)
    flat[:, 2] = 1.0
    try:
        ctx.set_target_normals(flat)
        ctx.set_source(src)
        recs, used, _, _ = _plane_session(icp, ctx, 4)
        assert used == [0] * 4
    finally:
        ctx.set_target_normals(nrm)
    ctx.set_source(src)
    ses = ctx.session(icp.params_default(max_iterations=4, flags=icp.FLAG_NO_EARLY_STOP))
    for k in range(4):
        rec = ses.step()
        assert bytes(rec) == bytes(recs[k])
    assert ses.done
    ses.close()


def test_default_metric_is_unchanged(icp, ctx):
    tgt, src, _ = pf.pair(N)
    p = icp.params_default(max_iterations=12)
    rc, res, hist, moved = icp.engine_register(p, src, tgt, device=0)
    assert rc == 0 and len(hist) > 0
    for metric in (None, icp.METRIC_POINT):
        ctx.set_source(src)
        ses = ctx.session(p) if metric is None else ctx.session(p, metric=metric)
        got = []
        while not ses.done:
            rec = ses.step()
            if rec is not None:
                got.append(rec)
            assert ses.last_plane()[1] == 0
        rc2, res2 = ses.finish()
        assert rc2 == 0
        if metric is None:  # after the first step the metric is fixed
            with pytest.raises(icp.IcpError) as e:
                ses.set_metric(icp.METRIC_PLANE)
            assert e.value.code == icp.EINVAL
        ses.close()
        assert [bytes(r) for r in got] == [bytes(h) for h in hist]
        assert bytes(res2.final_R) == bytes(res.final_R) and bytes(res2.final_t) == bytes(res.final_t)
        assert ctx.get_source().tobytes() == moved.tobytes()


def test_plane_metric_needs_normals_and_a_single_device(icp):
    tgt, src, _ = pf.pair(N)
    with icp.Context(0) as c:
        c.set_target(tgt)
        c.set_source(src)
        with pytest.raises(icp.IcpError) as e:
            c.session(icp.params_default(), metric=icp.METRIC_PLANE)
        assert e.value.code == icp.ENOTREADY
        c.estimate_target_normals(K)
        with pytest.raises(icp.IcpError) as e:
            c.plane_sums()  # before an iterate
        assert e.value.code == icp.ENOTREADY
        rc, res, hist = c.run(icp.params_default(max_iterations=3, flags=icp.FLAG_NO_EARLY_STOP), metric=icp.METRIC_PLANE)
        assert rc == 0 and res.success == 1 and len(hist) == 3
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as g:
        g.set_target(tgt)
        g.estimate_target_normals(K)
        g.set_source(src)
        g.iterate()
        with pytest.raises(icp.IcpError) as e:
            g.plane_sums()
        assert e.value.code == icp.EINVAL
