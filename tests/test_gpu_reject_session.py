"""A session with a rejector (engine.cpp icp_session_set_rejection) on the GPU: equal, bit for bit,
to the loop of the low-level calls it is made of, with both metrics and both rules; the default left
as it was; what the trimmed rule buys on the partial-overlap fixture, where the reference's cull ends
worse than it started; non-finite rows; the refusals."""
import ctypes as C

import numpy as np
import pytest

import reject_fixtures as rf

pytestmark = pytest.mark.gpu

K_NORMALS = 12


def _mat4_mul(icp, A, B):
    out = np.empty(16)
    a, b = np.ascontiguousarray(A, np.float64).reshape(16), np.ascontiguousarray(B, np.float64).reshape(16)
    icp.lib().icp_mat4_mul(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out.reshape(4, 4)


def _mat(rec_field):
    return np.array(rec_field[:], np.float64).reshape(4, 4)


@pytest.fixture(scope="module")
def ctx(icp):
    """A context holding the fixture's target with its 12-neighbour normals."""
    with icp.Context(0) as c:
        c.set_target(rf.overlap_pair()[0])
        c.estimate_target_normals(K_NORMALS)
        yield c


def _session(icp, c, iterations, metric=None, reject=None):
    """`iterations` steps with no early stop: (records, used_plane flags, the result)."""
    p = icp.params_default(max_iterations=iterations, flags=icp.FLAG_NO_EARLY_STOP)
    ses = c.session(p, metric=metric, reject=reject)
    recs, used = [], []
    while not ses.done:
        recs.append(ses.step())
        used.append(ses.last_plane()[1])
    rc, res = ses.finish()
    ses.close()
    return recs, used, rc, res


@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("reject", [("trim", 0.5), ("trim", 1.0), ("max_dist", 0.1)])
def test_session_equals_the_low_level_loop(icp, ctx, metric, reject):
    src = rf.overlap_pair()[1]
    mode = icp.REJECT_TRIM if reject[0] == "trim" else icp.REJECT_MAX_DIST
    plane = metric == "plane"
    ctx.set_source(src)
    recs, used, rc, _ = _session(icp, ctx, 5, icp.METRIC_PLANE if plane else None, (mode, reject[1]))
    assert rc == 0 and len(recs) == 5 and all(r is not None for r in recs)
    moved = ctx.get_source()
    ctx.set_source(src)
    T, Tc = None, np.eye(4)
    for it in range(5):
        st = ctx.iterate(T, it, icp.RULES_ENGINE, 3.0)
        tau = ctx.residual_select(fraction=reject[1]).value if mode == icp.REJECT_TRIM else reject[1]
        ps = ctx.pair_sums(tau)
        st.centroid_src[:], st.centroid_tgt[:], st.H[:] = ps.centroid_src[:], ps.centroid_tgt[:], ps.H[:]
        T = icp.best_fit_from_stats(st)  # session_core_step's best fit
        if plane:
            Tp, ok = icp.plane_solve(ctx.plane_sums_at(ps.centroid_src, tau))
            assert ok == used[it]
            T = Tp if ok else T
        Tc = _mat4_mul(icp, T, Tc)
        h = recs[it]
        assert (h.threshold, h.valid_points, h.rmse) == (tau, ps.valid, ps.rmse), it
        assert (h.mean, h.std, h.outlier_points) == (st.mean, st.std, st.n - ps.valid), it
        assert T.tobytes() == _mat(h.increment).tobytes(), it
        assert Tc.tobytes() == _mat(h.transform).tobytes(), it
    ctx.apply(T)
    assert ctx.get_source().tobytes() == moved.tobytes()
    if plane:
        assert used == [1] * 5
    # the same session through the run call with its options record
    ctx.set_source(src)
    p = icp.params_default(max_iterations=5, flags=icp.FLAG_NO_EARLY_STOP)
    rc, res, hist = ctx.run(p, metric=icp.METRIC_PLANE if plane else icp.METRIC_POINT, reject=(mode, reject[1]))
    assert rc == 0 and [bytes(h) for h in hist] == [bytes(r) for r in recs]
    assert ctx.get_source().tobytes() == moved.tobytes()


def test_default_is_unchanged(icp, ctx):
    tgt, src, _, _ = rf.overlap_pair()
    p = icp.params_default(max_iterations=12)
    rc, res, hist, moved = icp.engine_register(p, src, tgt, device=0)
    assert rc == 0 and len(hist) > 0
    for explicit in (False, True):
        ctx.set_source(src)
        ses = ctx.session(p, reject=(icp.REJECT_SIGMA, 0.0)) if explicit else ctx.session(p)
        got = []
        while not ses.done:
            rec = ses.step()
            if rec is not None:
                got.append(rec)
        rc2, res2 = ses.finish()
        ses.close()
        assert rc2 == 0 and [bytes(r) for r in got] == [bytes(h) for h in hist]
        assert bytes(res2.final_R) == bytes(res.final_R) and bytes(res2.final_t) == bytes(res.final_t)
        assert ctx.get_source().tobytes() == moved.tobytes()
    # and through the options record, on the device-resident loop as icp_engine_run
    ctx.set_source(src)
    rc3, res3, hist3 = ctx.run(p, reject=(icp.REJECT_SIGMA, 0.0))
    assert rc3 == 0 and [bytes(h) for h in hist3] == [bytes(h) for h in hist]
    assert ctx.get_source().tobytes() == moved.tobytes()


def test_trimmed_point_to_point_survives_partial_overlap(icp, ctx):
    """After 20 iterations TRIM 0.5 is below the initial error; the reference's cull is above it and
    at least 5 times TRIM's (CPU simulation: 1.7e-2 against 2.5e-1)."""
    _, src, T_true, _ = rf.overlap_pair()
    e0 = rf.t_rmse(np.eye(4), T_true)
    errs = {}
    for name, reject in (("sigma", None), ("trim", (icp.REJECT_TRIM, 0.5))):
        ctx.set_source(src)
        recs, _, rc, _ = _session(icp, ctx, 20, None, reject)
        assert rc == 0 and len(recs) == 20
        errs[name] = [rf.t_rmse(_mat(r.transform), T_true) for r in recs]
    print(f"point: initial {e0:.3e}; 3 sigma after 5 / 20 iterations {errs['sigma'][4]:.3e} / {errs['sigma'][19]:.3e}; "
          f"trim 0.5 {errs['trim'][4]:.3e} / {errs['trim'][19]:.3e}")
    assert errs["trim"][19] < e0 < errs["sigma"][19]
    assert errs["sigma"][19] >= 5 * errs["trim"][19]


def test_trimmed_point_to_plane_survives_partial_overlap(icp, ctx):
    """After 5 iterations TRIM 0.5 is at most 1e-3, the reference's cull at least 1e-2 (CPU
    simulation: 6.0e-5 against 8.5e-2)."""
    _, src, T_true, _ = rf.overlap_pair()
    errs = {}
    for name, reject in (("sigma", None), ("trim", (icp.REJECT_TRIM, 0.5))):
        ctx.set_source(src)
        recs, used, rc, _ = _session(icp, ctx, 5, icp.METRIC_PLANE, reject)
        assert rc == 0 and len(recs) == 5 and used == [1] * 5
        errs[name] = rf.t_rmse(_mat(recs[-1].transform), T_true)
    print(f"plane after 5 iterations: 3 sigma {errs['sigma']:.3e}; trim 0.5 {errs['trim']:.3e}")
    assert errs["trim"] <= 1e-3 and errs["sigma"] >= 1e-2


def test_non_finite_rows(icp, ctx):
    """Three NaN rows: the cull's session ends too-few at its first step (the mean is NaN); the
    trimmed plane session registers, the NaN rows ranked out."""
    _, src, T_true, _ = rf.overlap_pair()
    bad = rf.with_nan_rows(src)
    p = icp.params_default(max_iterations=5, flags=icp.FLAG_NO_EARLY_STOP)
    ctx.set_source(bad)
    ses = ctx.session(p)
    assert ses.step() is None and ses.done
    rc, res = ses.finish()
    ses.close()
    assert rc == -11 and res.status == 3  # ICP_ENGINE_TOO_FEW, ICP_STATUS_TOO_FEW
    ctx.set_source(bad)
    recs, used, rc, _ = _session(icp, ctx, 5, icp.METRIC_PLANE, (icp.REJECT_TRIM, 0.5))
    assert rc == 0 and len(recs) == 5 and used == [1] * 5
    err = rf.t_rmse(_mat(recs[-1].transform), T_true)
    print(f"plane, trim 0.5, three NaN rows, after 5 iterations: {err:.3e}")
    assert err <= 1e-3
    # the record keeps the iterate's own mean and std (NaN: icp_iteration_record has no n_bad field;
    # the three rows show in the counts of the calls the step is made of)
    n = len(bad)
    for r in recs:
        assert np.isnan(r.mean) and np.isnan(r.std)
        assert r.valid_points >= icp.trim_rank(0.5, n - 3) and r.outlier_points == n - r.valid_points
    assert ctx.residual_select(fraction=1.0).n_finite == n - 3
    assert int(np.isnan(ctx.get_source()).any(1).sum()) == 3


def test_refusals(icp, ctx):
    tgt, src, _, _ = rf.overlap_pair()
    p = icp.params_default(max_iterations=4, flags=icp.FLAG_NO_EARLY_STOP)
    ctx.set_source(src)
    ses = ctx.session(p)
    for mode, param in ((3, 0.5), (-1, 0.5), (icp.REJECT_TRIM, 0.0), (icp.REJECT_TRIM, 1.5), (icp.REJECT_TRIM, float("nan")),
                        (icp.REJECT_MAX_DIST, 0.0), (icp.REJECT_MAX_DIST, -1.0), (icp.REJECT_MAX_DIST, float("inf")),
                        (icp.REJECT_MAX_DIST, float("nan"))):
        with pytest.raises(icp.IcpError) as e:
            ses.set_rejection(mode, param)
        assert e.value.code == icp.EINVAL, (mode, param)
    ses.set_rejection(icp.REJECT_TRIM, 0.5)
    ses.set_rejection(icp.REJECT_SIGMA)  # before the first step it may still change
    ses.step()
    with pytest.raises(icp.IcpError) as e:
        ses.set_rejection(icp.REJECT_TRIM, 0.5)
    assert e.value.code == icp.EINVAL and "stepped" in str(e.value)
    ses.close()
    # the options record: an unknown version, a bad mode
    ctx.set_source(src)
    res, hist = icp._lib.Result(), (icp._lib.IterationRecord * 4)()
    opt = icp.run_options(version=2)
    assert icp.lib().icp_engine_run_options(ctx.handle, C.byref(p), C.byref(opt), C.byref(res), hist, 4, None) == icp.EINVAL
    rc, _, _ = ctx.run(p, reject=(7, 0.5))
    assert rc == icp.EINVAL
    with icp.Context(0) as c:
        c.set_target(tgt)
        c.set_source(src)
        c.comm_init_host(2, 0, lambda local: np.stack([local, local]))
        with pytest.raises(icp.IcpError) as e:
            c.session(p, reject=(icp.REJECT_TRIM, 0.5))
        assert e.value.code == icp.EINVAL and "communicator" in str(e.value)
        c.session(p, reject=(icp.REJECT_SIGMA, 0.0)).close()
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as g:
        g.set_target(tgt)
        g.set_source(src)
        for mode, param in ((icp.REJECT_TRIM, 0.5), (icp.REJECT_MAX_DIST, 0.1)):
            with pytest.raises(icp.IcpError) as e:
                g.session(p, reject=(mode, param))
            assert e.value.code == icp.EINVAL and "multi-device" in str(e.value)
