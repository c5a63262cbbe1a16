"""A generalized-ICP session (engine.cpp, ICP_METRIC_GICP) on the GPU: equal, bit for bit, to the
loop of the low-level calls it is made of, with and without a rejector; what it reports of its last
step; what it buys on the corner fixture and on the partial overlap, against the numpy loop run on
the context's own normals; the point sessions around it left as they were; the frame rule, the
refusals and the context's epsilon."""
import ctypes as C

import numpy as np
import pytest

import gicp_reference as G
import plane_fixtures as pf
import reject_fixtures as rf
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


def _gicp_session(icp, c, iterations, reject=None):
    """A generalized-ICP session of `iterations` steps with no early stop: (records, used flags, sums, result)."""
    p = icp.params_default(max_iterations=iterations, flags=icp.FLAG_NO_EARLY_STOP)
    ses = c.session(p, metric=icp.METRIC_GICP, reject=reject)
    recs, used, sums = [], [], []
    while not ses.done:
        recs.append(ses.step())
        s, u = ses.last_gicp()
        used.append(u)
        sums.append(s)
        assert ses.last_plane()[1] == 0
    rc, res = ses.finish()
    assert rc == 0
    ses.close()
    return recs, used, sums, res


@pytest.mark.parametrize("reject", [None, ("trim", 0.5), ("max_dist", 0.1)], ids=["sigma", "trim", "max_dist"])
def test_session_equals_the_low_level_loop(icp, ctx, reject):
    src = pf.pair(N)[1]
    mode = None if reject is None else (icp.REJECT_TRIM if reject[0] == "trim" else icp.REJECT_MAX_DIST, reject[1])
    ctx.set_source(src)
    ctx.estimate_source_normals(K)
    n0 = ctx.get_source_normals()
    recs, used, sums, _ = _gicp_session(icp, ctx, 5, mode)
    moved = ctx.get_source()
    assert used == [1] * 5 and len(recs) == 5 and all(r is not None for r in recs)
    assert all(s.epsilon == 1e-3 and s.n == r.valid_points for s, r in zip(sums, recs))
    ctx.set_source(src)
    ctx.set_source_normals(n0)
    T, Tc = None, np.eye(4)
    for it in range(5):
        st = ctx.iterate(T, it, icp.RULES_ENGINE, 3.0)
        if mode is None:
            s = ctx.gicp_sums(st.centroid_src, Tc[:3, :3], 1e-3)
        else:
            tau = ctx.residual_select(fraction=mode[1]).value if mode[0] == icp.REJECT_TRIM else mode[1]
            ps = ctx.pair_sums(tau)
            s = ctx.gicp_sums_at(ps.centroid_src, Tc[:3, :3], 1e-3, tau)
            assert (recs[it].threshold, recs[it].valid_points) == (tau, ps.valid)
        assert bytes(s) == bytes(sums[it]), it
        T, ok = icp.gicp_solve(s)
        assert ok == 1
        Tc = _mat4_mul(icp, T, Tc)
        assert T.tobytes() == _mat(recs[it].increment).tobytes(), it
        assert Tc.tobytes() == _mat(recs[it].transform).tobytes(), it
    ctx.apply(T)
    assert ctx.get_source().tobytes() == moved.tobytes()
    # the same session through the run call with its options record
    ctx.set_source(src)
    ctx.set_source_normals(n0)
    p = icp.params_default(max_iterations=5, flags=icp.FLAG_NO_EARLY_STOP)
    rc, res, hist = ctx.run(p, metric=icp.METRIC_GICP, reject=mode if mode else (icp.REJECT_SIGMA, 0.0))
    assert rc == 0 and [bytes(h) for h in hist] == [bytes(r) for r in recs]
    assert ctx.get_source().tobytes() == moved.tobytes()


@pytest.mark.parametrize("n", [6000, 20000])
def test_registration_beats_point_to_point(icp, n):
    tgt, src, T_true = pf.pair(n)
    with icp.Context(0) as c:
        c.set_target(tgt)
        c.estimate_target_normals(K)
        c.set_source(src)
        c.estimate_source_normals(K)
        nb, n0 = c.get_target_normals(), c.get_source_normals()
        recs, used, _, _ = _gicp_session(icp, c, 5)
        assert len(recs) == 5 and used == [1] * 5
        gicp_err = t_rmse(_mat(recs[-1].transform), T_true)
        c.set_source(src)
        ses = c.session(icp.params_default(max_iterations=30, flags=icp.FLAG_NO_EARLY_STOP))
        point_errs = []
        while not ses.done:
            point_errs.append(t_rmse(_mat(ses.step().transform), T_true))
        ses.close()
    assert len(point_errs) == 30
    want = G.numpy_gicp(tgt, src, T_true, 5, nrm_tgt=nb, nrm_src=n0)[-1]
    print(f"n={n}: GICP after 5 iterations {gicp_err:.3e} (numpy on the same normals {want:.3e}); "
          f"point best of 30 {min(point_errs):.3e} at iteration {int(np.argmin(point_errs)) + 1}")
    assert gicp_err < min(point_errs)
    assert abs(gicp_err - want) <= 5e-4 * want  # three digits


def test_trimmed_gicp_registers_the_partial_overlap(icp):
    tgt, src, T_true, _ = rf.overlap_pair()
    with icp.Context(0) as c:
        c.set_target(tgt)
        c.estimate_target_normals(K)
        c.set_source(src)
        c.estimate_source_normals(K)
        recs, used, _, _ = _gicp_session(icp, c, 5, (icp.REJECT_TRIM, 0.5))
    err = t_rmse(_mat(recs[-1].transform), T_true)
    print(f"overlap_pair, trim 0.5: GICP after 5 iterations {err:.3e}, used {used}")
    assert err <= 1e-3


def test_point_sessions_around_it_are_unchanged(icp, ctx):
    tgt, src, _ = pf.pair(N)
    p = icp.params_default(max_iterations=12)
    rc, res, hist, moved = icp.engine_register(p, src, tgt, device=0)
    assert rc == 0 and len(hist) > 0

    def point_session():
        ctx.set_source(src)
        ses = ctx.session(p)
        got = []
        while not ses.done:
            rec = ses.step()
            if rec is not None:
                got.append(rec)
            assert ses.last_gicp()[1] == 0 and ses.last_gicp()[0].n == 0
        rc2, res2 = ses.finish()
        ses.close()
        assert rc2 == 0 and [bytes(r) for r in got] == [bytes(h) for h in hist]
        assert bytes(res2.final_R) == bytes(res.final_R) and bytes(res2.final_t) == bytes(res.final_t)
        assert ctx.get_source().tobytes() == moved.tobytes()

    point_session()
    ctx.set_source(src)
    ctx.estimate_source_normals(K)
    ctx.set_gicp_epsilon(1e-2)
    try:
        _gicp_session(icp, ctx, 3)
    finally:
        ctx.set_gicp_epsilon(1e-3)
    point_session()
    # with the source's normals present, on the device-resident loop as icp_engine_run
    ctx.set_source(src)
    ctx.estimate_source_normals(K)
    rc3, res3, hist3 = ctx.run(p)
    assert rc3 == 0 and [bytes(h) for h in hist3] == [bytes(h) for h in hist]
    assert ctx.get_source().tobytes() == moved.tobytes()


def test_the_metric_needs_normals_made_where_the_source_stands(icp):
    tgt, src, T_true = pf.pair(N)
    p = icp.params_default(max_iterations=3, flags=icp.FLAG_NO_EARLY_STOP)

    def code(c, **kw):
        with pytest.raises(icp.IcpError) as e:
            c.session(p, metric=icp.METRIC_GICP, **kw)
        return e.value.code, str(e.value)

    with icp.Context(0) as c:
        c.set_target(tgt)
        c.set_source(src)
        assert code(c)[0] == icp.ENOTREADY  # no normals at all
        c.estimate_source_normals(K)
        assert code(c)[0] == icp.ENOTREADY  # none on the target
        c.estimate_target_normals(K)
        c.set_source(src)
        assert code(c)[0] == icp.ENOTREADY  # the new source has none
        c.estimate_source_normals(K)
        c.session(p, metric=icp.METRIC_GICP).close()
        # moved since the normals were made: by apply, by an iterate's fused transform, by a device-loop run
        c.apply(T_true)
        rc, msg = code(c)
        assert rc == icp.ENOTREADY and "moved" in msg
        c.estimate_source_normals(K)
        c.session(p, metric=icp.METRIC_GICP).close()
        c.iterate()  # no transform: the source stays
        c.session(p, metric=icp.METRIC_GICP).close()
        c.iterate(T_true, 1)
        assert code(c) == (rc, msg)
        c.estimate_source_normals(K)
        c.session(p, metric=icp.METRIC_GICP).close()
        assert c.run(icp.params_default(max_iterations=4))[0] == 0
        assert code(c) == (rc, msg)
        # a finished generalized-ICP session has moved it too
        c.set_source(src)
        c.estimate_source_normals(K)
        assert c.run(p, metric=icp.METRIC_GICP)[0] == 0
        assert code(c) == (rc, msg)
        # setting them where the source stands is the caller's word for their frame
        c.set_source_normals(c.get_source_normals())
        c.session(p, metric=icp.METRIC_GICP).close()
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as g:
        g.set_target(tgt)
        g.estimate_target_normals(K)
        g.set_source(src)
        assert code(g)[0] == icp.EINVAL


def test_the_context_s_epsilon_changes_the_step(icp, ctx):
    src = pf.pair(N)[1]
    steps = {}
    try:
        for eps in (1e-3, 2.0 ** -4):
            ctx.set_gicp_epsilon(eps)
            ctx.set_source(src)
            ctx.estimate_source_normals(K)
            recs, used, sums, _ = _gicp_session(icp, ctx, 2)
            assert used == [1, 1] and [s.epsilon for s in sums] == [eps, eps]
            steps[eps] = bytes(recs[0].increment)
    finally:
        ctx.set_gicp_epsilon(1e-3)
    assert steps[1e-3] != steps[2.0 ** -4]
