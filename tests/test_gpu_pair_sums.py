"""icp_hip_pair_sums and icp_hip_plane_sums_at on the GPU (reject_kernels.hip, plane_kernels.hip):
the pair sums against stats_reference.pairs_ref on the same valid set with that module's derived
bounds (reject_fixtures.check_pair_sums), at the selected thresholds, +inf, a threshold below every
residual and one of a set with ties; with and without the georeferenced offset; the valid count of
the iterate at its own threshold; the same bytes from two calls and from contexts that search
differently; the plane sums at the iterate's threshold byte-equal to icp_hip_plane_sums, and at a
selected threshold against numpy."""
import numpy as np
import pytest

import plane_fixtures as pf
import reject_fixtures as rf
import stats_reference as R

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 64, 65, 4096, 4097, 16385]


@pytest.fixture(scope="module")
def ctxs(icp):
    """Contexts holding shape_pair's target, plain and with stats_reference.GEO_OFFSET."""
    with icp.Context(0) as plain, icp.Context(0) as geo:
        plain.set_target(R.shape_pair(1, 5000)[0])
        geo.set_target(R.shape_pair(1, 5000, True)[0])
        yield {False: plain, True: geo}


def _state(c, tgt):
    idx, d = c.get_correspondences()
    return d, c.get_source(), tgt[idx]


@pytest.mark.parametrize("geo", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_against_the_reference(icp, ctxs, n, geo):
    c = ctxs[geo]
    tgt, src = R.shape_pair(n, 5000, geo)
    c.set_source(src)
    st = c.iterate()
    d, a, b = _state(c, tgt)
    ratios = {}
    thresholds = [c.residual_select(fraction=f).value for f in (0.5, 1.0)] + [float("inf"), float(d.min()) / 2]
    for thr in thresholds:
        ps = c.pair_sums(thr)
        rf.check_pair_sums(ps, d, a, b, thr, ratios, f"n {n} geo {geo} threshold {thr}")
    assert c.pair_sums(float("inf")).valid == n and c.pair_sums(float(d.min()) / 2).valid == 0
    assert c.pair_sums(st.threshold).valid == st.valid  # the iterate's own threshold, finite data
    R.print_ratios(f"pair sums n {n} geo {geo}", ratios)


def test_threshold_with_ties(icp):
    """A threshold that many residuals equal: valid == n_less + n_equal exactly."""
    tgt = R.lattice(17)
    r = rf.select_sets()["two_values_and_one"]
    with icp.Context(0) as c:
        c.set_target(tgt)
        c.set_source(R.lattice_queries(tgt, r))
        c.iterate()
        d, a, b = _state(c, tgt)
        for rank in (1, 2, len(r) // 3, len(r) // 3 + 1, len(r)):
            sel = c.residual_select(rank=rank)
            ps = c.pair_sums(sel.value)
            assert ps.valid == sel.n_less + sel.n_equal and ps.n_finite == sel.n_finite
            rf.check_pair_sums(ps, d, a, b, sel.value, None, f"ties rank {rank}")


def test_non_finite_rows_are_left_out(icp):
    tgt, src = R.degenerate_case("nan", 4097)
    with icp.Context(0) as c:
        c.set_target(tgt)
        c.set_source(src)
        st = c.iterate()
        assert st.valid == 0 and st.n_bad == 3  # the cull's mean is NaN
        d, a, b = _state(c, tgt)
        ps = c.pair_sums(float("inf"))
        assert ps.valid == 4094 and ps.n_finite == 4094
        rf.check_pair_sums(ps, d, a, b, float("inf"), None, "nan rows")


def test_same_bytes(icp, ctxs):
    tgt, src = R.shape_pair(16385, 5000)
    c = ctxs[False]
    c.set_source(src)
    c.iterate()
    thr = c.residual_select(fraction=0.5).value
    first = bytes(c.pair_sums(thr))
    assert bytes(c.pair_sums(thr)) == first
    for cfg in ({"candidate_cache": 0}, {"scan_groups": 1}):
        with icp.Context(0, cfg=cfg) as other:
            other.set_target(tgt)
            other.set_source(src)
            other.iterate()
            assert bytes(other.pair_sums(thr)) == first, cfg


def test_the_iterate_is_left_as_it_was(icp, ctxs):
    tgt, src = R.shape_pair(4097, 5000)
    c = ctxs[False]
    c.set_source(src)
    c.iterate()
    idx, d = c.get_correspondences()
    moved = c.get_source()
    c.pair_sums(float(np.median(d)))
    idx2, d2 = c.get_correspondences()
    assert idx2.tobytes() == idx.tobytes() and d2.tobytes() == d.tobytes() and c.get_source().tobytes() == moved.tobytes()


def test_argument_errors(icp):
    tgt, src = R.shape_pair(65, 5000)
    with icp.Context(0) as c:
        with pytest.raises(icp.IcpError) as e:
            c.pair_sums(float("nan"))
        assert e.value.code == icp.EINVAL
        with pytest.raises(icp.IcpError) as e:
            c.pair_sums(1.0)
        assert e.value.code == icp.ENOTREADY  # no target
        c.set_target(tgt)
        c.set_source(src)
        for call in (lambda: c.pair_sums(1.0), lambda: c.plane_sums_at((0.0, 0.0, 0.0), 1.0)):
            with pytest.raises(icp.IcpError) as e:
                call()
            assert e.value.code == icp.ENOTREADY  # no iterate; the plane sums: no normals either
        c.iterate()
        assert c.pair_sums(float("inf")).valid == 65
        with pytest.raises(icp.IcpError) as e:
            c.plane_sums_at((0.0, 0.0, 0.0), 1.0)
        assert e.value.code == icp.ENOTREADY  # no normals
        c.estimate_target_normals(8)
        for origin, thr in (((0.0, 0.0, 0.0), float("nan")), ((float("inf"), 0.0, 0.0), 1.0)):
            with pytest.raises(icp.IcpError) as e:
                c.plane_sums_at(origin, thr)
            assert e.value.code == icp.EINVAL
        c.comm_init_host(2, 0, lambda local: np.stack([local, local]))
        c.iterate()
        for call in (lambda: c.pair_sums(1.0), lambda: c.plane_sums_at((0.0, 0.0, 0.0), 1.0)):
            with pytest.raises(icp.IcpError) as e:
                call()
            assert e.value.code == icp.EINVAL and "communicator" in str(e.value)
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as g:
        g.set_target(tgt)
        g.estimate_target_normals(8)
        g.set_source(src)
        g.iterate()
        for call in (lambda: g.pair_sums(1.0), lambda: g.plane_sums_at((0.0, 0.0, 0.0), 1.0)):
            with pytest.raises(icp.IcpError) as e:
                call()
            assert e.value.code == icp.EINVAL and "multi-device" in str(e.value)


# ---- the plane sums at a threshold

@pytest.fixture(scope="module")
def plane_ctx(icp):
    with icp.Context(0) as c:
        c.set_target(pf.pair(6000)[0])
        c.estimate_target_normals(16)
        yield c


@pytest.mark.parametrize("n_src", [63, 4097, 6000])
def test_plane_sums_at_the_iterates_threshold_are_plane_sums(icp, plane_ctx, n_src):
    plane_ctx.set_source(pf.pair(6000)[1][:n_src])
    st = plane_ctx.iterate()
    want = bytes(plane_ctx.plane_sums(st.centroid_src))
    assert bytes(plane_ctx.plane_sums_at(st.centroid_src, st.threshold)) == want
    assert bytes(plane_ctx.plane_sums(st.centroid_src)) == want


@pytest.mark.parametrize("n_src", [63, 4097, 6000])
def test_plane_sums_at_a_selected_threshold(icp, plane_ctx, n_src):
    tgt = pf.pair(6000)[0]
    plane_ctx.set_source(pf.pair(6000)[1][:n_src])
    plane_ctx.iterate()
    src = plane_ctx.get_source()
    idx, d = plane_ctx.get_correspondences()
    nrm = plane_ctx.get_target_normals()
    for thr in (plane_ctx.residual_select(fraction=0.5).value, float("inf")):
        ps = plane_ctx.pair_sums(thr)
        origin = np.array(ps.centroid_src[:])
        s = plane_ctx.plane_sums_at(origin, thr)
        use = np.isfinite(d) & (d <= thr) & nrm[idx].any(1)
        A, g, r2, absA, absg, absr2 = pf.plane_sums_numpy(src[use], tgt[idx[use]], nrm[idx[use]], origin)
        n = int(use.sum())
        assert s.n == n and s.n + s.n_skipped == ps.valid and list(s.origin) == list(origin)
        f = (n + 8) * 2.0 ** -52  # test_gpu_plane's bound: any order of n terms, plus the terms' own roundings
        gotA = np.array(s.A[:]).reshape(6, 6)
        assert np.array_equal(gotA, gotA.T)
        assert (np.abs(gotA - A) <= f * absA).all() and (np.abs(np.array(s.g[:]) - g) <= f * absg).all()
        assert abs(s.sum_r2 - r2) <= f * absr2
