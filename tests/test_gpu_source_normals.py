"""The source's normals (ctx_gicp.cpp, icp_hip_estimate_source_normals and the set / get calls): the
rule is the target's word for word, so the bytes are those the same cloud gets as the target of a
second context, and those of plane_reference.normals_model on the brute-force (fl(d2), index) lists,
with and without a viewpoint and under both query orders (the result is in the caller's order and
does not depend on the slots). Then the round trips, the refusals and what drops the normals."""
import numpy as np
import pytest

import plane_fixtures as pf
import plane_reference as R
import reject_fixtures as rf

pytestmark = pytest.mark.gpu


def _clouds():
    src = pf.pair(6000)[1]
    return {
        "n63": (src[:63], 8),          # under a wave
        "n4097": (src[:4097], 16),     # several blocks of the k-NN walk, one over 4096
        "pair6000": (src, 16),
        "deep": (R.deep_copies()[0], 32),                      # copies no subdivision separates: the deepest private tree
        "strips": (R.strip_clusters(8, "geo", 1.0)[0], 8),     # above the rank rule, georeferenced
        "lines": (R.line_clusters(8, "geo", 1.0)[0], 8),       # below it: zero normals
    }


CLOUDS = _clouds()


def _view(cloud):
    return cloud.mean(0) + 3.0


@pytest.fixture(scope="module")
def wanted(icp):
    """(name, with viewpoint) -> (the normals the cloud gets as a target, the model's): made once."""
    out = {}
    for name, (cloud, k) in CLOUDS.items():
        idx = pf.knn_brute(cloud, cloud, k)[0]
        with icp.Context(0) as c:
            c.set_target(cloud)
            for with_view in (False, True):
                view = _view(cloud) if with_view else None
                c.estimate_target_normals(k, view)
                out[name, with_view] = (c.get_target_normals(), R.normals_model(cloud, idx, view, icp))
    return out


def _differ(got, want):
    return np.flatnonzero((got.view(np.int64) != want.view(np.int64)).any(1))


@pytest.mark.parametrize("query_order", [0, 1])
@pytest.mark.parametrize("with_view", [False, True], ids=["no_viewpoint", "viewpoint"])
@pytest.mark.parametrize("name", list(CLOUDS))
def test_bytes_are_the_target_rule_s(icp, wanted, name, with_view, query_order):
    cloud, k = CLOUDS[name]
    as_target, model = wanted[name, with_view]
    with icp.Context(0, cfg={"query_order": query_order}) as c:
        c.set_source(cloud)
        c.estimate_source_normals(k, _view(cloud) if with_view else None)
        got = c.get_source_normals()
        assert c.get_source().tobytes() == cloud.tobytes()  # the source itself is untouched
    for want, what in ((as_target, "the cloud as a target"), (model, "the model")):
        d = _differ(got, want)
        assert len(d) == 0, f"{what}: {len(d)} of {len(cloud)} normals differ, first at {d[0]}: {got[d[0]]!r} for {want[d[0]]!r}"
    if name == "lines":
        assert not got.any()
    if name == "strips":
        assert np.abs(np.einsum("ni,ni->n", got, got) - 1.0).max() <= 2.0 ** -50
    if name == "deep":
        assert (got[R.deep_copies()[1]] == 0.0).all()


def test_the_resident_source_as_it_stands(icp):
    """After a move the normals are those of the moved cloud."""
    cloud, k = CLOUDS["n4097"]
    T = pf.pair(6000)[2]
    with icp.Context(0) as c:
        c.set_source(cloud)
        c.apply(T)
        moved = c.get_source()
        c.estimate_source_normals(k)
        got = c.get_source_normals()
        c.set_target(moved)
        c.estimate_target_normals(k)
        assert got.tobytes() == c.get_target_normals().tobytes()
    assert np.abs(moved - cloud).max() > 0.01


def test_set_get_round_trips(icp, wanted):
    cloud, k = CLOUDS["n4097"]
    n = len(cloud)
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.sqrt((nrm * nrm).sum(1))[:, None]
    nrm[rng.choice(n, 50, replace=False)] = 0.0
    nrm[17] = [0.6, 0.8, 0.0]
    assert (np.abs((nrm * nrm).sum(1) - 1.0)[nrm.any(1)] <= 1e-12).all()
    for query_order in (0, 1):
        with icp.Context(0, cfg={"query_order": query_order}) as c:
            c.set_source(cloud)
            with pytest.raises(icp.IcpError) as e:
                c.get_source_normals()
            assert e.value.code == icp.ENOTREADY
            c.set_source_normals(nrm)
            assert c.get_source_normals().tobytes() == nrm.tobytes()
            # the device forms: set from a buffer, read into a buffer
            other = np.ascontiguousarray(nrm[::-1])
            d_in, d_out = c.to_device(other), c.device_buffer(other.nbytes)
            c.set_source_normals(d_in)
            assert c.get_source_normals().tobytes() == other.tobytes()
            c.get_source_normals(d_out)
            assert d_out.download(np.float64, (n, 3)).tobytes() == other.tobytes()
            # a non-unit row (or a NaN) is refused and the old normals stay, host and device form
            for bad_row in (nrm[17] * (1.0 + 1e-9), [0.6, np.nan, 0.0]):
                bad = nrm.copy()
                bad[17] = bad_row
                for form in (bad, c.to_device(bad)):
                    with pytest.raises(icp.IcpError) as e:
                        c.set_source_normals(form)
                    assert e.value.code == icp.EINVAL and "1 rows" in str(e.value)
                    assert c.get_source_normals().tobytes() == other.tobytes()
            # an estimate replaces them; a new source drops them, in every variant
            c.estimate_source_normals(k)
            assert c.get_source_normals().tobytes() == wanted["n4097", False][0].tobytes()
            c.set_source(cloud)
            with pytest.raises(icp.IcpError) as e:
                c.get_source_normals()
            assert e.value.code == icp.ENOTREADY
            c.set_source_normals(nrm)
            c.set_source_device(c.to_device(cloud), n)
            with pytest.raises(icp.IcpError) as e:
                c.get_source_normals(d_out)
            assert e.value.code == icp.ENOTREADY


def test_refusals(icp):
    cloud, k = CLOUDS["n63"]
    with icp.Context(0) as c:
        for call in (lambda: c.estimate_source_normals(8), lambda: c.get_source_normals()):
            with pytest.raises(icp.IcpError) as e:
                call()
            assert e.value.code == icp.ENOTREADY  # no source
        c.set_source(cloud)
        for bad_k in (2, icp.KNN_MAX + 1, 64):
            with pytest.raises(icp.IcpError) as e:
                c.estimate_source_normals(bad_k)
            assert e.value.code == icp.EINVAL
        c.set_source(cloud[:5])
        with pytest.raises(icp.IcpError) as e:
            c.estimate_source_normals(6)  # above the source size
        assert e.value.code == icp.EINVAL
        c.estimate_source_normals(5)
        c.set_source(cloud)
        for view in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0)):
            with pytest.raises(icp.IcpError) as e:
                c.estimate_source_normals(8, view)
            assert e.value.code == icp.EINVAL
        with pytest.raises(icp.IcpError) as e:
            c.get_source_normals()  # nothing of the refused calls stayed
        assert e.value.code == icp.ENOTREADY
        # a source with non-finite coordinates: the text says how many; the set call still works
        holes = rf.with_nan_rows(cloud)
        c.set_source(holes)
        with pytest.raises(icp.IcpError) as e:
            c.estimate_source_normals(8)
        assert e.value.code == icp.EINVAL and "3 source points" in str(e.value)
        nrm = np.zeros((len(cloud), 3))
        nrm[:, 2] = 1.0
        c.set_source_normals(nrm)
        assert c.get_source_normals().tobytes() == nrm.tobytes()
        for bad_ptr in (0, 8 + 4):
            with pytest.raises(icp.IcpError) as e:
                icp._lib._check(icp.lib().icp_hip_set_source_normals_device(c._h, bad_ptr))
            assert e.value.code == icp.EINVAL
    # the source of a device group is sharded: every call refuses
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as g:
        g.set_source(cloud)
        nrm = np.zeros((len(cloud), 3))
        for call in (lambda: g.estimate_source_normals(8), lambda: g.set_source_normals(nrm),
                     lambda: g.get_source_normals()):
            with pytest.raises(icp.IcpError) as e:
                call()
            assert e.value.code == icp.EINVAL
