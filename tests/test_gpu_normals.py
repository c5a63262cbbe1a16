"""Target normals (icp_hip_estimate_target_normals, knn_kernels.hip) on the corner fixture: the
neighbour sets are the brute-force k-NN sets, the normals numpy's eigenvectors on those sets, the
sign rule, degenerate neighbourhoods, and set / get / invalidation."""
import numpy as np
import pytest

import plane_fixtures as pf

pytestmark = pytest.mark.gpu

N = 6000
VIEW = np.array([2.0, 2.0, 2.0])


@pytest.fixture(scope="module")
def tgt():
    return pf.pair(N)[0]


@pytest.fixture(scope="module")
def ctx(icp, tgt):
    with icp.Context(0) as c:
        c.set_target(tgt)
        yield c


@pytest.fixture(scope="module")
def sets(tgt):
    """Brute-force neighbour sets of every target point (k = 16; the first 8 columns are k = 8's)."""
    return pf.knn_brute(tgt, tgt, 16)


def _eigh_normals(tgt, idx):
    """numpy's smallest eigenvector of each neighbourhood's covariance, and lambda0 / lambda1."""
    p = tgt[idx]                                   # (n, k, 3)
    d = p - p.mean(1, keepdims=True)
    Cm = np.einsum("nki,nkj->nij", d, d)
    w, v = np.linalg.eigh(Cm)
    return v[:, :, 0], w[:, 0] / w[:, 1]


@pytest.mark.parametrize("k", [8, 16])
def test_neighbour_sets_are_exact(ctx, tgt, sets, k):
    idx, d2 = ctx.knn(tgt, k)
    assert np.array_equal(idx, sets[0][:, :k]) and d2.tobytes() == sets[1][:, :k].tobytes()
    assert np.array_equal(idx[:, 0], np.arange(N))  # no copies: every point is its own first neighbour


@pytest.mark.parametrize("view", [None, VIEW], ids=["no_viewpoint", "viewpoint"])
@pytest.mark.parametrize("k", [8, 16])
def test_normals_match_eigh(ctx, tgt, sets, k, view):
    ctx.estimate_target_normals(k, view)
    nrm = ctx.get_target_normals()
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-14
    ref, ratio = _eigh_normals(tgt, sets[0][:, :k])
    good = ratio <= 0.1  # the eigenvector is well conditioned
    left_out = 1.0 - good.mean()
    assert left_out <= 0.10, left_out
    cosang = np.abs(np.einsum("ni,ni->n", nrm[good], ref[good]))
    sinang = np.linalg.norm(np.cross(nrm[good], ref[good]), axis=1)
    angle = np.arctan2(sinang, cosang)
    assert angle.max() <= 1e-9, angle.max()
    if view is None:
        lead = np.abs(nrm).argmax(1)  # first maximum: the lowest axis on a tie
        assert (nrm[np.arange(N), lead] > 0).all()
    else:
        assert (np.einsum("ni,ni->n", nrm[good], view - tgt[good]) >= 0).all()


def test_degenerate_neighbourhoods(icp):
    rng = np.random.default_rng(21)
    tgt = rng.uniform(-1.0, 1.0, size=(600, 3))
    where = np.sort(rng.choice(600, 20, replace=False))
    tgt[where] = [0.375, -0.5, 0.25]  # dyadic: the mean of copies is exact
    with icp.Context(0) as c:
        c.set_target(tgt)
        c.estimate_target_normals(8)
        nrm = c.get_target_normals()
    zero = (nrm == 0.0).all(1)
    # by the definition of the neighbours (smallest (d2, index)): every copy's 8 neighbours are the 8
    # copies of lowest index, so every copy's neighbourhood is one point; the copies with at least
    # 8 copies of lower or equal index are among them. A point whose other seven neighbours are all
    # copies has two distinct points for a neighbourhood, a line (S[1] is the sums' rounding, 1e-19
    # here, not zero). No other point has a zero normal
    idx, d2 = pf.knn_brute(tgt, tgt, 8)
    copies = (d2 == 0.0).all(1)
    assert np.array_equal(np.flatnonzero(copies), where)
    assert zero[where[7:]].all()
    two = np.array([len(np.unique(tgt[r], axis=0)) == 2 for r in idx])
    assert np.array_equal(np.flatnonzero(two), [3, 560])
    assert np.array_equal(zero, copies | two)
    assert np.abs(np.linalg.norm(nrm[~zero], axis=1) - 1.0).max() <= 1e-14


def test_set_get_and_invalidation(icp, tgt):
    rng = np.random.default_rng(22)
    src = pf.pair(N)[1]
    nrm = rng.normal(size=(N, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[rng.choice(N, 50, replace=False)] = 0.0
    assert (np.abs(np.einsum("ni,ni->n", nrm, nrm) - 1.0) <= 1e-12)[nrm.any(1)].all()
    with icp.Context(0) as c:
        c.set_target(tgt)
        with pytest.raises(icp.IcpError) as e:
            c.get_target_normals()
        assert e.value.code == icp.ENOTREADY
        c.set_target_normals(nrm)
        assert c.get_target_normals().tobytes() == nrm.tobytes()  # caller's order, bit for bit
        # the device variants
        with c.to_device(nrm[::-1].copy()) as up, c.device_buffer(24 * N) as down:
            c.set_target_normals(up)
            c.get_target_normals(down)
            assert down.download(np.float64).tobytes() == nrm[::-1].tobytes()
        # a row that is neither of unit length nor zero: refused, the normals stay
        bad = nrm.copy()
        bad[17] = [0.6, 0.0, 0.7]
        with pytest.raises(icp.IcpError) as e:
            c.set_target_normals(bad)
        assert e.value.code == icp.EINVAL
        assert c.get_target_normals().tobytes() == nrm[::-1].tobytes()
        # set_target drops them
        c.set_source(src)
        st = c.iterate()
        c.plane_sums(st.centroid_src)
        c.set_target(tgt)
        c.iterate()
        for call in (c.get_target_normals, lambda: c.plane_sums(st.centroid_src)):
            with pytest.raises(icp.IcpError) as e:
                call()
            assert e.value.code == icp.ENOTREADY
