"""icp_hip_knn (knn_kernels.hip) against brute force: the k target points smallest under
(fl(d2), original index), fl(d2) = dx*dx + dy*dy + dz*dz in numpy's unfused fp64. Indices and d2
match bit for bit in every case: a blob, a lattice where every distance ties many times, copies
deeper than a leaf holds, a root that is a leaf, and a query far outside the root box."""
import numpy as np
import pytest

import plane_fixtures as pf

pytestmark = pytest.mark.gpu


def _same(got, want):
    gi, gd = got
    wi, wd = want
    assert gi.dtype == np.int32 and gd.dtype == np.float64
    assert np.array_equal(gi, wi), f"{np.count_nonzero(gi != wi)} indices differ"
    assert gd.tobytes() == wd.tobytes()


@pytest.fixture(scope="module")
def blob(icp):
    tgt, src, _ = icp.synth_pair(20000, 2049)  # 2049 queries: no multiple of any block size
    return tgt, src, pf.knn_brute(src, tgt, 32)  # the first k columns are the answer for every k <= 32


@pytest.fixture(scope="module")
def blob_ctx(icp, blob):
    with icp.Context(0) as ctx:
        ctx.set_target(blob[0])
        yield ctx


@pytest.mark.parametrize("k", [1, 7, 32])
def test_blob(blob, blob_ctx, k):
    _, q, (wi, wd) = blob
    _same(blob_ctx.knn(q, k), (wi[:, :k].copy(), wd[:, :k].copy()))


def test_k1_is_the_nearest_neighbour_search(blob, blob_ctx):
    tgt, q, (wi, wd) = blob
    assert (wd[:, 0] < wd[:, 1]).all()  # no ties on the blob: the two tie rules cannot differ
    idx, d = blob_ctx.nn(q)
    ki, kd2 = blob_ctx.knn(q, 1)
    assert np.array_equal(ki[:, 0], idx)
    assert np.sqrt(kd2[:, 0]).tobytes() == d.tobytes()


def test_device_variant(icp, blob, blob_ctx):
    _, q, _ = blob
    k, n = 7, len(q)
    hi, hd = blob_ctx.knn(q, k)
    d_q = blob_ctx.to_device(q)
    with blob_ctx.device_buffer(4 * n * k) as b_idx, blob_ctx.device_buffer(8 * n * k) as b_d2:
        blob_ctx.knn_device(d_q, n, k, b_idx, b_d2)
        assert b_idx.download(np.int32).tobytes() == hi.tobytes()
        assert b_d2.download(np.float64).tobytes() == hd.tobytes()
        assert d_q.download(np.float64).tobytes() == q.tobytes()  # inputs are never written
        # either output may be null
        b_idx.upload(np.zeros(n * k, np.int32))
        blob_ctx.knn_device(d_q, n, k, b_idx, None)
        assert b_idx.download(np.int32).tobytes() == hi.tobytes()
    d_q.free()
    with pytest.raises(icp.IcpError) as e:
        blob_ctx.knn_device(q.ctypes.data, n, k, None, None)  # host memory is not a device pointer
    assert e.value.code == icp.EINVAL


@pytest.mark.parametrize("cfg", [{"candidate_cache": 0}, {"search": 1}], ids=["no_cache", "reference_search"])
def test_search_configuration_does_not_matter(icp, blob, blob_ctx, cfg):
    """The k-NN goes through neither the candidate cache nor the 1-NN search kernels."""
    tgt, q, _ = blob
    want = blob_ctx.knn(q, 7)
    with icp.Context(0, cfg=cfg) as ctx:
        ctx.set_target(tgt)
        _same(ctx.knn(q, 7), want)


def test_lattice(icp):
    g = np.arange(16, dtype=np.float64)
    rng = np.random.default_rng(5)
    # the 16^3 integer lattice, shuffled: a point's index says nothing about where it lies
    tgt = rng.permutation(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    on = tgt[rng.choice(len(tgt), 512, replace=False)]
    centres = rng.integers(0, 15, size=(512, 3)) + 0.5
    q = np.concatenate([on, centres])
    want = pf.knn_brute(q, tgt, 16)
    assert (want[1][:, 15] == want[1][:, 14]).mean() > 0.5  # most queries tie across the k-th place
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        _same(ctx.knn(q, 16), want)


def test_copies_deeper_than_a_leaf(icp):
    rng = np.random.default_rng(7)
    tgt = rng.normal(size=(4000, 3))
    where = rng.choice(4000, 40, replace=False)
    tgt[where] = tgt[where[0]]  # 40 copies: one depth-20 leaf with more points than k
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        assert ctx.target_info()["max_depth"] == 20
        q = tgt[where]
        want = pf.knn_brute(q, tgt, 16)
        assert np.array_equal(want[0][0], np.sort(where)[:16]) and (want[1] == 0.0).all()
        _same(ctx.knn(q, 16), want)


def test_root_leaf_and_k_range(icp):
    tgt = np.random.default_rng(8).normal(size=(5, 3))
    q = np.random.default_rng(9).normal(size=(70, 3))
    with icp.Context(0) as ctx:
        with pytest.raises(icp.IcpError) as e:
            ctx.knn(q, 3)
        assert e.value.code == icp.ENOTREADY  # no target
        ctx.set_target(tgt)
        assert ctx.target_info()["n_nodes"] == 1
        _same(ctx.knn(q, 5), pf.knn_brute(q, tgt, 5))
        for k in (6, 0, -1, 33):
            with pytest.raises(icp.IcpError) as e:
                ctx.knn(q, k)
            assert e.value.code == icp.EINVAL, k


def test_far_query(blob, blob_ctx):
    tgt = blob[0]
    q = np.array([[1e6, 0.0, 0.0], [-3.0, 1e6, 2.0], [1e6, -1e6, 1e6], [0.1, 0.2, 0.3]])
    _same(blob_ctx.knn(q, 4), pf.knn_brute(q, tgt, 4))
