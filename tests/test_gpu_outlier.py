"""Outlier removal on the device (icp_hip_outlier_filter and its _device variant) against the numpy
statement of the definition (tests/outlier_reference.py): the scores byte for byte, mean and std
within the bounds of the device's reduction (derived in outlier_reference.py's docstring: shifted
sums over a fixed tree, the same form as stats_reference.py's), the kept set exactly, on the fixture
cloud and on the smallest shapes at which the kernels can go wrong; the interface's contract; and a
context whose target, normals and iterated source the call leaves alone.

The kept set is checked against the reported threshold with the mode's own comparison: score <=
threshold in the statistical mode, score == threshold (= k, the saturated count) in the radius mode."""
import numpy as np
import pytest

import outlier_reference as orf
import plane_fixtures as pf

pytestmark = pytest.mark.gpu

STAT, RAD = orf.STATISTICAL, orf.RADIUS


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _st(st):
    return (st.n, st.kept, st.mean, st.std, st.threshold)


def _einval(icp, call, text=None):
    with pytest.raises(icp.IcpError) as e:
        call()
    assert e.value.code == icp.EINVAL, str(e.value)
    if text:
        assert text in str(e.value), str(e.value)
    return e.value


def _check(got, xyz, ref, mode, label=""):
    """One call's outputs against the reference of the same cloud."""
    p, ix, score, st = got
    assert score.dtype == np.float64 and ix.dtype == np.int32
    diff = np.flatnonzero(score != ref["score"])
    assert _bits(score, ref["score"]), f"{label}: {len(diff)} scores differ, first at {diff[:5]}"
    orf.check_stats(st, ref, label)
    kept = score <= st.threshold if mode == STAT else score == st.threshold
    assert np.array_equal(ix, np.flatnonzero(kept)), label
    assert np.array_equal(kept, ref["kept"]), label
    assert st.kept == len(ix) == len(p) and (np.diff(ix) > 0).all(), label
    assert _bits(p, xyz[ix]), label
    if mode == RAD:
        assert st.threshold == ref["threshold"]


FIXTURE_CASES = [(STAT, 8, 1.0), (STAT, 16, 2.0), (RAD, 4, 0.15)]
FIXTURE_IDS = ["sor_k8", "sor_k16", "radius"]


@pytest.mark.parametrize("mode,k,param", FIXTURE_CASES, ids=FIXTURE_IDS)
def test_fixture_cloud(icp, gpu_ctx, mode, k, param):
    xyz, _ = orf.fixture_cloud()
    ref = orf.fixture_reference(mode, k, param)
    got = gpu_ctx.outlier_filter(xyz, mode, k, param)
    _check(got, xyz, ref, mode, "fixture")
    assert got[3].kept == {8: 6012, 16: 6035, 4: 5813}[k]
    again = gpu_ctx.outlier_filter(xyz, mode, k, param)  # two calls: the same bytes, stats included
    assert all(_bits(a, b) for a, b in zip(got[:3], again[:3])) and _st(got[3]) == _st(again[3])


@pytest.mark.parametrize("cfg", [{"candidate_cache": 0}, {"search": 1}], ids=["no_cache", "reference_search"])
def test_context_settings_do_not_show(icp, gpu_ctx, cfg):
    xyz, _ = orf.fixture_cloud()
    with icp.Context(0, cfg) as ctx:
        for mode, k, param in FIXTURE_CASES:
            want = gpu_ctx.outlier_filter(xyz, mode, k, param)
            got = ctx.outlier_filter(xyz, mode, k, param)
            assert all(_bits(a, b) for a, b in zip(got[:3], want[:3])) and _st(got[3]) == _st(want[3])


# ---- the smallest shapes at which the kernels can go wrong

def _blob(n, seed):
    return np.random.default_rng(seed).normal(size=(n, 3))


def _both(gpu_ctx, xyz, k, ratio, radius, kmin, label):
    ref = orf.reference(xyz, STAT, k, ratio)
    _check(gpu_ctx.outlier_filter(xyz, STAT, k, ratio), xyz, ref, STAT, label + " statistical")
    ref = orf.reference(xyz, RAD, kmin, radius)
    _check(gpu_ctx.outlier_filter(xyz, RAD, kmin, radius), xyz, ref, RAD, label + " radius")


def test_five_points_in_a_root_leaf(icp, gpu_ctx):
    xyz = _blob(5, 3)
    _both(gpu_ctx, xyz, 4, 0.5, 1.5, 4, "n=5")  # k = n - 1: every other point is a neighbour
    _both(gpu_ctx, xyz, 1, 0.0, 1.0, 1, "n=5 k=1")
    two = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])
    p, ix, score, st = gpu_ctx.outlier_filter(two, STAT, 1, 0.0)
    assert score.tolist() == [5.0, 5.0] and ix.tolist() == [0, 1] and st.std == 0.0 and st.threshold == 5.0


@pytest.mark.parametrize("n", [2049, 4097, 8193], ids=["n2049", "one_past_a_part", "one_past_two_parts"])
def test_block_and_part_boundaries(icp, gpu_ctx, n):
    _both(gpu_ctx, _blob(n, n), 8, 1.0, 0.25, 5, f"n={n}")


def test_copies_in_one_deep_leaf(icp, gpu_ctx):
    rng = np.random.default_rng(7)
    xyz = rng.normal(size=(4000, 3))
    where = rng.choice(4000, 40, replace=False)
    xyz[where] = xyz[where[0]]  # 40 copies: one depth-20 leaf with more points than k
    for k in (16, 32):
        ref = orf.reference(xyz, STAT, k, 1.0)
        assert (ref["score"][where] == 0.0).all()  # self is excluded by index: 39 copies remain
        _check(gpu_ctx.outlier_filter(xyz, STAT, k, 1.0), xyz, ref, STAT, f"copies k={k}")
    ref = orf.reference(xyz, RAD, 39, 1e-3)
    assert ref["kept"].sum() == 40
    _check(gpu_ctx.outlier_filter(xyz, RAD, 39, 1e-3), xyz, ref, RAD, "copies radius")
    assert gpu_ctx.outlier_filter(xyz, RAD, 40, 1e-3)[3].kept == 0


def test_identical_points(icp, gpu_ctx):
    xyz = np.tile([[1.25, -3.5, 7.0]], (100, 1))
    p, ix, score, st = gpu_ctx.outlier_filter(xyz, STAT, 8, 1.0)
    assert (score == 0.0).all() and st.mean == 0.0 and st.std == 0.0 and st.threshold == 0.0
    assert st.kept == 100 and ix.tolist() == list(range(100)) and _bits(p, xyz)
    p, ix, score, st = gpu_ctx.outlier_filter(xyz, RAD, 99, 0.5)
    assert (score == 99.0).all() and st.kept == 100 and st.std == 0.0 and st.mean == 99.0


def test_lattice_ties(icp, gpu_ctx):
    xyz, interior = orf.lattice8()
    # statistical, k = 6: the interior's score is exactly 1.0, the shell's three values lie above
    _check(gpu_ctx.outlier_filter(xyz, STAT, 6, 1.0), xyz, orf.reference(xyz, STAT, 6, 1.0), STAT, "lattice k=6")
    # k = 3, ratio 0: every point, the corners too, has three neighbours at exactly 1.0, so every
    # score equals the mean and the threshold: kept by <=
    s3 = gpu_ctx.outlier_filter(xyz, STAT, 3, 0.0)
    _check(s3, xyz, orf.reference(xyz, STAT, 3, 0.0), STAT, "lattice k=3")
    assert (s3[2] == 1.0).all() and s3[3].std == 0.0 and s3[3].threshold == 1.0 and s3[3].kept == 512
    # radius 1.0, min 6: d2 == r2 counts, the interior is kept; one ulp below nothing is
    got = gpu_ctx.outlier_filter(xyz, RAD, 6, 1.0)
    _check(got, xyz, orf.reference(xyz, RAD, 6, 1.0), RAD, "lattice radius 1")
    assert np.array_equal(got[1], np.flatnonzero(interior))
    below = float(np.nextafter(1.0, 0.0))
    got = gpu_ctx.outlier_filter(xyz, RAD, 6, below)
    _check(got, xyz, orf.reference(xyz, RAD, 6, below), RAD, "lattice radius below 1")
    assert got[3].kept == 0 and (got[2] == 0.0).all()


def test_one_point_far_away(icp, gpu_ctx):
    xyz = _blob(2001, 5)
    xyz[777] = [1e6, -1e6, 1e6]
    ref = orf.reference(xyz, STAT, 8, 1.0)
    got = gpu_ctx.outlier_filter(xyz, STAT, 8, 1.0)
    _check(got, xyz, ref, STAT, "far point")
    assert 777 not in got[1] and got[2][777] == ref["score"][777] > 1e6


def test_georeferenced_offset(icp, gpu_ctx):
    xyz = np.ascontiguousarray(orf.fixture_cloud()[0] + [4.5e5, 5.4e6, 300.0])
    ref = orf.reference(xyz, STAT, 8, 1.0)
    _check(gpu_ctx.outlier_filter(xyz, STAT, 8, 1.0), xyz, ref, STAT, "shifted")
    ref = orf.reference(xyz, RAD, 4, 0.15)
    _check(gpu_ctx.outlier_filter(xyz, RAD, 4, 0.15), xyz, ref, RAD, "shifted radius")


def test_k32(icp, gpu_ctx):
    xyz, _ = orf.fixture_cloud()
    assert icp.KNN_MAX == 32
    _check(gpu_ctx.outlier_filter(xyz, STAT, 32, 1.5), xyz, orf.reference(xyz, STAT, 32, 1.5), STAT, "k=32")


def test_radius_counts_past_the_list_limit(icp, gpu_ctx):
    """k = 200 neighbours wanted within a radius that holds about 50: no list, no saturation."""
    xyz, injected = orf.fixture_cloud()
    ref = orf.reference(xyz, RAD, 200, 0.36)
    med = float(np.median(ref["score"][~injected]))
    assert 25 <= med <= 100 and ref["score"].max() < 200
    got = gpu_ctx.outlier_filter(xyz, RAD, 200, 0.36)
    _check(got, xyz, ref, RAD, "k=200")
    assert got[3].kept == 0 and got[3].threshold == 200.0


# ---- the interface

@pytest.fixture(scope="module")
def dev_case(icp, gpu_ctx):
    xyz, _ = orf.fixture_cloud()
    want = gpu_ctx.outlier_filter(xyz, STAT, 8, 1.0)
    buf = gpu_ctx.to_device(xyz)
    yield xyz, want, buf
    buf.free()


def test_capacity_too_small(icp, gpu_ctx, dev_case):
    xyz, (p, ix, score, st), buf = dev_case
    n, m = len(xyz), len(ix)
    e = _einval(icp, lambda: gpu_ctx.outlier_filter(xyz, STAT, 8, 1.0, cap=m - 1), "capacity")
    assert e.m == m
    dp, di, ds = gpu_ctx.device_buffer(24 * m), gpu_ctx.device_buffer(4 * m), gpu_ctx.device_buffer(8 * n)
    for b in (dp, di, ds):
        b.upload(np.full(b.nbytes, 0xA5, np.uint8))
    e = _einval(icp, lambda: gpu_ctx.outlier_filter_device(buf, n, STAT, 8, 1.0, cap=m - 1, d_xyz_out=dp, d_index_out=di,
                                                           d_score_out=ds), "capacity")
    assert e.m == m
    for b in (dp, di, ds):
        assert (b.download(np.uint8) == 0xA5).all()  # untouched
        b.free()
    got = gpu_ctx.outlier_filter(xyz, STAT, 8, 1.0, cap=m)  # exactly enough
    assert _bits(got[1], ix)


def test_counts_only(icp, gpu_ctx, dev_case):
    xyz, (p, ix, score, st), buf = dev_case
    m, got = gpu_ctx.outlier_filter_device(buf, len(xyz), STAT, 8, 1.0)  # all outputs null, whatever cap says
    assert m == len(ix) and _st(got) == _st(st)
    import ctypes as C
    mm = C.c_int64(0)
    rc = icp.lib().icp_hip_outlier_filter(gpu_ctx.handle, xyz.ctypes.data_as(C.c_void_p), len(xyz), RAD, 4, 0.15, 0,
                                          None, None, None, C.byref(mm), None)  # the host call, stats null too
    assert rc == 0 and mm.value == 5813


def test_device_variant_matches_the_host_variant(icp, gpu_ctx, dev_case):
    xyz, (p, ix, score, st), buf = dev_case
    n, m = len(xyz), len(ix)
    cap = m + 5
    dp, di, ds = gpu_ctx.device_buffer(24 * cap), gpu_ctx.device_buffer(4 * cap), gpu_ctx.device_buffer(8 * n)
    for b in (dp, di):
        b.upload(np.full(b.nbytes, 0xA5, np.uint8))
    got_m, got_st = gpu_ctx.outlier_filter_device(buf, n, STAT, 8, 1.0, cap=cap, d_xyz_out=dp, d_index_out=di,
                                                  d_score_out=ds)
    assert got_m == m and _st(got_st) == _st(st)
    assert _bits(dp.download(np.float64, (cap, 3))[:m], p) and _bits(di.download(np.int32)[:m], ix)
    assert _bits(ds.download(np.float64), score)
    assert (dp.download(np.uint8)[24 * m:] == 0xA5).all() and (di.download(np.uint8)[4 * m:] == 0xA5).all()
    assert _bits(buf.download(np.float64, (n, 3)), xyz)  # the input is never written
    # single outputs
    assert gpu_ctx.outlier_filter_device(buf, n, RAD, 4, 0.15, cap=cap, d_index_out=di)[0] == 5813
    assert _bits(di.download(np.int32)[:5813], gpu_ctx.outlier_filter(xyz, RAD, 4, 0.15)[1])
    for b in (dp, di, ds):
        b.free()


def test_host_pointers_are_refused(icp, gpu_ctx, dev_case):
    xyz, (p, ix, score, st), buf = dev_case
    n, m = len(xyz), len(ix)
    host3, hosti, hosts = np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros(n)
    _einval(icp, lambda: gpu_ctx.outlier_filter_device(xyz.ctypes.data, n, STAT, 8, 1.0))
    _einval(icp, lambda: gpu_ctx.outlier_filter_device(buf, n, STAT, 8, 1.0, cap=n, d_xyz_out=host3.ctypes.data))
    _einval(icp, lambda: gpu_ctx.outlier_filter_device(buf, n, STAT, 8, 1.0, cap=n, d_index_out=hosti.ctypes.data))
    _einval(icp, lambda: gpu_ctx.outlier_filter_device(buf, n, STAT, 8, 1.0, d_score_out=hosts.ctypes.data))
    _einval(icp, lambda: gpu_ctx.outlier_filter_device(buf.ptr + 4, n - 1, STAT, 8, 1.0))  # not 8-byte aligned
    _einval(icp, lambda: gpu_ctx.outlier_filter_device(None, n, STAT, 8, 1.0))
    assert not host3.any() and not hosti.any() and not hosts.any()


def test_argument_errors(icp, gpu_ctx):
    xyz = _blob(50, 9)
    f = gpu_ctx.outlier_filter
    _einval(icp, lambda: f(xyz[:1], STAT, 1, 1.0))                      # n < 2
    _einval(icp, lambda: f(np.empty((0, 3)), RAD, 1, 1.0))
    for k in (0, -1, 33, 50):
        _einval(icp, lambda: f(xyz, STAT, k, 1.0))                      # k out of [1, min(32, n - 1)]
    _einval(icp, lambda: f(xyz[:10], STAT, 10, 1.0))                    # k > n - 1
    assert f(xyz[:10], STAT, 9, 1.0)[3].n == 10
    for k in (0, -3, 50):
        _einval(icp, lambda: f(xyz, RAD, k, 1.0))                       # k out of [1, n - 1]
    assert f(xyz, RAD, 49, 100.0)[3].kept == 50                        # no list limit in the radius mode
    for r in (float("nan"), float("inf"), -float("inf")):
        _einval(icp, lambda: f(xyz, STAT, 4, r))                        # std_ratio not finite
    assert f(xyz, STAT, 4, -1.0)[3].n == 50                             # any finite ratio
    for r in (0.0, -1.0, float("nan"), float("inf")):
        _einval(icp, lambda: f(xyz, RAD, 4, r))                         # radius not finite or <= 0
    for mode in (2, -1):
        _einval(icp, lambda: f(xyz, mode, 4, 1.0), "mode")
    bad = xyz.copy()
    bad[3, 1] = np.nan
    _einval(icp, lambda: f(bad, STAT, 4, 1.0))                          # a non-finite coordinate
    bad[3, 1] = np.inf
    _einval(icp, lambda: f(bad, RAD, 4, 1.0))


def test_multi_device_context_answers_as_a_plain_one(icp, gpu_ctx, dev_case):
    xyz, want, _ = dev_case
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as ctx:
        got = ctx.outlier_filter(xyz, STAT, 8, 1.0)
        assert all(_bits(a, b) for a, b in zip(got[:3], want[:3])) and _st(got[3]) == _st(want[3])
        m, n = len(want[1]), len(xyz)
        buf, dp, ds = ctx.to_device(xyz), ctx.device_buffer(24 * m), ctx.device_buffer(8 * n)
        assert ctx.outlier_filter_device(buf, n, STAT, 8, 1.0, cap=m, d_xyz_out=dp, d_score_out=ds)[0] == m
        assert _bits(dp.download(np.float64, (m, 3)), want[0]) and _bits(ds.download(np.float64), want[2])
        for b in (buf, dp, ds):
            b.free()


# ---- the context is untouched

def test_the_context_is_untouched(icp):
    tgt, src, _ = pf.pair(6000)
    xyz, _ = orf.fixture_cloud()
    with icp.Context(0) as ctx:
        with pytest.raises(icp.IcpError) as e:
            ctx.outlier_last_timing()
        assert e.value.code == icp.ENOTREADY
        ctx.set_target(tgt)
        ctx.estimate_target_normals(16)
        ctx.set_source(src)
        st = ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)
        ctx.iterate(icp.best_fit_from_stats(st), 1, icp.RULES_ENGINE, 3.0)

        def state():
            return (*ctx.nn(xyz[:500]), *ctx.get_correspondences(), ctx.get_target_normals(), ctx.get_source())

        before, info = state(), ctx.target_info()
        for mode, k, param in FIXTURE_CASES:
            got = ctx.outlier_filter(xyz, mode, k, param)
            assert _bits(got[2], orf.fixture_reference(mode, k, param)["score"])
        after = state()
        assert all(_bits(a, b) for a, b in zip(before, after)) and ctx.target_info() == info
        ms = ctx.outlier_last_timing()
        assert ms.shape == (4,) and (ms >= 0.0).all() and ms[0] > 0.0 and ms[1] > 0.0
        st2 = ctx.iterate(None, 2, icp.RULES_ENGINE, 3.0)  # and the context still iterates
        assert st2.n == len(src)


def test_module_level_call(icp, gpu_ctx, dev_case):
    xyz, want, _ = dev_case
    got = icp.outlier_filter(xyz, icp.OUTLIER_STATISTICAL, 8, 1.0)
    assert all(_bits(a, b) for a, b in zip(got[:3], want[:3])) and _st(got[3]) == _st(want[3])
