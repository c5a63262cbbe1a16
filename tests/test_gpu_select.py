"""icp_hip_residual_select on the GPU (reject_kernels.hip): the value bit-equal to numpy.partition
over the finite residuals the context itself reports, the rank and the three counts equal to the
reference's; at the shapes of the statistics tests, on residual sets that exercise the key's digits
one at a time, with non-finite rows, twice in a row and on contexts that search differently, and every
refusal of the contract."""
import numpy as np
import pytest

import reject_fixtures as rf
import stats_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(icp):
    """A context holding the 5000-point target of stats_reference.shape_pair."""
    with icp.Context(0) as c:
        c.set_target(R.shape_pair(1, 5000)[0])
        yield c


@pytest.fixture(scope="module")
def lat(icp):
    """A context holding stats_reference.lattice(17)."""
    with icp.Context(0) as c:
        c.set_target(R.lattice(17))
        yield c


def _residuals(c, src):
    c.set_source(src)
    c.iterate()
    return c.get_correspondences()[1]


@pytest.mark.parametrize("n", R.SHAPE_SOURCES)
def test_shapes(icp, ctx, n):
    d = _residuals(ctx, R.shape_pair(n, 5000)[1])
    assert np.isfinite(d).all()
    for rank in sorted({r for r in (1, 2, n // 2, n - 1, n) if 1 <= r <= n}):
        rf.check_select(ctx.residual_select(rank=rank), d, rank, f"n {n}")
        rf.check_select(ctx.residual_select(fraction=float("nan"), rank=rank), d, rank, f"n {n}: fraction ignored")
    for f in (0.5, 1.0):
        rf.check_select(ctx.residual_select(fraction=f), d, icp.trim_rank(f, n), f"n {n} fraction {f}")
    assert ctx.residual_select(fraction=1.0).value == d.max()
    assert ctx.residual_select(rank=1).value == d.min()


def test_every_rank_at_257(icp, ctx):
    d = _residuals(ctx, R.shape_pair(257, 5000)[1])
    s = np.sort(d)
    for rank in range(1, 258):
        got = ctx.residual_select(rank=rank)
        assert got.value == s[rank - 1] and got.rank == rank and got.n_finite == 257
        assert got.n_less <= rank - 1 < got.n_less + got.n_equal


@pytest.mark.parametrize("kind", ["constant", "zero", "near"])
@pytest.mark.parametrize("n", R.DEGENERATE_SOURCES)
def test_degenerate_residuals(icp, lat, kind, n):
    d = _residuals(lat, R.degenerate_case(kind, n)[1])
    for rank in rf.boundary_ranks(d) + [n // 2]:
        rf.check_select(lat.residual_select(rank=rank), d, rank, f"{kind} {n}")
    got = lat.residual_select(fraction=0.5)
    if kind == "constant":
        assert (got.value, got.n_less, got.n_equal) == (0.5, 0, n)
    if kind == "zero":
        assert np.float64(got.value).tobytes() == np.float64(0.0).tobytes() and got.n_equal == n
    if kind == "near":
        assert len(np.unique(d)) == 3 and got.n_equal < n


@pytest.mark.parametrize("name", sorted(rf.select_sets()))
def test_constructed_residuals(icp, lat, name):
    """Low bits only, 41 binades, two values and a lone smaller one: ranks on both sides of every
    boundary between equal runs (of up to 64 boundaries)."""
    r = rf.select_sets()[name]
    d = _residuals(lat, R.lattice_queries(R.lattice(17), r))
    n = len(d)
    assert len(np.unique(d)) >= 3
    for rank in rf.boundary_ranks(d):
        rf.check_select(lat.residual_select(rank=rank), d, rank, name)
    for f in (0.5, 1.0):
        rf.check_select(lat.residual_select(fraction=f), d, icp.trim_rank(f, n), name)
    if name == "two_values_and_one":
        got = lat.residual_select(rank=1)
        assert (got.value, got.n_less, got.n_equal) == (0.125, 0, 1)
        got = lat.residual_select(rank=2)
        assert got.n_less == 1 and got.n_equal == n // 3 - 1


@pytest.mark.parametrize("n", R.DEGENERATE_SOURCES)
def test_non_finite_rows_are_not_ranked(icp, lat, n):
    d = _residuals(lat, R.degenerate_case("nan", n)[1])
    assert int(np.isfinite(d).sum()) == n - 3
    for rank in (1, n - 4, n - 3):
        rf.check_select(lat.residual_select(rank=rank), d, rank, f"nan {n}")
    got = lat.residual_select(fraction=1.0)
    assert got.rank == n - 3 and got.n_finite == n - 3
    with pytest.raises(icp.IcpError) as e:
        lat.residual_select(rank=n - 2)
    assert e.value.code == icp.EINVAL and e.value.n_finite == n - 3


def test_no_finite_residual(icp, lat):
    src = np.full((3, 3), np.nan)
    src[1] = np.inf
    d = _residuals(lat, src)
    assert not np.isfinite(d).any()
    for kw in ({"rank": 1}, {"fraction": 0.5}):
        with pytest.raises(icp.IcpError) as e:
            lat.residual_select(**kw)
        assert e.value.code == icp.EINVAL and e.value.n_finite == 0


def test_repeats_and_other_search_paths(icp, ctx):
    tgt, src = R.shape_pair(16385, 5000)
    _residuals(ctx, src)
    calls = [{"fraction": 0.5}, {"rank": 1}, {"rank": 16385}, {"rank": 777}]
    first = [bytes(ctx.residual_select(**kw)) for kw in calls]
    assert [bytes(ctx.residual_select(**kw)) for kw in calls] == first
    for cfg in ({"candidate_cache": 0}, {"scan_groups": 1}):
        with icp.Context(0, cfg=cfg) as other:
            other.set_target(tgt)
            _residuals(other, src)
            assert [bytes(other.residual_select(**kw)) for kw in calls] == first, cfg


def test_the_iterate_is_left_as_it_was(icp, ctx):
    src = R.shape_pair(4097, 5000)[1]
    _residuals(ctx, src)
    idx, d = ctx.get_correspondences()
    moved = ctx.get_source()
    ctx.residual_select(fraction=0.5)
    idx2, d2 = ctx.get_correspondences()
    assert idx2.tobytes() == idx.tobytes() and d2.tobytes() == d.tobytes()
    assert ctx.get_source().tobytes() == moved.tobytes()


def test_argument_errors(icp):
    tgt, src = R.shape_pair(65, 5000)
    with icp.Context(0) as c:
        for kw in ({"rank": -1}, {"fraction": 0.0}, {"fraction": 1.5}, {"fraction": -0.5}, {"fraction": float("nan")}):
            with pytest.raises(icp.IcpError) as e:
                c.residual_select(**kw)
            assert e.value.code == icp.EINVAL, kw
        with pytest.raises(icp.IcpError) as e:
            c.residual_select(fraction=0.5)
        assert e.value.code == icp.ENOTREADY  # no target
        c.set_target(tgt)
        c.set_source(src)
        with pytest.raises(icp.IcpError) as e:
            c.residual_select(fraction=0.5)
        assert e.value.code == icp.ENOTREADY  # no iterate on this source
        c.iterate()
        assert c.residual_select(fraction=0.5).rank == 32
        c.set_source(src)
        with pytest.raises(icp.IcpError) as e:
            c.residual_select(rank=1)
        assert e.value.code == icp.ENOTREADY  # a new source
        c.comm_init_host(2, 0, lambda local: np.stack([local, local]))
        c.iterate()
        with pytest.raises(icp.IcpError) as e:
            c.residual_select(fraction=0.5)
        assert e.value.code == icp.EINVAL and "communicator" in str(e.value)
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as g:
        g.set_target(tgt)
        g.set_source(src)
        g.iterate()
        with pytest.raises(icp.IcpError) as e:
            g.residual_select(fraction=0.5)
        assert e.value.code == icp.EINVAL and "multi-device" in str(e.value)
