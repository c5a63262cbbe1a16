"""What test_gpu_geo_search.py relies on, proven on the CPU at every offset of geo_fixtures.OFFSETS:

  * which fixtures are shiftable (geo_fixtures.SHIFTABLE, and no other), and that the octree of a
    shiftable fixture keeps its structure while its boxes do not shift exactly (tree_shift);
  * every pre-check of the fixtures at every offset: the near tie's two gaps, the follow-lists
    clouds' overflowing waves and halves, the ball chain's (a) to (d), the flat shell's rounds;
  * the oracle's nn() under both rule sets against the numpy brute force, index and residual bits,
    at every query outside the 2^-48 window;
  * the count of queries inside the window, per fixture and offset, against the cap of
    geo_fixtures.tie_cap (measured: 0 on every fixture at every offset);
  * for the shiftable fixtures, the oracle's answers at the offsets are the origin's bits.
"""
import numpy as np
import pytest

import ball_fixtures as bf
import geo_fixtures as gf
import test_gpu_ball_chain as chain
import test_gpu_follow_lists as follow_lists


@pytest.mark.parametrize("name", gf.SEARCH_FIXTURES)
def test_which_fixtures_shift(icp, name):
    tgt, src, mp, md = gf.clouds(icp, name, "origin")
    assert gf.shiftable(tgt, src) == (name in gf.SHIFTABLE)
    if name in gf.SHIFTABLE:
        for where in gf.PLACES:
            t, s, _, _ = gf.clouds(icp, name, where)
            assert (t - gf.OFFSETS[where]).tobytes() == tgt.tobytes() and (s - gf.OFFSETS[where]).tobytes() == src.tobytes()
        boxes, structure = gf.tree_shift(icp, tgt, mp, md)
        assert structure and not boxes  # the root box's 0.001 is on no grid: see tree_shift


def test_shiftable_predicate():
    grid = np.round(np.random.default_rng(3).uniform(-4, 4, (100, 3)) / gf.GRID) * gf.GRID
    assert gf.exactly_shiftable(grid)
    assert not gf.exactly_shiftable(grid + bf.CLUSTER_STEP)  # 2^-44: below the fp64 ulp at 5e6
    assert not gf.exactly_shiftable(np.random.default_rng(4).uniform(-4, 4, (100, 3)))


@pytest.mark.parametrize("where", gf.PLACES)
@pytest.mark.parametrize("name", gf.SEARCH_FIXTURES)
def test_oracle_equals_brute_force(icp, oracle, name, where):
    tgt, src, mp, md = gf.clouds(icp, name, where)
    bidx, bd, tie = gf.brute(tgt, src)
    print(f"{name} at {where}: {int(tie.sum())} of {len(src)} queries inside the tie window")
    assert tie.sum() <= gf.tie_cap(name) * len(src)
    tree = oracle.OracleTree(tgt, mp, md)
    for init in (oracle.DBL_MAX, 1e20):  # engine and CLI rules
        oidx, od = tree.nn(src, init_best=init)
        np.testing.assert_array_equal(oidx[~tie], bidx[~tie])
        np.testing.assert_array_equal(od[~tie], bd[~tie])


@pytest.mark.parametrize("name", gf.SHIFTABLE)
def test_oracle_is_translation_invariant_on_shiftable_fixtures(icp, oracle, name):
    answers = []
    for where in gf.PLACES:
        tgt, src, mp, md = gf.clouds(icp, name, where)
        answers.append(oracle.OracleTree(tgt, mp, md).nn(src, init_best=oracle.DBL_MAX))
    for idx, d in answers[1:]:
        np.testing.assert_array_equal(idx, answers[0][0])
        np.testing.assert_array_equal(d, answers[0][1])


@pytest.mark.parametrize("where", gf.PLACES)
def test_near_tie_gaps(where):
    info = gf.check_near_tie(*gf.near_tie(where))
    print(where, info)
    assert info["min_rel_gap"] > 2.0 ** -38 > 512 * gf.WINDOW and info["max_gap_over_e_abs"] < 0.125


@pytest.mark.parametrize("where", gf.PLACES)
def test_near_tie_close_gaps(icp, where):
    tgt, q = gf.near_tie_close(where)
    ext = gf.wave_ext_floor(icp, q)
    info = gf.check_near_tie(tgt, q, ext)
    print(where, info, "ext floor", ext.min(), "nearest", gf.CLOSE_D)
    assert info["min_rel_gap"] > 2.0 ** -38 > 512 * gf.WINDOW and info["max_gap_over_e_abs"] < 0.125
    # the key's cleared bits (up to 2^-19 of the distance) are below a tenth of e_abs in every wave
    assert 2.0 ** -19 * 1.01 * gf.CLOSE_D < 0.1 * gf.scan32_e_abs(ext.min())


@pytest.mark.parametrize("where", gf.PLACES)
@pytest.mark.parametrize("n", bf.SIZES)
def test_follow_lists_waves_and_halves_overflow(icp, n, where):
    tgt, src = gf.follow(n, where)
    follow_lists._assert_buckets_overflow(icp, tgt, src)


@pytest.mark.parametrize("where", gf.PLACES)
@pytest.mark.parametrize("name,n", [(name, n) for name in gf.BALL_NAMES for n in bf.SIZES])
def test_ball_chain_prechecks(icp, name, n, where):
    tgt, src, mp, md = gf.ball(name, n, where)
    info = chain._precheck(icp, "shell" if name == "shell_grid" else name, n, tgt, src, gf.ball_model(icp, name, where))
    print(name, n, where, info)


def test_deep_shell_stays_at_the_origin():
    """Twelve points CLUSTER_STEP apart are one point at every offset: the deep trees that
    shell_deep20 / shell_deep40 are for do not exist there (the precondition that drops them)."""
    tgt = bf.shell_deep_target()
    for where in gf.PLACES[1:]:
        assert len(np.unique(tgt + gf.OFFSETS[where], axis=0)) < len(tgt)
