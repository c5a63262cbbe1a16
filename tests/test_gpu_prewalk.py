"""The prewalk of the candidate cache (icp_hip_set_prewalk; k_prewalk_filter + k_wave_prewalk on the
context's second stream): records refreshed between two searches change which waves walk, never a
result. Every case compares a run with the prewalk against the same run without it, bit for bit,
and against the CPU oracle's octree NN where the case states it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 100_000
ITERS = 12
LOOK = 2.0


def _registration(icp, ctx, src, look, iters=ITERS, counters=False):
    """`iters` host-driven iterates of the plain ICP loop; per iterate (idx, dist[, counters])."""
    ctx.set_source(src)
    ctx.set_prewalk(look)
    out, T = [], None
    for k in range(iters):
        st = ctx.iterate(T, k, icp.RULES_ENGINE, 3.0)
        idx, d = ctx.get_correspondences()
        out.append((idx, d, ctx.debug_counters() if counters else None))
        T = icp.best_fit_from_stats(st)
    return out


@pytest.fixture(scope="module")
def pair(icp):
    tgt, src, _ = icp.synth_pair(N, yaw_deg=3.0)
    return tgt, src


@pytest.fixture(scope="module")
def runs(icp, pair):
    """The 12-iterate registration with debug counters, prewalk on and off, and the moved source
    the on-run ends with."""
    tgt, src = pair
    with icp.Context(0, {"debug_counters": 1}) as ctx:
        ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
        on = _registration(icp, ctx, src, LOOK, counters=True)
        moved = ctx.get_source()
        off = _registration(icp, ctx, src, 0.0, counters=True)
    return on, off, moved


def test_registration_bit_identical_and_oracle(icp, oracle, pair, runs):
    on, off, moved = runs
    for k, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a[0], b[0]), f"iterate {k}: idx differs with the prewalk"
        assert np.array_equal(a[1], b[1]), f"iterate {k}: dist differs with the prewalk"
    oidx, od = oracle.OracleTree(pair[0]).nn(moved, init_best=oracle.DBL_MAX)
    assert np.array_equal(on[-1][0], oidx) and np.array_equal(on[-1][1], od)


def test_prewalk_replaces_walks(runs):
    on, off, _ = runs
    moved_off = sum(c["walk_moved"] for _, _, c in off[2:])
    moved_on = sum(c["walk_moved"] for _, _, c in on[2:])
    stores = sum(c["prewalk_stores"] for _, _, c in on[2:])
    print(f"walk_moved off {moved_off} on {moved_on} prewalk_stores {stores}")
    assert moved_off >= 300, "the case does not re-walk: the test would pass vacuously"
    assert moved_on < moved_off
    assert stores > 0
    assert all(c["prewalk_stores"] == 0 for _, _, c in off)


def test_invalidation_with_a_prewalk_pending(icp, pair):
    """set_source with another cloud, set_target and close() directly after an iterate that ran a
    prewalk (look-ahead 64: every reusing wave asks, the longest prewalk this source gives), with
    no call in between that waits for the device: the prewalk may still be running on the side
    stream. The results after each equal a fresh context's."""
    tgt, src = pair
    tgt2, src2, _ = icp.synth_pair(30_000, yaw_deg=1.0, seed_target=7, seed_source=8)

    def iterates(ctx, k):
        """k iterates and nothing else: the last call is an iterate whose prewalk may still run"""
        T = None
        for j in range(k):
            T = icp.best_fit_from_stats(ctx.iterate(T, j, icp.RULES_ENGINE, 3.0))

    def fresh(target):
        with icp.Context(0) as ctx:
            ctx.set_target(target, 10, 20, icp.RULES_ENGINE)
            ctx.set_source(src2)
            ctx.set_prewalk(64.0)
            iterates(ctx, 3)
            return ctx.get_correspondences()

    with icp.Context(0) as ctx:
        ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
        ctx.set_source(src)
        ctx.set_prewalk(64.0)
        iterates(ctx, 4)
        ctx.set_source(src2)  # directly after an iterate
        iterates(ctx, 3)
        a = ctx.get_correspondences()
        ctx.set_source(src)
        iterates(ctx, 4)
        ctx.set_target(tgt2, 10, 20, icp.RULES_ENGINE)  # directly after an iterate
        ctx.set_source(src2)
        iterates(ctx, 3)
        b = ctx.get_correspondences()
        ctx.set_source(src)
        iterates(ctx, 4)
        # the context closes directly after an iterate
    ctx = icp.Context(0)
    ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
    ctx.set_source(src)
    ctx.set_prewalk(64.0)
    iterates(ctx, 4)
    ctx.close()  # a context that only iterated, closed directly after its last iterate
    for x, y in ((a, fresh(tgt)), (b, fresh(tgt2))):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def test_more_requests_than_the_list_takes(icp, oracle, pair):
    """A large explicit transform every iterate and the longest look-ahead: every reusing wave
    asks, more than the list's cap (an eighth of the waves); the rest walk in the search."""
    tgt, src = pair
    a = np.deg2rad(0.3)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = [0.02, -0.01, 0.005]
    cap = max(64, ((N + 63) // 64) // 8)
    tree = oracle.OracleTree(tgt)
    with icp.Context(0, {"debug_counters": 1}) as ctx:
        ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
        ctx.set_source(src)
        ctx.set_prewalk(64.0)
        hits, stores = [], []
        for k in range(6):
            ctx.iterate(T if k else None, k, icp.RULES_ENGINE, 3.0)
            c = ctx.debug_counters()
            hits.append(c["cache_hits"])
            stores.append(c["prewalk_stores"])
            if k in (3, 5):
                idx, d = ctx.get_correspondences()
                oidx, od = tree.nn(ctx.get_source(), init_best=oracle.DBL_MAX)
                assert np.array_equal(idx, oidx) and np.array_equal(d, od), f"iterate {k}"
    print(f"cap {cap} cache_hits {hits} prewalk_stores {stores}")
    assert max(hits[2:]) > cap, "fewer reusing waves than the cap: nothing was dropped"
    assert 0 < max(stores) <= cap


def test_prewalk_overflow_retries_and_matches_oracle(icp, oracle):
    """Prewalks whose B+ overflows. 30000 target points and 4096 queries inside a 1 cm cube: a
    wave's box (a kd bucket of 64 queries, ~1/64 of the cube, plus its balls) holds ~700 of them
    and its B+ with the margin alone ~850, below the 1008 a record takes. The records are stored
    under a motion of 1e-7 (no lead to speak of); then every iterate moves the queries by 3e-5 per
    axis, about 1 % of a box: the boxes stay inside their records (every reusing wave asks,
    look-ahead 64), while the B+ of a prewalk, led by 8 x 3e-5 per axis, holds ~1.5 x the box:
    it overflows and walks again with a quarter of the margin and the lead (counted); one that
    still overflows leaves the old record (counted: the denser waves, whose box alone holds
    nearly 1008). Every iterate
    equals the oracle."""
    rng = np.random.default_rng(5)
    tgt, src, _ = icp.synth_pair(20_000, yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0, t=(0.0, 0.0, 0.0))
    tgt = np.vstack([tgt, rng.uniform(0.0, 0.01, (30_000, 3))])
    src = np.vstack([src, rng.uniform(0.001, 0.009, (4096, 3))])
    tree = oracle.OracleTree(tgt)
    stores = retries = kept = 0
    with icp.Context(0, {"debug_counters": 1}) as ctx:
        ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
        ctx.set_source(src)
        ctx.set_prewalk(64.0)
        for k in range(7):
            T = np.eye(4)
            T[:3, 3] = (1e-7 if k < 2 else 3e-5) * np.array([1.0, 1.0, -1.0])
            ctx.iterate(T if k else None, k, icp.RULES_ENGINE, 3.0)
            c = ctx.debug_counters()
            stores += c["prewalk_stores"]
            retries += c["prewalk_retries"]
            kept += c["prewalk_kept_old"]
            idx, d = ctx.get_correspondences()
            oidx, od = tree.nn(ctx.get_source(), init_best=oracle.DBL_MAX)
            assert np.array_equal(idx, oidx) and np.array_equal(d, od), f"iterate {k}"
    print(f"prewalk_stores {stores} prewalk_retries {retries} prewalk_kept_old {kept}")
    assert stores > 0
    assert retries > 0, "no prewalk overflowed: the case misses what it is for"
    assert kept > 0, "no prewalk overflowed twice: the old-record exit was not reached"


def _session_steps(icp, ctx, tgt, src, look, steps, batch=False):
    ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
    ctx.set_source(src)
    ctx.set_prewalk(look)
    sess = ctx.session(icp.params_default(max_iterations=steps + 1, tolerance=1e-6, flags=icp.FLAG_NO_EARLY_STOP))
    out = []
    if batch:
        assert sess.step_n(steps) == steps
        out.append(ctx.get_correspondences())
    else:
        for _ in range(steps):
            assert sess.step() is not None
            out.append(ctx.get_correspondences())
    out.append((sess.transform().copy(), ctx.get_source()))
    sess.close()
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


@pytest.mark.parametrize("kind", ["host_group_of_2", "rccl_one_rank"])
def test_multi_rank_on_equals_off(icp, pair, kind):
    tgt, src = pair

    def run(look):
        ctx = icp.Context(devices=[0, 0]) if kind == "host_group_of_2" else icp.Context(0)
        with ctx:
            if kind == "rccl_one_rank":
                ctx.comm_init(1, 0, icp.Context.unique_id())
            return _session_steps(icp, ctx, tgt, src, look, 8)

    _same(run(LOOK), run(0.0))


def test_device_loop_on_equals_off(icp, pair):
    """Iterates of the device-resident loop never prewalk (the session step overwrites the transform
    the prewalk would read): the setting changes nothing there."""
    tgt, src = pair

    def run(look):
        with icp.Context(0, icp.config(device_loop=1)) as ctx:
            return _session_steps(icp, ctx, tgt, src, look, 12, batch=True)

    _same(run(LOOK), run(0.0))
