"""The certified search at georeferenced coordinates, path by path (geo_fixtures.py: the clouds, the
offsets and the CPU checks; test_geo_fixtures.py proves on the CPU what is relied on here).

Every rounding term of the search (ball_radius32's amax 2^-44, box_lo / box_hi's |b| 2^-52, the fp32
frames of the staged points, the queries and the cache entries, k_prewalk_filter's rebuilt box,
certify_prev's fp32 separation) is ~1e-13 for a cloud at the origin and up to 1e-9 m (fp64) or 0.5 m
(fp32) at the offsets. Each test runs at the origin (the control), geo (4e5, 5e6, 100), far
(-7.3e6, 2.1e6, -40) and ecef (-2.7e6, -4.3e6, 3.85e6: a large z as well).

Every comparison is of indices and residual bits (assert_array_equal), at every step and for every
query, against the CPU oracle's nn() at that place; transforms are fitted once (by the
reference-order context) and handed to every context under test, so the moved sources are the same
bits everywhere. A path test also proves from the debug counters that its path ran, by a counter > 0
or == a value derived on the CPU. The shiftable fixtures (geo_fixtures.SHIFTABLE) must in addition
return the origin's bits on their untransformed steps. Every context has no_warmup = 1.

  1  the reference-order kernel == the oracle, every fixture, engine and CLI rules; the default
     certified search likewise
  2  test_gpu_wave_instances.py's sequence on the 1 mm slab and the blob: scan_groups x
     candidate_cache x certify_prev, scan32 = 0, cell_starts = 0 (cache_stores, cache_hits,
     prev_cert_lanes); two instances on the shiftable slab, whose first iterate is the origin's bits
  3  the cache under motion: stored, reused, loose (walk_loose), left (walk_moved), reused again
  4  the fp64 re-scan on the near-tie fixture (fp64_scan_waves)
  5  the half and wide lists (test_gpu_follow_lists.py's matrix and expected counts)
  6  the ball chain (test_gpu_ball_chain.py's cases, modes and counter expectations from the
     shifted tree); shell_deep* stay at the origin, where that file runs them
  7  the prewalk (prewalk_stores) against no prewalk
  8  host and device query order, host and device octree builder
  9  a host-driven session against the device loop, each iterate against the oracle
  10 a two-member host group at geo

No matrix is thinned at any offset: the whole file takes some eleven seconds.
"""
import itertools

import numpy as np
import pytest

import ball_fixtures as bf
import geo_fixtures as gf
import test_gpu_ball_chain as chain
import test_gpu_follow_lists as follow_lists
import test_gpu_wave_instances as waves

pytestmark = pytest.mark.gpu

PLACES = gf.PLACES
SLAB = "slab_mm_2048"
SLAB_GRID = "slab_grid_2048"


def _same(got, want, label):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{label}: indices")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{label}: residuals")


@pytest.fixture(scope="module")
def trees(icp, oracle):
    """(name, where) -> the fixture's clouds and its oracle tree, built once."""
    cache = {}

    def get(name, where):
        if (name, where) not in cache:
            tgt, src, mp, md = gf.clouds(icp, name, where)
            cache[name, where] = (tgt, src, mp, md, oracle.OracleTree(tgt, mp, md))
        return cache[name, where]

    return get


@pytest.fixture(scope="module")
def ref_ctx(icp):
    with icp.Context(0, icp.config(search=icp.SEARCH_REFERENCE, no_warmup=1)) as ctx:
        yield ctx


# ---- 1: the reference-order kernel

@pytest.mark.parametrize("where", PLACES)
@pytest.mark.parametrize("name", gf.SEARCH_FIXTURES)
def test_reference_kernel_equals_oracle(icp, oracle, trees, ref_ctx, name, where):
    tgt, src, mp, md, tree = trees(name, where)
    for rules, init in ((icp.RULES_ENGINE, oracle.DBL_MAX), (icp.RULES_CLI, 1e20)):
        want = tree.nn(src, init_best=init)
        ref_ctx.set_target(tgt, mp, md, rules)
        _same(ref_ctx.nn(src), want, f"nn, rules {rules}")
        ref_ctx.set_source(src)
        ref_ctx.iterate(None, 0, rules, 3.0)
        _same(ref_ctx.get_correspondences(), want, f"first iterate, rules {rules}")


@pytest.mark.parametrize("where", PLACES)
@pytest.mark.parametrize("name", gf.SEARCH_FIXTURES)
def test_default_search_equals_oracle(icp, oracle, trees, name, where):
    """The certified search as configured by default, on every fixture (the small sources too: one
    wave, one wave and a query, three waves and a query): nn(), the first iterate, and an iterate
    after it (the previous residuals as guesses), under both rule sets."""
    tgt, src, mp, md, tree = trees(name, where)
    with icp.Context(0, icp.config(no_warmup=1)) as ctx:
        for rules, init in ((icp.RULES_ENGINE, oracle.DBL_MAX), (icp.RULES_CLI, 1e20)):
            want = tree.nn(src, init_best=init)
            ctx.set_target(tgt, mp, md, rules)
            _same(ctx.nn(src), want, f"nn, rules {rules}")
            ctx.set_source(src)
            ctx.iterate(None, 0, rules, 3.0)
            _same(ctx.get_correspondences(), want, f"first iterate, rules {rules}")
            ctx.iterate(np.eye(4), 1, rules, 3.0)
            _same(ctx.get_correspondences(), want, f"second iterate, rules {rules}")
            if name in gf.SHIFTABLE:
                o_tgt, o_src, _, _, o_tree = trees(name, "origin")
                _same(ctx.nn(src), o_tree.nn(o_src, init_best=init), "translation invariance, nn")


# ---- 2: the wave-search instances

WAVE_STEPS = ("first iterate", "iterate 1 (transform)", "iterate 2 (transform)", "nn of the moved source",
              "iterate without a transform")
WAVE_MATRIX = [dict(scan_groups=g, candidate_cache=c, certify_prev=p)
               for g, c, p in itertools.product((1, 2, 4), (0, 1), (0, 3))]
WAVE_MATRIX += [dict(scan32=0), dict(cell_starts=0)]  # against the matrix's scan32 = 1, cell_starts = 1
WAVE_SHIFTABLE = [dict(scan_groups=1, candidate_cache=1, certify_prev=3), dict(scan_groups=4, candidate_cache=1, certify_prev=0)]


def _wave_cases():
    for name in (SLAB, "blob"):
        for where in PLACES:
            for cfg in WAVE_MATRIX:
                yield pytest.param(name, where, cfg, id=f"{name}-{where}-" + "-".join(f"{k}{v}" for k, v in cfg.items()))
    for where in PLACES:  # the shiftable slab: two instances, and the origin's bits on the first iterate
        for cfg in WAVE_SHIFTABLE:
            yield pytest.param(SLAB_GRID, where, cfg, id=f"{SLAB_GRID}-{where}-" + "-".join(f"{k}{v}" for k, v in cfg.items()))


def _wave_run(icp, ctx, tgt, src, transforms):
    """waves._steps, with the source each step searched and the counters after it."""
    seen = []

    def after(ctx):
        seen.append((ctx.get_source(), ctx.debug_counters()))

    steps, fitted = waves._steps(icp, ctx, tgt, src, transforms, after)
    return steps, fitted, seen


@pytest.fixture(scope="module")
def wave_reference(icp, oracle, trees):
    """(name, where) -> the reference-order context's sequence, its fitted transforms, and the
    oracle's answers for the source of each step (checked against each other here)."""
    cache = {}

    def get(name, where):
        if (name, where) in cache:
            return cache[name, where]
        tgt, src, _, _, tree = trees(name, where)
        with icp.Context(0, icp.config(search=icp.SEARCH_REFERENCE, no_warmup=1, debug_counters=1)) as ctx:
            steps, fitted, seen = _wave_run(icp, ctx, tgt, src, None)
        want = [tree.nn(s, init_best=oracle.DBL_MAX) for s, _ in seen]
        for label, got, w in zip(WAVE_STEPS, steps, want):
            _same(got, w, f"reference order, {label}")
        cache[name, where] = (want, fitted, [s for s, _ in seen])
        return cache[name, where]

    return get


@pytest.mark.parametrize("name,where,cfg", list(_wave_cases()))
def test_wave_instances(icp, trees, wave_reference, name, where, cfg):
    tgt, src, _, _, _ = trees(name, where)
    want, fitted, sources = wave_reference(name, where)
    with icp.Context(0, icp.config(no_warmup=1, debug_counters=1, **cfg)) as ctx:
        steps, _, seen = _wave_run(icp, ctx, tgt, src, fitted)
    for label, got, w, (s, c), rs in zip(WAVE_STEPS, steps, want, seen, sources):
        print(name, where, cfg, label, {k: c[k] for k in ("waves", "cache_stores", "cache_hits", "prev_cert_lanes",
                                                          "walk_moved", "walk_loose", "fp64_scan_waves", "overflow_waves")})
        np.testing.assert_array_equal(s, rs, err_msg=f"{label}: the moved source")
        _same(got, w, label)
    c1, c2 = seen[1][1], seen[2][1]
    if cfg.get("candidate_cache", 1) == 1:
        assert c1["cache_stores"] > 0, "the first transformed iterate stored no record"
        assert c2["cache_hits"] > 0, "the second transformed iterate reused no record"
    else:
        assert c1["cache_stores"] == c2["cache_hits"] == 0
    if cfg.get("certify_prev", 0) == 3:
        assert c1["prev_cert_lanes"] + c2["prev_cert_lanes"] > 0, "no previous match was certified"
    if name in gf.SHIFTABLE:
        o_want, _, _ = wave_reference(name, "origin")
        _same(steps[0], o_want[0], "translation invariance, first iterate")


# ---- 3: the cache under motion

def _motion(where):
    """The source starts 0.15 m above the slab. Steps: a tiny move (records of the wide boxes are
    stored), a tiny move (reused), the drop onto the surface (guesses of 0.3 m: new boxes), a tiny
    move (the boxes shrink to the residuals, inside the stored B+ but far smaller: loose), a tiny
    move (reused), 0.25 m along x (out of B+: moved), two tiny moves (loose again, then reused)."""
    def T(t):
        M = np.eye(4)
        M[:3, 3] = t
        return gf.conjugate(M, where)

    tiny = T([1e-4, -1e-4, 0.0])
    return [("store", tiny), ("reuse", tiny), ("drop", T([0.0, 0.0, -0.15])), ("loose", tiny), ("reuse 2", tiny),
            ("moved", T([0.25, 0.0, 0.0])), ("loose 2", tiny), ("reuse 3", tiny)]


def _motion_run(icp, oracle, cfg, tgt, lifted, tree, where):
    out = []
    with icp.Context(0, cfg) as ctx:
        ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
        ctx.set_source(lifted)
        ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)
        for k, (label, T) in enumerate(_motion(where)):
            ctx.iterate(T, k + 1, icp.RULES_ENGINE, 3.0)
            out.append((label, ctx.get_correspondences(), ctx.get_source(), ctx.debug_counters()))
    return out


@pytest.mark.parametrize("where", PLACES)
def test_cache_motion(icp, oracle, trees, where):
    tgt, src, _, _, tree = trees(SLAB, where)
    lifted = src + np.array([0.0, 0.0, 0.15])
    # candidate_loose 300: vol(B+) <= 3 vol(B). On 32 waves a box shrinks ~10 x (from balls of 0.3 m
    # to the residuals), not the 15 x of the default, which is set for millions of points.
    on = _motion_run(icp, oracle, icp.config(no_warmup=1, debug_counters=1, candidate_loose=300), tgt, lifted, tree, where)
    off = _motion_run(icp, oracle, icp.config(no_warmup=1, debug_counters=1, candidate_cache=0), tgt, lifted, tree, where)
    by = {}
    for (label, got, s, c), (_, ogot, os_, _) in zip(on, off):
        print(where, label, {k: c[k] for k in ("waves", "cache_stores", "cache_hits", "walk_moved", "walk_loose",
                                               "overflow_waves", "fp64_scan_waves")})
        np.testing.assert_array_equal(s, os_, err_msg=f"{label}: the moved source")
        _same(got, ogot, f"{label}: cache on against off")
        _same(got, tree.nn(s, init_best=oracle.DBL_MAX), f"{label}: against the oracle")
        by[label] = c
    assert by["store"]["cache_stores"] > 0
    assert by["reuse"]["cache_hits"] > 0
    assert by["loose"]["walk_loose"] + by["loose 2"]["walk_loose"] > 0, "no record was found loose"
    assert by["drop"]["walk_moved"] + by["moved"]["walk_moved"] > 0, "no wave left its B+"
    assert by["reuse 2"]["cache_hits"] > 0 and by["reuse 3"]["cache_hits"] > 0, "no reuse after the re-walks"


# ---- 4: the fp64 re-scan

@pytest.mark.parametrize("where", PLACES)
@pytest.mark.parametrize("name", ("near_tie", "near_tie_close"))
def test_fp64_rescan_on_near_ties(icp, oracle, trees, name, where):
    """near_tie_close runs in the host query order, for which geo_fixtures.wave_ext_floor bounds ext
    on the CPU: there the certificate rests on e_abs, not on the slack of the selection key's
    cleared bits. (A scratch build with e_abs from ext / 4 still passes: DESIGN.md section 4.)"""
    tgt, src, mp, md, tree = trees(name, where)
    for rules, init in ((icp.RULES_ENGINE, oracle.DBL_MAX), (icp.RULES_CLI, 1e20)):
        want = tree.nn(src, init_best=init)
        with icp.Context(0, icp.config(no_warmup=1, debug_counters=1, query_order=int(name == "near_tie_close"))) as ctx:
            ctx.set_target(tgt, mp, md, rules)
            ctx.set_source(src)
            ctx.iterate(None, 0, rules, 3.0)
            first = ctx.get_correspondences()
            c0 = ctx.debug_counters()
            ctx.iterate(np.eye(4), 1, rules, 3.0)  # after a search: the previous residuals as guesses
            second = ctx.get_correspondences()
            c1 = ctx.debug_counters()
            nn = ctx.nn(src)
        print(name, where, rules, {k: (c0[k], c1[k]) for k in ("waves", "fp64_scan_waves", "overflow_waves", "not_joined")})
        _same(first, want, "first iterate")
        _same(second, want, "second iterate")
        _same(nn, want, "nn")
        assert c0["fp64_scan_waves"] > 0 and c1["fp64_scan_waves"] > 0, "no wave re-scanned in fp64"


# ---- 5: the half and wide lists

@pytest.mark.parametrize("where", PLACES)
@pytest.mark.parametrize("n,overflow_halves,wide_pass", list(itertools.product(bf.SIZES, (0, 1), (0, 1))))
def test_half_and_wide_lists(icp, oracle, trees, n, overflow_halves, wide_pass, where):
    tgt, src, _, _, tree = trees(f"follow_{n}", where)
    want = tree.nn(src, init_best=oracle.DBL_MAX)
    cfg = icp.config(no_warmup=1, debug_counters=1, query_order=1, overflow_halves=overflow_halves, wide_pass=wide_pass)
    with icp.Context(0, cfg) as ctx:
        ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
        ctx.set_source(src)
        ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)
        got = ctx.get_correspondences()
        first = ctx.debug_counters()
        nn = ctx.nn(src)
        both = ctx.debug_counters()  # nn() adds to the iterate's counters
    _same(got, want, "first iterate")
    _same(nn, want, "nn")
    expect = follow_lists._expected(n // 64, overflow_halves == 1, wide_pass == 0)
    for label, c, times in (("first iterate", first, 1), ("first iterate + nn", both, 2)):
        counted = {"overflow_waves": c["overflow_waves"], "halves": c["halves"],
                   "wide_entries": c["wide_waves"] + c["wide_stack"]}
        assert counted == {k: times * v for k, v in expect.items()}, label


# ---- 6: the ball chain

def _ball_cases():
    for where in PLACES:
        for name in gf.BALL_NAMES:
            for n in bf.SIZES:
                for ball_mode, cell_starts in chain.MODES:
                    yield pytest.param(name, n, ball_mode, cell_starts, where,
                                       id=f"{name}-{n}-mode{ball_mode}-cells{cell_starts}-{where}")


@pytest.fixture(scope="module")
def ball_reference(icp, oracle):
    cache = {}

    def get(name, n, where):
        if (name, n, where) not in cache:
            tgt, src, mp, md = gf.ball(name, n, where)
            cache[name, n, where] = chain._reference_case(icp, oracle, _chain_name(name), n, tgt, src, mp, md,
                                                          gf.ball_model(icp, name, where),
                                                          gf.conjugate(chain._far_move(), where))
        return cache[name, n, where]

    return get


def _chain_name(name):
    return "shell" if name == "shell_grid" else name  # the shell's chain and expectations, on the grid


@pytest.mark.parametrize("name,n,ball_mode,cell_starts,where", list(_ball_cases()))
def test_ball_chain(icp, ball_reference, name, n, ball_mode, cell_starts, where):
    case = ball_reference(name, n, where)
    got, errors = chain._run_case(icp, case, _chain_name(name), n, ball_mode, cell_starts, gf.ball_model(icp, name, where),
                                  gf.conjugate(chain._far_move(), where))
    assert "oracle" in case[4]  # every size here is compared with the oracle (n <= 1024)
    if f"{name}_{n}" in gf.SHIFTABLE and where != "origin":
        origin = ball_reference(name, n, "origin")[4]
        for k in (0, 2):  # the untransformed steps: the first iterate and nn of the source
            for j, what in enumerate(("indices", "residuals")):
                if got["steps"][k][j].tobytes() != origin["oracle"][k][j].tobytes():
                    errors.append(f"{chain.STEP_NAMES[k]}: {what} are not the origin's (translation invariance)")
    assert not errors, "\n".join(errors)


# ---- 7: the prewalk

def _drift(where, k):
    """Iterate k's motion: along (1, -0.6, 0) by 4 mm x 1.5^(k-1) with 0.02 degrees about z. The
    stored lead is 8 x the displacement of the iterate that stored the record, so a drift that
    grows uses it up within a few iterates and the look-ahead of 2 asks before the box leaves."""
    a = np.radians(0.02)
    M = np.eye(4)
    M[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    M[:3, 3] = np.array([1.0, -0.6, 0.0]) * 0.004 * 1.5 ** (k - 1)
    return gf.conjugate(M, where)


@pytest.mark.parametrize("where", PLACES)
def test_prewalk_on_equals_off(icp, oracle, trees, where):
    tgt, src, _, _, tree = trees(SLAB, where)

    def run(look):
        out = []
        with icp.Context(0, icp.config(no_warmup=1, debug_counters=1)) as ctx:
            ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
            ctx.set_source(src)
            ctx.set_prewalk(look)
            for k in range(8):
                ctx.iterate(_drift(where, k) if k else None, k, icp.RULES_ENGINE, 3.0)
                out.append((ctx.get_correspondences(), ctx.get_source(), ctx.debug_counters()))
        return out

    on, off = run(2.0), run(0.0)
    for k, ((got, s, c), (ogot, os_, oc)) in enumerate(zip(on, off)):
        print(where, k, {n: (c[n], oc[n]) for n in ("prewalk_stores", "cache_hits", "cache_stores", "walk_moved", "walk_loose")})
        np.testing.assert_array_equal(s, os_)
        _same(got, ogot, f"iterate {k}: prewalk on against off")
        _same(got, tree.nn(s, init_best=oracle.DBL_MAX), f"iterate {k}: against the oracle")
    assert sum(c["prewalk_stores"] for _, _, c in on) > 0, "the prewalk stored no record"
    assert all(c["prewalk_stores"] == 0 for _, _, c in off)
    # A prewalked record is exact wherever its box lies (its list is that of the B+ it stores), so a
    # box rebuilt in the wrong place changes no result: it shows only here. The records the prewalk
    # stored are the ones the next boxes lie in, so fewer waves leave their B+ than without it
    # (as test_gpu_prewalk.py's test_prewalk_replaces_walks asserts at the origin).
    moved_on, moved_off = (sum(c["walk_moved"] for _, _, c in run[2:]) for run in (on, off))
    assert moved_off > 0 and moved_on < moved_off, (moved_on, moved_off)


# ---- 8: query order and builders

@pytest.mark.parametrize("where", PLACES)
@pytest.mark.parametrize("name", (SLAB, "slab_cont_2048"))
def test_query_order_and_builders(icp, trees, wave_reference, name, where):
    tgt, src, _, _, _ = trees(name, where)
    want, fitted, sources = wave_reference(name, where)
    for cfg in (dict(query_order=0, octree_builder=icp.BUILD_AUTO), dict(query_order=1, octree_builder=icp.BUILD_AUTO),
                dict(query_order=0, octree_builder=icp.BUILD_HOST), dict(query_order=1, octree_builder=icp.BUILD_HOST)):
        with icp.Context(0, icp.config(no_warmup=1, debug_counters=1, **cfg)) as ctx:
            steps, _, seen = _wave_run(icp, ctx, tgt, src, fitted)
            assert ctx.target_build_info()[0] == (cfg["octree_builder"] == icp.BUILD_AUTO)
            if cfg["query_order"] == 1:
                np.testing.assert_array_equal(ctx.query_order(), icp.source_shard_order(src))
        for label, got, w, (s, _), rs in zip(WAVE_STEPS, steps, want, seen, sources):
            np.testing.assert_array_equal(s, rs, err_msg=f"{cfg} {label}: the moved source")
            _same(got, w, f"{cfg} {label}")


# ---- 9: the session loop

@pytest.mark.parametrize("where", PLACES)
def test_session_host_loop_equals_device_loop(icp, oracle, trees, where):
    tgt, src, _, _, tree = trees(SLAB, where)
    params = icp.params_default(max_iterations=6, tolerance=1e-9, flags=icp.FLAG_NO_EARLY_STOP)

    def register(loop):
        with icp.Context(0, icp.config(no_warmup=1, device_loop=loop)) as ctx:
            ctx.set_target(tgt, 10, 20, params.rules)
            ctx.set_source(src)
            rc, res, hist = ctx.run(params)
            return rc, bytes(memoryview(res)), [bytes(memoryview(h)) for h in hist], ctx.get_source(), ctx.get_correspondences()

    host, dev = register(0), register(1)
    assert host[0] == dev[0] == 0 and len(host[2]) >= 5
    assert host[1] == dev[1] and host[2] == dev[2], "the records differ"
    np.testing.assert_array_equal(host[3], dev[3])
    _same(host[4], dev[4], "the last correspondences")
    with icp.Context(0, icp.config(no_warmup=1)) as ctx:
        ctx.set_target(tgt, 10, 20, params.rules)
        ctx.set_source(src)
        sess = ctx.session(params)
        records = []
        for k in range(len(host[2])):
            rec = sess.step()
            assert rec is not None
            records.append(bytes(memoryview(rec)))
            s = ctx.get_source()  # the source this iterate searched
            _same(ctx.get_correspondences(), tree.nn(s, init_best=oracle.DBL_MAX), f"iterate {k} against the oracle")
        sess.close()
    assert records == host[2], "stepping and icp_engine_run give different records"


# ---- 10: a group

def test_host_group_of_two_at_geo(icp, oracle, trees, wave_reference):
    tgt, src, _, _, tree = trees(SLAB, "geo")
    want, fitted, sources = wave_reference(SLAB, "geo")

    def run(ctx):
        out = []
        with ctx:
            ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
            ctx.set_source(src)
            for k, T in enumerate((None, *fitted)):
                ctx.iterate(T, k, icp.RULES_ENGINE, 3.0)
                out.append((ctx.get_correspondences(), ctx.get_source()))
        return out

    cfg = icp.config(no_warmup=1)
    group = run(icp.Context(devices=[0, 0], cfg=cfg, transport=icp.XPORT_HOST))
    plain = run(icp.Context(0, cfg))
    for k, ((g, gs), (p, ps)) in enumerate(zip(group, plain)):
        np.testing.assert_array_equal(gs, ps)
        np.testing.assert_array_equal(gs, sources[k])
        _same(g, p, f"iterate {k}: group against one context")
        _same(g, want[k], f"iterate {k}: against the oracle")
