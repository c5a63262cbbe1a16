"""k_nn_ball's chain (csrc/nn_ball.hip), link by link, at the smallest shapes that reach each link:
the 16-lane ball walk, the budgeted per-lane search (lane_query), the wave-cooperative branch and
bound (wave_bb), the reference-order DFS, and the direct mode that enters at wave_bb.

Queries get onto the ball list as in test_gpu_follow_lists.py: with the wide pass off (wide_pass =
1) and the half pass off (overflow_halves = 0) every query of a wave whose search box holds more
than kWaveCandCap target points goes there with its guess. The clouds and the CPU pre-checks that
make each link certain are in ball_fixtures.py; they run, and assert, before the fixture's first GPU
call (the `reference` fixture below).

Every fixture and source size runs under ball_mode 1, 2, 0 x cell_starts 1, 0: a first iterate, a
second iterate with the transform fitted from the reference run's statistics (the ball kernel
then reads the stored, moved queries), nn() of the original source (nn_core's own carve-up) and a
third iterate after a far move (0.16, eight times uniform's nearest distances: the previous matches
are loose guesses, balls overflow and the per-lane searches that follow mostly finish within their
budget, the one outcome of link 2 that the first iterates never show: uniform's balls do not
overflow, the shells' searches all run out of budget).
At every step the indices and residuals equal a search = REFERENCE context's bit for bit, the
iterates' statistics (valid, mean, std, rmse, H) equal that context's, and for these small sources
the CPU oracle's answers too. The first iterate's debug counters prove the link ran. The expected
counts follow from the code and the pre-checks, not from a run:

  n_ball_search   64 x (n // 64) on uniform and lattice_ties: the full waves. On the shells it is n:
                  pre-check (d) holds for every query, so the last, partial wave of 65 and 193
                  (one query) overflows as well, and so does the half wave of the long case (64 x
                  (n // 64) would count the full waves only)
  shells, ball walk   every entry has a finite guess (an overflowed wave's lanes are listed with
                  their own guess u, which the first iterate's descent always finds), so every ball
                  is walked and overflows by (a): ball_overflow = n_ball_search (no +inf guess: the
                  counters not_covered and no_guess, the only sources of one, are printed and are 0);
                  every per-lane search runs out of budget by (b): lane_handed = bb_queries =
                  n_lane_search = n_ball_search; wave_bb cannot overflow by (c): bb_overflow = 0
  shells, direct  bb_queries = n_lane_search = n_ball_search, lane_handed = 0, bb_overflow = 0, and
                  no ball is walked: ball_overflow = ball_points = 0
  shell_flat      the leaf points wave_bb must list (ball_fixtures.listed_points, a lower bound
                  from the CPU) exceed kBBPts x bb_steps, so some step listed more than kBBPts points
                  and ran the `base` loop for more than one round
  shell_ties      the shells' counts, and every wave_bb returns 2 (the nearest point and its mirror
                  image tie): lane_exact = n_ball_search <= n_fallback. Under the ball walk this
                  is the DFS run inline by lane 0 after the handed-over search (lattice_ties' balls
                  do not overflow: its ties are caught by the ball walk itself, follow = 2, and
                  never reach wave_bb there)
  lattice_ties    direct: wave_bb returns 2 (or 0) for every query, lane_exact = bb_queries =
                  n_ball_search. Ball walk: every entry ends in the reference-order DFS (follow = 2,
                  or an uncertified lane_query, or wave_bb's 2), each counted once in
                  dfs_finishes: n_fallback >= n_ball_search
  uniform, ball walk   ball_points > 0 and ball_overflow < n_ball_search

ball_mode 0 takes the direct mode when n_ball_search > 4 x blocks, blocks = min(ceil(n / 4), 8192)
(launch_nn_follow sizes the grid by the launch's n queries). n_ball_search <= n <= 4 ceil(n / 4), so
below 32 768 queries the rule always picks the ball walk: 64, 65 and 193 all land on the ball-walk
side, none of them on the other. test_shell_large adds the other side: 40 000
queries on the shell under ball_mode 0 (40 000 > 4 x 8192: direct).

test_shell_large's second case is the ball walk forced (ball_mode 1) on 500 000 shell queries: 8192
blocks of four groups, 16 trips per block, the queue flushed inside the loop (qn > 64 - kBallGroups)
and the grid-stride's later trips. Reference-order context only, no CPU oracle.

shell_deep runs under max_depth 20 (device builder) and 40 (host builder): stack levels 20 and 40,
so launch_nn_follow's LDS and ball_queue_off are levels x 512 bytes (10 240 and 20 480) instead of
the 8192-byte floor of every other fixture (levels <= 16).

wave_bb's frontier overflow (bb_overflow > 0) is printed for every case; no fixture here reaches it.
"""
import itertools
import time

import numpy as np
import pytest

import ball_fixtures as bf

pytestmark = pytest.mark.gpu

CASES = [(name, n) for name in ("uniform", "shell", "shell_deep20", "shell_deep40", "shell_flat") for n in bf.SIZES]
CASES += [(name, n) for name in ("shell_ties", "lattice_ties") for n in bf.LATTICE_SIZES]
MODES = list(itertools.product((1, 2, 0), (1, 0)))  # ball_mode x cell_starts
BALL_COUNTERS = ("ball_overflow", "ball_points", "lane_handed", "bb_queries", "bb_steps", "bb_overflow", "lane_exact",
                 "not_covered", "no_guess", "overflow_waves")


def _config(icp, ball_mode, cell_starts):
    # fused_cull = 0: the statistics come from the full cull pass, as in the reference-order context
    # (same host query order there), so they are the same sums in the same order and must be equal
    # to the bit. The fused sums add in another order by design (test_gpu_fused_cull.py: 1e-12).
    return icp.config(no_warmup=1, debug_counters=1, query_order=1, wide_pass=1, overflow_halves=0, fused_cull=0,
                      ball_mode=ball_mode, cell_starts=cell_starts)


def _record(st):
    return (st.valid, st.mean, st.std, st.rmse, tuple(st.H))


def _far_move():
    """2 degrees about z and (0.12, -0.09, 0.06): some 0.16, eight times the uniform cloud's nearest
    distances, so the previous matches are loose guesses."""
    c, s = np.cos(np.radians(2.0)), np.sin(np.radians(2.0))
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.12, -0.09, 0.06]
    return T


def _steps(icp, ctx, tgt, src, mp, md, T=None, counters=False, far_move=None):
    """The four steps in one context. T None: fitted from this context's first iterate (the
    reference run). far_move None: _far_move() (a shifted fixture hands in its own). Returns the steps' (indices, residuals), the iterates' records, T, the moved
    sources, the IterStats of the iterates and the counters of each step."""
    ctx.set_target(tgt, mp, md, icp.RULES_ENGINE)
    ctx.set_source(src)
    st0 = ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)
    out = [ctx.get_correspondences()]
    dbg = [ctx.debug_counters()] if counters else []
    if T is None:
        T = icp.best_fit_from_stats(st0)
    st1 = ctx.iterate(T, 1, icp.RULES_ENGINE, 3.0)
    out.append(ctx.get_correspondences())
    moved = ctx.get_source()
    if counters:
        dbg.append(ctx.debug_counters())
    out.append(ctx.nn(src))
    if counters:
        both = ctx.debug_counters()  # nn() adds to the last iterate's counters
        dbg.append({k: both[k] - dbg[1][k] for k in both})
    st2 = ctx.iterate(_far_move() if far_move is None else far_move, 2, icp.RULES_ENGINE, 3.0)
    out.append(ctx.get_correspondences())
    far = ctx.get_source()
    if counters:
        dbg.append(ctx.debug_counters())
    return {"steps": out, "records": [_record(st0), _record(st1), _record(st2)], "T": T, "moved": moved, "far": far,
            "st0": st0, "st2": st2, "dbg": dbg,
            "levels": ctx.target_info()["stack_levels"], "on_device": ctx.target_build_info()[0]}


def _precheck(icp, name, n, tgt, src, model=None):
    """The fixture's CPU pre-checks (they assert). Returns what they measured, for the log. model:
    the tree model of a shifted target (default: the fixture's own)."""
    model = bf.tree_model(icp, name) if model is None else model
    info = {"levels": model["levels"], "max_depth": model["max_depth"]}
    if name.startswith("shell"):
        # every query alone overflows its wave (d), so the partial waves need no box check
        info.update(bf.check_chain(model, tgt, src) if n <= 1024 else bf.check_chain_in_cube(model, tgt))
    else:
        info["wave_box"] = bf.check_waves_overflow(icp, tgt, src)
    if name == "shell_deep20":
        assert (model["max_depth"], model["levels"]) == (20, 20), info
    elif name == "shell_deep40":
        assert (model["max_depth"], model["levels"]) == (40, 40), info
    else:
        assert model["levels"] <= 16, info  # the 8192-byte floor of launch_nn_follow's LDS
    if name == "shell_flat":
        info["top64_leaf_points"] = bf.check_flat_rounds(model)
    if name in ("lattice_ties", "shell_ties"):
        info["ties"] = bf.check_ties(tgt, src)
    return info


def _reference_case(icp, oracle, name, n, tgt, src, mp, md, model=None, far_move=None):
    """A case's clouds, the reference-order context's four steps and, for the small sources, the
    oracle's answers, after the pre-checks (model, far_move: a shifted fixture's, see _precheck, _steps)."""
    info = _precheck(icp, name, n, tgt, src, model)
    print("pre-checks", name, n, info)
    # the same (host) query order as the contexts under test: the statistics are sums in slot order
    with icp.Context(0, icp.config(search=icp.SEARCH_REFERENCE, no_warmup=1, query_order=1)) as ctx:
        ref = _steps(icp, ctx, tgt, src, mp, md, far_move=far_move)
    assert ref["levels"] == info["levels"] and ref["on_device"] == (md <= bf.GPU_BUILD_MAX_DEPTH), (name, ref["levels"])
    assert np.all(np.isfinite(ref["T"])) and np.all(np.isfinite(ref["moved"])), name
    if n <= 1024:
        tree = oracle.OracleTree(tgt, mp, md)
        first = tree.nn(src, init_best=oracle.DBL_MAX)
        ref["oracle"] = [first, tree.nn(ref["moved"], init_best=oracle.DBL_MAX), first,
                         tree.nn(ref["far"], init_best=oracle.DBL_MAX)]
    for a in (ref["moved"], ref["far"], *(x for pair in ref["steps"] + ref.get("oracle", []) for x in pair)):
        a.setflags(write=False)
    return tgt, src, mp, md, ref


@pytest.fixture(scope="module")
def reference(icp, oracle):
    """(name, n) -> the clouds, the reference-order context's four steps and, for the small
    sources, the oracle's answers; computed once per case, after its pre-checks."""
    cache = {}

    def get(name, n):
        if (name, n) in cache:
            return cache[name, n]
        cache[name, n] = _reference_case(icp, oracle, name, n, *bf.clouds(name, n))
        return cache[name, n]

    return get


STEP_NAMES = ("first iterate", "second iterate (moved source)", "nn of the source", "third iterate (far move)")


def _compare(errors, got, ref):
    """Bit-for-bit comparison of a context's four steps with the reference run (and the oracle)."""
    def same(label, a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            errors.append(f"{label}: {int((a != b).sum()) if a.shape == b.shape else 'shape'} of {a.size} differ")

    for k, name in enumerate(STEP_NAMES):
        same(f"{name}: indices vs the reference order", got["steps"][k][0], ref["steps"][k][0])
        same(f"{name}: residuals vs the reference order", got["steps"][k][1], ref["steps"][k][1])
        if "oracle" in ref:
            same(f"{name}: indices vs the oracle", got["steps"][k][0], ref["oracle"][k][0])
            same(f"{name}: residuals vs the oracle", got["steps"][k][1], ref["oracle"][k][1])
    same("moved source", got["moved"], ref["moved"])
    same("far source", got["far"], ref["far"])
    for k, step in enumerate((0, 1, 3)):
        if got["records"][k] != ref["records"][k]:
            errors.append(f"{STEP_NAMES[step]}: statistics {got['records'][k]} != reference {ref['records'][k]}")


def _direct(n, n_ball, ball_mode):
    """launch_nn_follow's grid and k_nn_ball's rule."""
    blocks = min(-(-n // bf.BALL_GROUPS), bf.BALL_MAX_BLOCKS)
    return ball_mode == 2 or (ball_mode == 0 and n_ball > 4 * blocks)


def _check_counters(errors, icp, name, n, ball_mode, got, tgt, src, model=None):
    """The first iterate's counters against the counts derived in the module docstring."""
    st, c = got["st0"], got["dbg"][0]
    shell = name.startswith("shell")
    n_ball = n if shell else 64 * (n // 64)
    direct = _direct(n, n_ball, ball_mode)

    def want(label, ok):
        if not ok:
            errors.append(f"counters: {label}")

    want(f"n_ball_search {st.n_ball_search} != {n_ball}", st.n_ball_search == n_ball)
    want(f"bb_overflow {c['bb_overflow']} > 0 on a fixture that cannot reach it", c["bb_overflow"] == 0 or not shell)
    if shell and not direct:
        want("ball walk: lane_handed == bb_queries == n_lane_search == ball_overflow == n_ball_search",
             c["lane_handed"] == c["bb_queries"] == st.n_lane_search == c["ball_overflow"] == n_ball)
        want("ball walk: bb_steps > 0", c["bb_steps"] > 0)
    if shell and direct:
        want("direct: bb_queries == n_lane_search == n_ball_search", c["bb_queries"] == st.n_lane_search == n_ball)
        want("direct: lane_handed == ball_overflow == ball_points == 0",
             c["lane_handed"] == c["ball_overflow"] == c["ball_points"] == 0)
    if name == "shell_flat" and st.n_ball_search == n_ball:
        listed = bf.listed_points(bf.tree_model(icp, name) if model is None else model, tgt, src)
        want(f"shell_flat: listed points {listed} <= {bf.BB_PTS} x bb_steps {c['bb_steps']}: no multi-round step proven",
             listed > bf.BB_PTS * c["bb_steps"])
    if name == "shell_ties":
        want("every wave_bb ends in a tie: lane_exact == n_ball_search <= n_fallback",
             c["lane_exact"] == n_ball <= st.n_fallback)
    if name == "lattice_ties" and direct:
        want("direct: lane_exact == bb_queries == n_ball_search", c["lane_exact"] == c["bb_queries"] == n_ball)
    if name == "lattice_ties" and not direct:
        want(f"ball walk: n_fallback {st.n_fallback} < n_ball_search", st.n_fallback >= n_ball)
    if name == "uniform" and not direct:
        want("ball walk: ball_points > 0 and ball_overflow < n_ball_search",
             c["ball_points"] > 0 and c["ball_overflow"] < n_ball)
        # the far move (not derived from a pre-check: a guard that the step still reaches the link)
        f, sf = got["dbg"][3], got["st2"]
        want(f"far move: no ball overflowed or no per-lane search finished within its budget "
             f"(ball_overflow {f['ball_overflow']}, n_lane_search {sf.n_lane_search}, lane_handed {f['lane_handed']})",
             f["ball_overflow"] > 0 and sf.n_lane_search > f["lane_handed"])


def _run(icp, reference, name, n, ball_mode, cell_starts):
    return _run_case(icp, reference(name, n), name, n, ball_mode, cell_starts)


def _run_case(icp, case, name, n, ball_mode, cell_starts, model=None, far_move=None):
    tgt, src, mp, md, ref = case
    with icp.Context(0, _config(icp, ball_mode, cell_starts)) as ctx:
        got = _steps(icp, ctx, tgt, src, mp, md, T=ref["T"], counters=True, far_move=far_move)
    for step, c in zip(STEP_NAMES, got["dbg"]):
        print(f"{name} n {n} ball_mode {ball_mode} cell_starts {cell_starts} {step}:",
              {k: c[k] for k in BALL_COUNTERS})
    st = got["st0"]
    print(f"{name} n {n} ball_mode {ball_mode} cell_starts {cell_starts} first iterate: n_ball_search {st.n_ball_search} "
          f"n_lane_search {st.n_lane_search} n_fallback {st.n_fallback} levels {got['levels']} "
          f"ball_queue_off {max(bf.BALL_LDS_FLOOR, 512 * got['levels'])}")
    errors = []
    _compare(errors, got, ref)
    _check_counters(errors, icp, name, n, ball_mode, got, tgt, src, model)
    return got, errors


@pytest.mark.parametrize("ball_mode,cell_starts", MODES)
@pytest.mark.parametrize("name,n", CASES)
def test_chain(icp, reference, name, n, ball_mode, cell_starts):
    _, errors = _run(icp, reference, name, n, ball_mode, cell_starts)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("n,ball_mode", [(40_000, 0), (bf.N_LONG, 1)])
def test_shell_large(icp, reference, n, ball_mode):
    """40 000 queries under the rule (ball_mode 0): the direct side of it. 500 000 under ball_mode 1:
    the ball walk's grid-stride trips and the flush inside its loop (only ball_mode 1 reaches them:
    the rule sends a list this long to the direct mode)."""
    reference("shell", n)  # outside the timing
    t0 = time.perf_counter()
    _, errors = _run(icp, reference, "shell", n, ball_mode, 1)
    print(f"shell n {n} ball_mode {ball_mode}: {time.perf_counter() - t0:.3f} s for the certified context's four steps")
    assert not errors, "\n".join(errors)


def test_shell_is_deterministic(icp, reference):
    """The same shell case twice: the same bytes at every step (and the same statistics)."""
    runs = [_run(icp, reference, "shell", 193, 1, 1)[0] for _ in range(2)]
    for (ia, da), (ib, db) in zip(runs[0]["steps"], runs[1]["steps"]):
        assert ia.tobytes() == ib.tobytes() and da.tobytes() == db.tobytes()
    assert runs[0]["records"] == runs[1]["records"] and runs[0]["moved"].tobytes() == runs[1]["moved"].tobytes()
