"""The iterate's statistics record (reduce_kernels.hip, wave_stats.h: k_moments, k_cull_waves in
its full and fused modes, wave_cov_sums, the merge trees, k_finalize_moments, k_merge_cov_last) at
the shapes where its control flow changes and on degenerate residuals, against the high-precision
reference and the derived bounds of tests/stats_reference.py. Every record is checked in three
layers (stats_reference.check_record): exact self-consistency, accuracy within the bounds, and the
exact valid count wherever no residual lies within the threshold's bound of the threshold.

The inputs' own properties (the gap condition, the band-lane counts) are validated on the CPU by
tests/test_stats_reference.py. Each test prints its largest error / bound ratio per field.

Exact ties. Where the reference threshold equals a residual in exact arithmetic, whether that
residual counts as valid is decided by the rounding of mean + k sd, the reference engine's as much
as ours, so the valid count is not compared with the exact one (layer 3 only): a single residual
under the plain rule (sd = 0, threshold = the residual), two residuals at sigma 1 (mean + sd is
the larger one), and the zero and constant residuals of the degenerate cases. Every other case
must keep the gap.
"""
import numpy as np
import pytest

import stats_reference as R

pytestmark = pytest.mark.gpu

_TREES = {}


def _tree(oracle, tgt):
    key = (len(tgt), tgt[:1].tobytes())
    if key not in _TREES:
        _TREES[key] = oracle.OracleTree(tgt)
    return _TREES[key]


def _assert_oracle_pairs(oracle, tgt, a, idx, d, label):
    oidx, od = _tree(oracle, tgt).nn(a, init_best=oracle.DBL_MAX)
    assert np.array_equal(idx, oidx), label
    assert d.tobytes() == od.tobytes(), label


def _iterates(icp, oracle, ctx, tgt, src, rules, sigma, iters, ratios, label, *, fit=True, members=1, layer3=True,
              pairs_from_oracle=False):
    """Set the clouds and run `iters` iterates (the first without a transform, the later ones with
    the best fit of the previous record, or with the identity): yields (iteration, record, path,
    d, idx, reference, band in force) after the three layers have been applied."""
    ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
    ctx.set_source(src)
    T, a_first, b_first, band = None, None, None, R.Band()
    for it in range(iters):
        st = ctx.iterate(T, it, rules, sigma)
        path = ctx.last_cull_path()
        idx, d = ctx.get_correspondences()
        a = ctx.get_source()
        b = tgt[idx]
        lab = f"{label} iterate {it}"
        if pairs_from_oracle:
            _assert_oracle_pairs(oracle, tgt, a, idx, d, lab)
        ref = R.check_record(st, d, a, b, rules, it, sigma, a_first=a_first, b_first=b_first, members=members,
                             ratios=ratios, layer3=layer3, label=lab)
        yield it, st, path, d, idx, ref, band
        if ref is not None:
            band.next(float(ref["thr"]))
        if it == 0:
            a_first, b_first = a, b
        T = icp.best_fit_from_stats(st) if fit and ref is not None else np.eye(4)


@pytest.fixture(scope="module")
def ctx(icp):
    with icp.Context(0) as c:
        yield c


# ---- a. shape boundaries

@pytest.mark.parametrize("rules,sigma", R.RULE_CASES)
@pytest.mark.parametrize("n_src,n_tgt", R.SHAPE_CASES)
def test_shape_boundaries(icp, oracle, ctx, n_src, n_tgt, rules, sigma):
    """A wave (64), the 8-wave minimum of a cull block (512), a moments part (4096), two parts and
    the 256-wave cull block (16385), each with its neighbours; four iterates. At 5000 target points
    the correspondences are the oracle's bit for bit."""
    tgt, src = R.shape_pair(n_src, n_tgt)
    ratios = {}
    label = f"n_src {n_src} n_tgt {n_tgt} rules {rules} sigma {sigma}"
    for it, st, path, d, idx, ref, band in _iterates(icp, oracle, ctx, tgt, src, rules, sigma, 4, ratios, label,
                                                     pairs_from_oracle=n_tgt == 5000):
        if it == 0:
            assert path == 0, label
        if it >= 2 and band.holds(float(ref["thr"])):
            assert path == 1, (label, it)
        if n_src == 1 and not (rules == R.RULES_ENGINE and it == 0):
            # the shift is the residual itself: the sums are zeros, the record exact
            assert st.mean == d[0] and st.std == 0.0 and st.threshold == d[0] and st.valid == 1, (label, it)
    R.print_ratios(label, ratios)


# ---- b. georeferenced magnitudes

@pytest.mark.parametrize("rules,sigma", [(R.RULES_ENGINE, 3.0), (R.RULES_CLI, 1.0)])
@pytest.mark.parametrize("n_src", R.GEO_SOURCES)
def test_georeferenced_statistics_of_the_reported_pairs(icp, oracle, ctx, n_src, rules, sigma):
    """The clouds of the shape cases plus (4e5, 5e6, 100): the statistics of whatever pairs the
    context reports, within the bounds that hold at the origin (sums taken at the offset's scale
    instead of the data's spread would miss the bound on H by about eight orders of magnitude),
    and each reported residual is sqrt(fl(dx^2 + dy^2 + dz^2)) of its reported pair.

    It deliberately does not assert that the reported pairs are the nearest ones: the search's
    parity with the oracle at such offsets is out of scope here."""
    tgt, src = R.shape_pair(n_src, 5000, geo=True)
    ratios = {}
    label = f"geo n_src {n_src} rules {rules} sigma {sigma}"
    ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
    ctx.set_source(src)
    T, a_first, b_first = None, None, None
    for it in range(4):
        st = ctx.iterate(T, it, rules, sigma)
        idx, d = ctx.get_correspondences()
        a = ctx.get_source()
        b = tgt[idx]
        e = a - b
        assert np.array_equal(d, np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])), (label, it)
        R.check_record(st, d, a, b, rules, it, sigma, a_first=a_first, b_first=b_first, ratios=ratios, layer3=False,
                       label=f"{label} iterate {it}")
        if it == 0:
            a_first, b_first = a, b
        T = icp.best_fit_from_stats(st)
    R.print_ratios(label, ratios)


# ---- c. the band's paths

@pytest.fixture(scope="module")
def band_ctxs(icp):
    with icp.Context(0, {"debug_counters": 1}) as fused, icp.Context(0, {"debug_counters": 1, "fused_cull": 0}) as full:
        yield fused, full


@pytest.mark.parametrize("name", R.BAND_CASES)
def test_band_paths(icp, oracle, band_ctxs, name):
    """Single-wave sources (64 and 40 queries) with constructed residuals on a lattice target,
    identity transforms under CLI rules: the threshold repeats bit for bit, the band narrows from
    25 % (second iterate) to 5 % (third, fourth). The band holds 0, 1, 8 (the most a thread adds
    lane by lane), 9 (the wave tree) or more than 32 lanes, on both sides of the threshold
    (stats_reference.band_case; the counts are validated on the CPU). fz_band is the band-lane count
    of the waves the search finished, fz_recompute the waves it flagged for the cull: a case
    without a far query must run unflagged with the reference's band-lane count, a case with one
    (it leaves the wave search) flagged. Every iterate also against a fused_cull = 0 context."""
    fused, full = band_ctxs
    tgt, src, sigma, want, flagged = R.band_case(name)
    ratios = {}
    runs = [_iterates(icp, oracle, c, tgt, src, R.RULES_CLI, sigma, 4, ratios, f"{name} fused_cull {f}", fit=False,
                      pairs_from_oracle=True) for c, f in ((fused, 1), (full, 0))]
    thr0 = None
    seen = []
    for (it, st, path, d, idx, ref, band), (_, sf, pf, df, idxf, _, _) in zip(*runs):
        dbg = fused.debug_counters()
        lanes = int(band.lanes(d).sum())
        seen.append((lanes, dbg["fz_band"], dbg["fz_recompute"], path))
        assert pf == 0 and np.array_equal(idx, idxf) and d.tobytes() == df.tobytes(), (name, it)
        assert st.valid == sf.valid == ref["valid"], (name, it)
        thr0 = st.threshold if it == 0 else thr0
        assert st.threshold == thr0, (name, it)
        if it == 0:
            assert path == 0 and dbg["fz_band"] == 0 and dbg["fz_recompute"] == 0, (name, seen)
            continue
        assert path == 1, (name, seen)
        assert band.delta == (0.25 if it == 1 else 0.05), (name, it)
        if flagged:
            assert dbg["fz_recompute"] == 1 and dbg["fz_band"] == 0, (name, seen)
        else:
            assert dbg["fz_recompute"] == 0 and dbg["fz_band"] == lanes, (name, seen)
        claim = want[0] if it == 1 else want[1]
        if claim == "many":
            assert lanes >= 32, (name, seen)
        elif claim is not None:
            assert lanes == claim, (name, seen)
    print(f"\n[band lanes] {name}: (reference lanes, fz_band, fz_recompute, path) per iterate {seen}")
    R.print_ratios(name, ratios)


# ---- d. degenerate residuals

@pytest.mark.parametrize("rules", [R.RULES_ENGINE, R.RULES_CLI])
@pytest.mark.parametrize("n_src", R.DEGENERATE_SOURCES)
def test_zero_residuals(icp, oracle, ctx, n_src, rules):
    """The source is target rows exactly: every moment is 0.0, every pair valid, H within its
    bound, and no band is ever set (a zero threshold): full passes throughout."""
    tgt, src = R.degenerate_case("zero", n_src)
    ratios = {}
    for it, st, path, d, idx, ref, band in _iterates(icp, oracle, ctx, tgt, src, rules, 3.0, 3, ratios,
                                                     f"zero {n_src}", fit=False, pairs_from_oracle=True):
        assert st.mean == 0.0 and st.std == 0.0 and st.threshold == 0.0 and st.rmse == 0.0, it
        assert st.valid == n_src and path == 0, it
    R.print_ratios(f"zero {n_src} rules {rules}", ratios)


@pytest.mark.parametrize("rules", [R.RULES_ENGINE, R.RULES_CLI])
@pytest.mark.parametrize("n_src", R.DEGENERATE_SOURCES)
def test_constant_dyadic_residuals(icp, oracle, ctx, n_src, rules):
    """Lattice queries all displaced by (0.5, 0, 0): mean 0.5 and std 0.0 exactly (the m2 clamp),
    the threshold 0.75 on an engine-rules first iterate and 0.5 otherwise, every pair valid (each
    residual equals the threshold from the second iterate on)."""
    tgt, src = R.degenerate_case("constant", n_src)
    ratios = {}
    for it, st, path, d, idx, ref, band in _iterates(icp, oracle, ctx, tgt, src, rules, 3.0, 3, ratios,
                                                     f"constant {n_src}", fit=False, pairs_from_oracle=True):
        assert np.all(d == 0.5) and st.mean == 0.5 and st.std == 0.0, it
        assert st.threshold == (0.75 if rules == R.RULES_ENGINE and it == 0 else 0.5), it
        assert st.valid == n_src and st.rmse == 0.5, it
        if it == 0:
            assert path == 0
        elif band.holds(st.threshold):
            assert path == 1, it  # every lane of every wave is a band lane on the threshold
    R.print_ratios(f"constant {n_src} rules {rules}", ratios)


@pytest.mark.parametrize("rules", [R.RULES_ENGINE, R.RULES_CLI])
@pytest.mark.parametrize("n_src", R.DEGENERATE_SOURCES)
def test_nearly_constant_residuals(icp, oracle, ctx, n_src, rules):
    """Residuals 0.5 + 2^-30 (i % 3): the variance is 2^-60 of the squared mean, so sum (d - c)^2
    - (sum (d - c))^2 / n cancels down to rounding (the neighbourhood of the m2 clamp) and the
    variance bound is the W^2 term alone; under the plain rule every lane of every wave lies in
    the band. Every pair is valid (the gap holds: the threshold lies 1.4 2^-30 above the largest)."""
    tgt, src = R.degenerate_case("near", n_src)
    ratios = {}
    for it, st, path, d, idx, ref, band in _iterates(icp, oracle, ctx, tgt, src, rules, 3.0, 3, ratios,
                                                     f"near {n_src}", fit=False, pairs_from_oracle=True):
        assert st.valid == n_src, it
        if it >= 1 and band.holds(st.threshold):
            assert path == 1, it
    R.print_ratios(f"nearly constant {n_src} rules {rules}", ratios)


@pytest.mark.parametrize("n_src", R.DEGENERATE_SOURCES)
def test_non_finite_queries(icp, oracle, ctx, n_src):
    """Three NaN rows: they are counted, nothing is valid (the mean is NaN), the extremes are those
    of the finite residuals (layer 1), and no band is set."""
    tgt, src = R.degenerate_case("nan", n_src)
    for it, st, path, d, idx, ref, band in _iterates(icp, oracle, ctx, tgt, src, R.RULES_ENGINE, 3.0, 3, {},
                                                     f"nan {n_src}", fit=False):
        assert ref is None and st.n_bad == 3 and st.valid == 0 and path == 0, it
        fin = np.isfinite(d)
        assert int(fin.sum()) == n_src - 3 and st.min_d == 0.5 and st.max_d == 0.5, it


# ---- e. other routes to the same record

@pytest.mark.parametrize("n_src", [3, 65, 4097])
def test_host_transport_group_of_three(icp, oracle, n_src):
    """Three members on one device over the host transport (one-query shards at n_src 3): the
    members' records are merged by the Chan formulas in k_finalize_moments and k_finalize_cov."""
    tgt, src = R.shape_pair(n_src, 5000)
    ratios = {}
    label = f"group n_src {n_src}"
    with icp.Context(devices=[0, 0, 0], transport=icp.XPORT_HOST) as g:
        for it, st, path, d, idx, ref, band in _iterates(icp, oracle, g, tgt, src, R.RULES_ENGINE, 3.0, 4, ratios,
                                                         label, members=3, pairs_from_oracle=True):
            pass
    R.print_ratios(label, ratios)


def _session(icp, tgt, src, iters, device_loop):
    with icp.Context(0, {"device_loop": device_loop}) as c:
        c.set_target(tgt, 10, 20, icp.RULES_ENGINE)
        c.set_source(src)
        rc, res, hist = c.run(icp.params_default(max_iterations=iters, tolerance=0.0, flags=icp.FLAG_NO_EARLY_STOP))
        assert rc == 0 and len(hist) == iters
        recs = [(h.valid_points, h.rmse, h.mean, h.std, h.threshold, tuple(h.transform)) for h in hist]
        return recs, hist, c.get_correspondences()[1]


@pytest.mark.parametrize("n_src", [65, 4097, 16385])
def test_session_records_host_and_device_loop(icp, n_src):
    """Six iterations as a host-driven session and as the device-resident loop (whose cull ends in
    k_merge_cov_last): equal records bit for bit; the host loop's first and last records against
    the reference (the residuals of the last search; a one-iteration session's for the first)."""
    tgt, src = R.shape_pair(n_src, 5000)
    host, hist, d_last = _session(icp, tgt, src, 6, 0)
    dev, _, d_dev = _session(icp, tgt, src, 6, 1)
    assert host == dev and d_last.tobytes() == d_dev.tobytes()
    one, _, d_first = _session(icp, tgt, src, 1, 0)
    assert one[0][:5] == host[0][:5]
    ratios = {}
    p = icp.params_default()
    R.check_session_record(hist[0], d_first, p.rules, 0, p.sigma_multiplier, ratios=ratios, label="first")
    R.check_session_record(hist[5], d_last, p.rules, 5, p.sigma_multiplier, ratios=ratios, label="last")
    R.print_ratios(f"session n_src {n_src}", ratios)
