"""The reference of tests/stats_reference.py and the inputs of tests/test_gpu_stats_shapes.py,
validated on the CPU alone: the longdouble sums against the exact ones, and for every input the
conditions the GPU tests lean on, with the correspondences of the CPU oracle (the transforms of
the later iterates are the oracle's best fits of the reference's valid pairs, which differ from
the GPU's in the last bits only; the GPU tests assert the gap condition again on their own data).
No GPU case leans on 3 sd >= 0.5 mean: the reference applies the engine's first-iterate rule as
cull_threshold states it, whichever branch it takes.
"""
from fractions import Fraction

import numpy as np
import pytest

import stats_reference as R


def _rel(got, want, scale=None):
    scale = abs(want) if scale is None else scale
    return 0.0 if got == want else float(abs(got - want) / scale)


@pytest.mark.parametrize("offset", [(0.0, 0.0, 0.0), tuple(R.GEO_OFFSET)])
def test_longdouble_reference_matches_exact_sums(offset):
    """8193 pairs, at the origin and at a georeferenced offset: every quantity to 2^-60 relative
    (an entry of H relative to the sum of the magnitudes of its terms' factors, m Ra Rb: an
    off-diagonal entry is itself a cancelling sum)."""
    n = 8193
    rng = np.random.default_rng(5)
    b = R.cloud(n, 21) + offset
    a = b + 0.05 * rng.normal(size=(n, 3)) + [0.1, -0.05, 0.02]
    d = np.sqrt(((a - b) ** 2).sum(1))
    tol = 2.0 ** -60
    me, ve = R.moments_ref(d, exact=True)
    ml, vl = R.moments_ref(d, exact=False)
    assert _rel(ml, me) <= tol and _rel(vl, ve) <= tol
    pe, pl = R.pairs_ref(d, a, b, exact=True), R.pairs_ref(d, a, b, exact=False)
    assert _rel(pl["rmse"], pe["rmse"]) <= tol
    Ra = [max(abs(Fraction(float(x)) - pe["ca"][k]) for x in a[:, k]) for k in range(3)]
    Rb = [max(abs(Fraction(float(x)) - pe["cb"][k]) for x in b[:, k]) for k in range(3)]
    for k in range(3):
        # a centroid relative to itself where it is away from zero, to the spread at the origin
        assert _rel(pl["ca"][k], pe["ca"][k], max(abs(pe["ca"][k]), Ra[k])) <= tol
        assert _rel(pl["cb"][k], pe["cb"][k], max(abs(pe["cb"][k]), Rb[k])) <= tol
        for l in range(3):
            assert _rel(pl["H"][k][l], pe["H"][k][l], n * Ra[k] * Rb[l]) <= tol
    assert _rel(pl["H"][0][0], pe["H"][0][0]) <= tol  # a diagonal entry: no cancellation


def test_threshold_rule_is_cull_threshold():
    m, s = Fraction(3, 4), Fraction(1, 8)
    assert R.threshold_rule(m, s, 3.0, 0, R.RULES_ENGINE) == m + m / 2       # 3 sd < mean / 2
    assert R.threshold_rule(m, s, 3.0, 1, R.RULES_ENGINE) == m + 3 * s
    assert R.threshold_rule(m, s, 3.0, 0, R.RULES_CLI) == m + 3 * s
    assert R.threshold_rule(m, 2 * s, 1.0, 0, R.RULES_ENGINE) == m + m / 2
    assert R.threshold_rule(m, 4 * s, 1.0, 0, R.RULES_ENGINE) == m + 4 * s


def test_exact_ties_are_recognised():
    """The threshold equals a residual in exact arithmetic: one residual, two at sigma 1, constant
    residuals. Nothing else counts as a tie."""
    assert R.reference([0.3], R.RULES_CLI, 0, 3.0)["tie"]
    assert not R.reference([0.3], R.RULES_ENGINE, 0, 3.0)["tie"]            # 1.5 mean
    assert R.reference([0.3, 0.7], R.RULES_CLI, 0, 1.0)["tie"]
    assert not R.reference([0.3, 0.7], R.RULES_CLI, 0, 3.0)["tie"]
    assert R.reference([0.5] * 65, R.RULES_ENGINE, 1, 3.0)["tie"]
    r = R.reference([0.3, 0.7, 0.9], R.RULES_CLI, 0, 1.0)
    assert not r["tie"] and r["gap"] and r["valid"] == 2


def _simulate(oracle, tgt, src, rules, sigma, iters, fit):
    """The iterates of a context on the CPU: yields (iteration, d, a, b, reference, band in force)."""
    tree = oracle.OracleTree(tgt)
    a = np.array(src)
    band = R.Band()
    for it in range(iters):
        idx, d = tree.nn(a, init_best=oracle.DBL_MAX)
        ref = R.reference(d, rules, it, sigma)
        yield it, d, a, tgt[idx], ref, band
        thr = float(ref["thr"])
        band.next(thr)
        if fit:
            v = d <= thr
            a = oracle.transform(oracle.best_fit(a[v], tgt[idx[v]]), a)


def _tie_expected(n_src, rules, sigma, it):
    """The shape cases whose threshold is a residual by algebra: a single residual under the plain
    rule (sd = 0), two residuals at sigma 1 (mean + sd is the larger one)."""
    plain = not (rules == R.RULES_ENGINE and it == 0)
    return (n_src == 1 and plain) or (n_src == 2 and sigma == 1.0 and plain)


@pytest.mark.parametrize("rules,sigma", R.RULE_CASES)
@pytest.mark.parametrize("n_src,n_tgt", R.SHAPE_CASES)
def test_shape_inputs_keep_the_gap(oracle, n_src, n_tgt, rules, sigma):
    tgt, src = R.shape_pair(n_src, n_tgt)
    for it, d, a, b, ref, band in _simulate(oracle, tgt, src, rules, sigma, 4, fit=True):
        if _tie_expected(n_src, rules, sigma, it):
            assert ref["tie"], it
        else:
            assert ref["gap"] and not ref["tie"], (it, float(ref["thr"]), float(ref["b_thr"]))


@pytest.mark.parametrize("name", R.BAND_CASES)
def test_band_inputs(oracle, name):
    """The constructed residuals: unambiguous matches, the gap on every iterate, and the band-lane
    counts the GPU test claims (the second iterate's 25 % band, the later iterates' 5 % band),
    with band lanes on both sides of the threshold where there are two or more."""
    tgt, src, sigma, want, flagged = R.band_case(name)
    seen = []
    for it, d, a, b, ref, band in _simulate(oracle, tgt, src, R.RULES_CLI, sigma, 4, fit=False):
        assert ref["gap"] and not ref["tie"]
        lanes = band.lanes(d)
        seen.append((int(lanes.sum()), int((d[lanes] <= float(ref["thr"])).sum())))
        if not flagged:
            assert d.max() <= 1.5 + 1e-12 and d.min() >= 0.5 - 1e-12
    assert seen[0] == (0, 0) and seen[2] == seen[3]
    for (count, below), claim in zip(seen[1:3], want):
        if claim == "many":
            assert count >= 32 + (0 if flagged else 1)
        elif claim is not None:
            assert count == claim
        if count >= 2 and claim is not None:
            assert 0 < below < count
    # the far query is far enough to leave its wave's search box: its radius against 3 x the mean
    if flagged:
        assert d.max() > 3.0 * d.mean() * 1.5


def test_band_cases_cover_every_band_size():
    sizes = set()
    for name in R.BAND_CASES:
        want = R.band_case(name)[3]
        if not R.band_case(name)[4]:
            sizes.update(w for w in want if w is not None)
    assert sizes >= {0, 1, 8, 9, "many"}


@pytest.mark.parametrize("n_src", R.DEGENERATE_SOURCES)
def test_degenerate_inputs(oracle, n_src):
    tgt, src = R.degenerate_case("zero", n_src)
    for it, d, a, b, ref, band in _simulate(oracle, tgt, src, R.RULES_ENGINE, 3.0, 3, fit=False):
        assert not d.any() and ref["tie"] and ref["thr"] == 0 and not band.ok
    tgt, src = R.degenerate_case("constant", n_src)
    for rules in (R.RULES_ENGINE, R.RULES_CLI):
        for it, d, a, b, ref, band in _simulate(oracle, tgt, src, rules, 3.0, 3, fit=False):
            assert np.all(d == 0.5) and ref["var"] == 0
            first = rules == R.RULES_ENGINE and it == 0
            assert ref["thr"] == (Fraction(3, 4) if first else Fraction(1, 2)) and ref["tie"] == (not first)
    tgt, src = R.degenerate_case("near", n_src)
    for rules in (R.RULES_ENGINE, R.RULES_CLI):
        for it, d, a, b, ref, band in _simulate(oracle, tgt, src, rules, 3.0, 3, fit=False):
            assert np.array_equal(d, 0.5 + 2.0 ** -30 * (np.arange(n_src) % 3)) and ref["gap"] and not ref["tie"]
            assert ref["valid"] == n_src
    tgt, src = R.degenerate_case("nan", n_src)
    assert int(np.isnan(src).any(1).sum()) == 3


@pytest.mark.parametrize("n_src", R.GEO_SOURCES)
def test_geo_inputs_are_the_shape_inputs_shifted(n_src):
    tgt, src = R.shape_pair(n_src, 5000)
    gtgt, gsrc = R.shape_pair(n_src, 5000, geo=True)
    np.testing.assert_allclose(gtgt - R.GEO_OFFSET, tgt, atol=1e-9)
    np.testing.assert_allclose(gsrc - R.GEO_OFFSET, src, atol=1e-9)
