"""High-precision reference of an iterate's statistics record, its derived error bounds, and the
inputs of tests/test_gpu_stats_shapes.py (a helper module, not a conftest; the inputs are also
validated on the CPU by tests/test_stats_reference.py).

Reference. Given the residuals d, the moved source a and the matches b = tgt[idx]:
  mean, var = sum (d - mean)^2 / n, sd = sqrt(var), threshold = cull_threshold (icp_common.h),
  over a valid set V: rmse = sqrt(sum d^2 / m), the centroids ca, cb, H = sum (a - ca)(b - cb)^T.
Up to 257 pairs the sums are exact (fractions.Fraction); above, centred two-pass sums in
np.longdouble of values shifted by the first one (an exact subtraction for the data used here),
converted to Fraction afterwards. Where np.longdouble has fewer than 63 mantissa bits the exact
sums are used throughout. Square roots are taken in longdouble (or of a float where it is no wider):
their relative error of 2^-63 is far below every bound's 2^-51 relative term.

Bounds (derived, u = 2^-53; the kernels sum values shifted by a data point, so each term is at
most the data's spread). n finite residuals, W = max_d - min_d; V the valid set, m = |V|;
Ra_k = max over V of |a_ik - ca_k| + the largest displacement of any source point since the
source's first iterate, Rb_l likewise for the matches b. (The displacement term: once a band is
set the pair shift is no longer taken from the iterate's data. cull_params copies fz_sh, the
shift of the iterate that set the first band, and band_next hands the same values on, so the
shift is a pair of the source's first iterate, which has since moved. Measured from the previous
iterate alone the term would not cover a shift that old; the difference is a few per cent of Ra
on the inputs used here.)
  mean       |dmean| <= 2^-52 ((n + 4) W + |mean|)
  variance   |std_gpu^2 - var| <= 2^-52 (2n + 16) W^2 + 2^-51 var      (W = 0 forces std == 0.0)
  threshold  the two above through the rule, dsd <= min(dvar / sd, sqrt(dvar)), + 2^-51 |thr|
             (both bounds of dsd hold: |x - y| (x + y) = |x^2 - y^2| with x + y >= sd, and
             |x - y|^2 <= |x^2 - y^2| for x, y >= 0; the minimum is the tighter statement)
  rmse       |drmse| <= (m + 8) 2^-53 rmse
  centroid   |dca_k| <= 2^-52 ((m + 4) 2 Ra_k + |ca_k|)
  H          |dH_kl| <= 8 (m + 8 + 4 members) 2^-52 m Ra_k Rb_l
"""
import functools
from fractions import Fraction

import numpy as np

RULES_ENGINE, RULES_CLI = 0, 1     # icp_hip.h ICP_RULES_*
EXACT_MAX = 257                    # pairs summed exactly
LD_OK = np.finfo(np.longdouble).nmant >= 63
_LD = np.longdouble
E52, E51, E53 = Fraction(1, 2 ** 52), Fraction(1, 2 ** 51), Fraction(1, 2 ** 53)
FIELDS = ("mean", "var", "threshold", "rmse", "centroid_src", "centroid_tgt", "H")


# ---- conversions

def _fr(x):
    """A float or longdouble as the Fraction it is (two floats hold a longdouble's 64 bits)."""
    if isinstance(x, Fraction):
        return x
    hi = float(x)
    lo = float(_LD(x) - _LD(hi)) if LD_OK else 0.0
    return Fraction(hi) + Fraction(lo)


def _ld(fr):
    """A Fraction rounded to longdouble (to a float where longdouble is no wider)."""
    hi = float(fr)
    if not LD_OK:
        return _LD(hi)
    return _LD(hi) + _LD(float(fr - Fraction(hi)))


def _sqrt(fr):
    return _fr(np.sqrt(_ld(fr))) if fr > 0 else Fraction(0)


def _exact(n, exact):
    if not LD_OK:
        return True
    return n <= EXACT_MAX if exact is None else exact


# ---- the reference

def moments_ref(d, exact=None):
    """(mean, var) of the finite residuals d as Fractions."""
    d = np.asarray(d, np.float64)
    n = len(d)
    if _exact(n, exact):
        f = [Fraction(float(x)) for x in d]
        mean = sum(f) / n
        return mean, sum((x - mean) ** 2 for x in f) / n
    c = d[0]
    x = d.astype(_LD) - _LD(c)           # exact: the residuals lie within 2^11 ulps' range of each other
    m1 = x.sum() / n
    y = x - m1
    e = y.sum() / n                      # the rounding of m1, taken back out (corrected two-pass)
    var = (y * y).sum() / n - e * e
    return Fraction(float(c)) + _fr(m1) + _fr(e), _fr(var)


def threshold_rule(mean, sd, sigma, iteration, rules):
    """cull_threshold of icp_common.h on Fractions."""
    sigma = Fraction(float(sigma))
    if rules == RULES_ENGINE and iteration == 0:
        return mean + max(sigma * sd, mean / 2)
    return mean + sigma * sd


def pairs_ref(d, a, b, exact=None):
    """rmse, the centroids and H of the given pairs as Fractions: dict(m, rmse, ca, cb, H)."""
    d, a, b = np.asarray(d, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = len(d)
    if _exact(m, exact):
        fa = [[Fraction(float(v)) for v in row] for row in a]
        fb = [[Fraction(float(v)) for v in row] for row in b]
        ca = [sum(r[k] for r in fa) / m for k in range(3)]
        cb = [sum(r[k] for r in fb) / m for k in range(3)]
        H = [[sum((ra[k] - ca[k]) * (rb[l] - cb[l]) for ra, rb in zip(fa, fb)) for l in range(3)] for k in range(3)]
        ss = sum(Fraction(float(x)) ** 2 for x in d) / m
    else:
        # columns as contiguous vectors: numpy sums those pairwise (error ~ log2(m) 2^-64, not m 2^-64)
        xa = np.ascontiguousarray((a.astype(_LD) - a[0].astype(_LD)).T)
        xb = np.ascontiguousarray((b.astype(_LD) - b[0].astype(_LD)).T)
        ma, mb = [x.sum() / m for x in xa], [x.sum() / m for x in xb]
        ya = [np.ascontiguousarray(x - c) for x, c in zip(xa, ma)]
        yb = [np.ascontiguousarray(x - c) for x, c in zip(xb, mb)]
        ea, eb = [y.sum() / m for y in ya], [y.sum() / m for y in yb]
        Hl = np.array([[(ya[k] * yb[l]).sum() - m * ea[k] * eb[l] for l in range(3)] for k in range(3)])
        ca = [Fraction(float(a[0][k])) + _fr(ma[k]) + _fr(ea[k]) for k in range(3)]
        cb = [Fraction(float(b[0][k])) + _fr(mb[k]) + _fr(eb[k]) for k in range(3)]
        H = [[_fr(Hl[k, l]) for l in range(3)] for k in range(3)]
        x = d.astype(_LD)
        ss = _fr((x * x).sum() / m)
    return dict(m=m, rmse=_sqrt(ss), ca=ca, cb=cb, H=H)


# ---- the band of the fused cull (reduce_kernels.hip band_next), in floats as the kernel has it

class Band:
    """lo, hi of the band the next iterate's search sums below; ok False: none (a new source, a
    threshold that is not positive and finite)."""

    def __init__(self):
        self.ok, self.thr, self.lo, self.hi, self.delta = False, 0.0, 0.0, 0.0, 0.0

    def holds(self, thr, margin=1e-9):
        """The threshold lies inside the band, by more than a relative margin."""
        return self.ok and self.lo * (1 + margin) <= thr <= self.hi * (1 - margin)

    def lanes(self, d):
        """The band lanes of the residuals d: lo < d <= hi."""
        d = np.asarray(d)
        return (d > self.lo) & (d <= self.hi) if self.ok else np.zeros(len(d), bool)

    def next(self, thr):
        delta = 0.25
        if self.ok and self.thr > 0.0:
            delta = min(0.5, 2.0 * abs(thr / self.thr - 1.0) + 0.05)
        self.ok = bool(np.isfinite(thr) and thr > 0.0)
        self.thr, self.lo, self.hi, self.delta = thr, thr * (1.0 - delta), thr * (1.0 + delta), delta


# ---- the checks of one record

def _ratio(ratios, field, err, bound):
    r = 0.0 if err == 0 else (float("inf") if bound == 0 else float(err / bound))
    if ratios is not None:
        ratios[field] = max(ratios.get(field, 0.0), r)
    return r


def reference(d, rules, iteration, sigma):
    """The reference's mean, var, sd, threshold (Fractions), the threshold's error bound and the
    gap condition of the residuals d (all finite): no residual within that bound of the threshold.
    tie: the threshold equals a residual in exact arithmetic (zero or constant residuals, a single
    residual, two residuals at sigma 1: mean + sd is then the larger one)."""
    d = np.asarray(d, np.float64)
    n = len(d)
    mean, var = moments_ref(d)
    sd = _sqrt(var)
    thr = threshold_rule(mean, sd, sigma, iteration, rules)
    W = Fraction(float(d.max())) - Fraction(float(d.min()))
    b_mean = E52 * ((n + 4) * W + abs(mean))
    b_var = E52 * (2 * n + 16) * W * W + E51 * var
    b_sd = _sqrt(b_var) * (1 + E52)
    if var > 0:
        b_sd = min(b_sd, b_var / sd * (1 + E52))
    s = Fraction(float(sigma))
    if rules == RULES_ENGINE and iteration == 0:
        b_thr = b_mean + max(s * b_sd, b_mean / 2) + E51 * abs(thr)
    else:
        b_thr = b_mean + s * b_sd + E51 * abs(thr)
    thr_f = float(thr)
    near = np.abs(d - thr_f) <= float(b_thr) * 1.0000001 + abs(thr_f) * 2.0 ** -52
    gap = not any(abs(Fraction(float(x)) - thr) <= b_thr for x in d[near])
    # an exact tie: (d_i - mean)^2 == (thr - mean)^2 with the exact variance, no square root taken
    if rules == RULES_ENGINE and iteration == 0 and mean * mean / 4 >= s * s * var:
        t2 = mean * mean / 4
    else:
        t2 = s * s * var
    tie = any(Fraction(float(x)) >= mean and (Fraction(float(x)) - mean) ** 2 == t2 for x in d[near])
    valid = int(sum(1 for x in d[near] if Fraction(float(x)) <= thr) + np.count_nonzero((d <= thr_f) & ~near))
    return dict(n=n, mean=mean, var=var, sd=sd, thr=thr, W=W, b_mean=b_mean, b_var=b_var, b_thr=b_thr, gap=gap,
                tie=tie, valid=valid)


def check_record(st, d, a, b, rules, iteration, sigma, *, a_first=None, b_first=None, members=1, ratios=None,
                 layer3=True, label=""):
    """The three layers on one record `st` (icp_iter_stats fields as attributes): the reported
    residuals d, the moved source a, the matches b = tgt[idx]; a_first, b_first the same arrays of
    the first iterate on this source (None: this is the first). Returns the reference (reference()), or
    None for residuals that are not all finite (layer 1 only)."""
    d, a, b = np.asarray(d, np.float64), np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = len(d)
    fin = np.isfinite(d)
    # 1. self-consistency, exact
    assert st.n == n, label
    assert st.valid == int(np.count_nonzero(d <= st.threshold)), label
    assert st.n_bad == int(np.count_nonzero(~fin)), label
    if fin.any():
        assert st.min_d == d[fin].min() and st.max_d == d[fin].max(), label
    if not fin.all():
        return None
    # 2. accuracy
    ref = reference(d, rules, iteration, sigma)
    fails = []

    def cmp(field, got, want, bound):
        err = abs(Fraction(float(got)) - want)
        if _ratio(ratios, field, err, bound) > 1.0:
            fails.append(f"{field}: got {float(got)!r}, reference {float(want)!r}, error {float(err):.3e} > bound "
                         f"{float(bound):.3e}")

    cmp("mean", st.mean, ref["mean"], ref["b_mean"])
    err = abs(Fraction(float(st.std)) ** 2 - ref["var"])
    if _ratio(ratios, "var", err, ref["b_var"]) > 1.0:
        fails.append(f"var: std {st.std!r}, reference sd {float(ref['sd'])!r}, error {float(err):.3e} > bound "
                     f"{float(ref['b_var']):.3e}")
    cmp("threshold", st.threshold, ref["thr"], ref["b_thr"])
    v = d <= st.threshold
    m = int(v.sum())
    assert m > 0, label
    p = pairs_ref(d[v], a[v], b[v])
    cmp("rmse", st.rmse, p["rmse"], (m + 8) * E53 * p["rmse"])
    da = 0.0 if a_first is None else float(np.sqrt(((a - a_first) ** 2).sum(1)).max())
    db = 0.0 if b_first is None else float(np.sqrt(((b - b_first) ** 2).sum(1)).max())
    Ra = [max(abs(Fraction(float(x)) - p["ca"][k]) for x in (a[v][:, k].min(), a[v][:, k].max())) + Fraction(da)
          for k in range(3)]
    Rb = [max(abs(Fraction(float(x)) - p["cb"][k]) for x in (b[v][:, k].min(), b[v][:, k].max())) + Fraction(db)
          for k in range(3)]
    for k in range(3):
        cmp("centroid_src", st.centroid_src[k], p["ca"][k], E52 * ((m + 4) * 2 * Ra[k] + abs(p["ca"][k])))
        cmp("centroid_tgt", st.centroid_tgt[k], p["cb"][k], E52 * ((m + 4) * 2 * Rb[k] + abs(p["cb"][k])))
    for k in range(3):
        for l in range(3):
            cmp("H", st.H[3 * k + l], p["H"][k][l], 8 * (m + 8 + 4 * members) * E52 * m * Ra[k] * Rb[l])
    assert not fails, f"{label}: " + "; ".join(fails)
    # 3. the exact valid count, where no residual lies within the threshold's bound of the threshold
    if layer3:
        assert ref["gap"] or ref["tie"], f"{label}: a residual within {float(ref['b_thr']):.3e} of the threshold"
        if ref["gap"]:
            assert st.valid == ref["valid"], label
    return ref


def check_session_record(h, d, rules, iteration, sigma, *, ratios=None, label=""):
    """Layers 1 and 2 on a session's history record h (mean, std, threshold, valid_points, rmse)
    with the residuals d of its iteration."""
    d = np.asarray(d, np.float64)
    assert np.isfinite(d).all(), label
    v = d <= h.threshold
    assert h.valid_points == int(v.sum()), label
    ref = reference(d, rules, iteration, sigma)
    m = int(v.sum())
    rmse = _sqrt(sum(Fraction(float(x)) ** 2 for x in d[v]) / m) if m <= EXACT_MAX or not LD_OK else \
        pairs_ref(d[v], np.zeros((m, 3)), np.zeros((m, 3)))["rmse"]
    checks = [("mean", Fraction(h.mean), ref["mean"], ref["b_mean"]),
              ("var", Fraction(h.std) ** 2, ref["var"], ref["b_var"]),
              ("threshold", Fraction(h.threshold), ref["thr"], ref["b_thr"]),
              ("rmse", Fraction(h.rmse), rmse, (m + 8) * E53 * rmse)]
    fails = [f"{f}: error {float(abs(g - w)):.3e} > bound {float(b):.3e}" for f, g, w, b in checks
             if _ratio(ratios, f, abs(g - w), b) > 1.0]
    assert not fails, f"{label}: " + "; ".join(fails)
    return ref


def print_ratios(name, ratios):
    print(f"\n[stats ratios] {name}: " + " ".join(f"{k}={ratios.get(k, 0.0):.3g}" for k in FIELDS))


# ---- the inputs

def motion():
    """1 degree about z and a 0.1 shift."""
    t = np.deg2rad(1.0)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]
    T[:3, 3] = [0.1, -0.05, 0.02]
    return T


def cloud(n, seed):
    """test_gpu_device_clouds._cloud."""
    return np.random.default_rng(seed).normal(size=(n, 3)) * [20.0, 20.0, 5.0]


GEO_OFFSET = np.array([4e5, 5e6, 100.0])
SHAPE_SOURCES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4095, 4096, 4097, 8193, 16385]
SHAPE_CASES = [(n, 5000) for n in SHAPE_SOURCES] + [(n, t) for t in (1, 11) for n in (1, 65, 4097)]
RULE_CASES = [(RULES_ENGINE, 3.0), (RULES_ENGINE, 1.0), (RULES_CLI, 3.0), (RULES_CLI, 1.0)]
GEO_SOURCES = [65, 4097]


@functools.lru_cache(maxsize=None)
def shape_pair(n_src, n_tgt, geo=False):
    """(target, source): the target is cloud(n_tgt, 1); the source its rows (drawn with
    replacement) plus 0.05 noise, moved by motion(). geo: both plus GEO_OFFSET. Shared: read only."""
    tgt = cloud(n_tgt, 1)
    rng = np.random.default_rng(1000 + n_src)
    src = tgt[rng.integers(0, n_tgt, n_src)] + 0.05 * rng.normal(size=(n_src, 3))
    T = motion()
    src = src @ T[:3, :3].T + T[:3, 3]
    if geo:
        tgt, src = tgt + GEO_OFFSET, src + GEO_OFFSET
    tgt, src = np.ascontiguousarray(tgt), np.ascontiguousarray(src)
    tgt.setflags(write=False)
    src.setflags(write=False)
    return tgt, src


def lattice(side):
    """side^3 points of spacing 8, in a fixed shuffled order."""
    g = np.arange(side) * 8.0
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(p[np.random.default_rng(7).permutation(len(p))])


def lattice_queries(tgt, residuals, far=None):
    """Query i = lattice point i displaced along x by residuals[i] (at most 1.5 of a spacing of 8:
    the match is unambiguous). far = (lane, D): that query lies D below the lattice's corner along
    x instead, outside the lattice (its match is the corner)."""
    q = tgt[: len(residuals)].copy()
    q[:, 0] += residuals
    if far is not None:
        lane, D = far
        q[lane] = tgt[np.argmin(tgt.sum(1))] - [D, 0.0, 0.0]
    return q


def _band_residuals(n, k, seed):
    """n residuals in [0.5, 1.5] whose k lanes closest to mean + sd lie within 4 % of it, on both
    sides (k >= 2), and every other lane more than 25 % away: a low cluster at 0.5 .. 0.62 and a
    high one at 1.5. The k lanes follow the threshold in a fixed-point iteration."""
    rng = np.random.default_rng(seed)
    n_hi = n // 8
    low = rng.uniform(0.5, 0.62, n - k - n_hi)
    e = np.linspace(-0.04, 0.04, k + 2)[1:-1] if k > 1 else np.array([-0.02] * k)
    e = e + 0.003 * (np.abs(e) < 0.002)  # none on the threshold itself
    t = 1.0
    for _ in range(60):
        r = np.concatenate([low, t * (1 + e), np.full(n_hi, 1.5)])
        t = r.mean() + r.std()
    return rng.permutation(r)


@functools.lru_cache(maxsize=None)
def band_case(name):
    """(target, source, sigma, expected band lanes of the second iterate (a 25 % band) and of the
    later ones (5 %), flagged): constructed residuals on a single-wave source, identity
    transforms, CLI rules. None for a count: not claimed (asserted against the reference only)."""
    tgt = lattice(5)
    far, sigma = None, 1.0
    if name == "uniform64":        # about half the lanes within 25 % of mean + sd
        r, want = np.random.default_rng(11).uniform(0.5, 1.5, 64), ("many", None)
    elif name == "uniform40":      # a partial wave
        r, want = np.random.default_rng(12).uniform(0.5, 1.5, 40), (None, None)
    elif name == "far64":          # lane 17 leaves the wave search: the cull recomputes the wave
        r, want, far = np.random.default_rng(13).uniform(0.5, 1.5, 64), (None, None), (17, 40.0)
    elif name == "far40":
        r, want, far = np.random.default_rng(14).uniform(0.5, 1.5, 40), (None, None), (3, 40.0)
    elif name == "farband64":      # flagged, with band lanes: a nearer far query and a low threshold
        r, want, far, sigma = np.random.default_rng(15).uniform(0.5, 1.5, 64), ("many", None), (17, 12.0), 0.1
    elif name == "farband40":      # flagged: 12 band lanes (a tree), then 8 (lane by lane)
        r, want, far, sigma = np.random.default_rng(58).uniform(0.5, 1.5, 40), (12, 8), (3, 12.0), 0.1
    else:                          # band<k>_<n>
        k, n = (int(s) for s in name[4:].split("_"))
        r, want = _band_residuals(n, k, 100 + k), (k, k)
    src = lattice_queries(tgt, r, far)
    for arr in (tgt, src):
        arr.setflags(write=False)
    return tgt, src, sigma, want, far is not None


BAND_CASES = ["band0_64", "band1_64", "band8_64", "band9_64", "uniform64", "band0_40", "band1_40", "band8_40",
              "band9_40", "uniform40", "far64", "far40", "farband64", "farband40"]

DEGENERATE_SOURCES = [65, 4097]


@functools.lru_cache(maxsize=None)
def degenerate_case(kind, n_src):
    """(target, source). zero: the source is target rows exactly; constant: lattice queries all
    displaced by (0.5, 0, 0); near: by 0.5 + 2^-30 (i % 3), residuals that differ in their last
    23 bits only; nan: the constant source with three NaN rows."""
    tgt = lattice(17)  # 4913 points
    src = tgt[:n_src].copy()
    if kind != "zero":
        src[:, 0] += 0.5
    if kind == "near":
        src[:, 0] += 2.0 ** -30 * (np.arange(n_src) % 3)  # exact: the coordinates are below 2^8
    if kind == "nan":
        src[[5, n_src // 2, n_src - 1]] = np.nan
    tgt.setflags(write=False)
    src.setflags(write=False)
    return tgt, src
