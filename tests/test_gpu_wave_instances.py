"""Every k_nn_wave instance against the reference-order kernel, bit for bit.

The wave search is compiled in 48 instances (transform x scan groups x certificate x debug counters
x cache mode); the other suites reach them piecemeal and at 300k to 1M points. Here each
combination of scan_groups x debug_counters x certify_prev x candidate_cache runs, on 20k points
(313 waves), the sequence that visits its instances: a first iterate without a transform, two
iterates with the fitted transform, an nn() of the moved source (an untransformed search after a
search) and a further iterate without a transform. Indices and residuals must equal those of a
search = REFERENCE context at every step (that kernel equals the CPU oracle: test_gpu_parity.py).
No tolerance, nothing skipped. The wide, half and fp64 re-scan paths stay with the 1M tests.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 20_000


def _steps(icp, ctx, tgt, src, transforms, after=None):
    """The sequence's (indices, residuals) per step; transforms: the two fitted ones, or None to
    fit them from this context's own statistics (the reference run). after(ctx): called once each
    step has run (test_gpu_geo_search.py reads the moved source and the counters there)."""
    out, fitted = [], []
    after = after or (lambda ctx: None)
    ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
    ctx.set_source(src)
    st = ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)
    out.append(ctx.get_correspondences())
    after(ctx)
    for k in (1, 2):
        T = icp.best_fit_from_stats(st) if transforms is None else transforms[k - 1]
        fitted.append(T)
        st = ctx.iterate(T, k, icp.RULES_ENGINE, 3.0)
        out.append(ctx.get_correspondences())
        after(ctx)
    out.append(ctx.nn(ctx.get_source()))
    after(ctx)
    ctx.iterate(None, 3, icp.RULES_ENGINE, 3.0)
    out.append(ctx.get_correspondences())
    after(ctx)
    return out, fitted


@pytest.fixture(scope="module")
def reference_run(icp):
    tgt, src, _ = icp.synth_pair(N)
    with icp.Context(0, icp.config(search=icp.SEARCH_REFERENCE, no_warmup=1)) as ctx:
        steps, fitted = _steps(icp, ctx, tgt, src, None)
    for idx, d in steps:
        idx.setflags(write=False)
        d.setflags(write=False)
    return tgt, src, steps, fitted


@pytest.mark.parametrize("scan_groups,debug_counters,certify_prev,candidate_cache",
                         list(itertools.product((1, 2, 4), (0, 1), (0, 3), (0, 1))))
def test_every_wave_instance_equals_reference(icp, reference_run, scan_groups, debug_counters, certify_prev,
                                              candidate_cache):
    tgt, src, ref, fitted = reference_run
    cfg = icp.config(no_warmup=1, scan_groups=scan_groups, debug_counters=debug_counters, certify_prev=certify_prev,
                     candidate_cache=candidate_cache)
    with icp.Context(0, cfg) as ctx:
        got, _ = _steps(icp, ctx, tgt, src, fitted)
    names = ("first iterate", "iterate 1 (transform)", "iterate 2 (transform)", "nn of the moved source",
             "iterate without a transform")
    for name, (idx, d), (ridx, rd) in zip(names, got, ref):
        np.testing.assert_array_equal(idx, ridx, err_msg=name)
        np.testing.assert_array_equal(d, rd, err_msg=name)
