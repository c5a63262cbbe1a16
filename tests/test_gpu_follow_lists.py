"""The half and wide lists of the certified search (csrc/follow_lists.h), filled to their per-wave
maximum at the smallest shapes.

Target: 20 000 points uniform in the unit cube; source: 64, 65 and 193 points uniform in the same
cube (one, one and three full waves, the last two with a wave of one query behind them). Every
full wave's search box then holds far more than kWaveCandCap = 1008 target points, and so does
each of its 32-query halves: every full wave overflows, pushes both halves when the half pass is on
(the halves list's capacity, two entries per wave), and every half overflows again. Each
configuration (overflow_halves x wide_pass) runs a source's first iterate (search_launch's lists in
the context's buffers, host query order) and then nn() of the same points (nn_core's own carve-up,
the caller's order). Indices and residuals must equal a search = REFERENCE context's bit for bit,
and the debug counters must show that the lists were used:

  overflow_waves  full waves, plus their two halves each when the half pass is on (a half that
                  overflows again is counted in the same slot)
  halves          2 x full waves when the half pass is on, else 0
  wide entries    wide_waves + wide_stack (an entry the wide pass finished + one it gave up after
                  its segment budget): the full waves, or their halves when the half pass is on;
                  0 when the wide pass is off

The boxes are checked on the CPU first (_assert_buckets_overflow, with the library's host query
order): over the three sources and both orders, the fewest target points inside the bounding box
of a full wave's queries is 5501, of a 32-query half's 2125 (n = 193, host order; the search box
is larger: it holds the queries' balls).
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TGT = 20_000
SIZES = (64, 65, 193)
CAND_CAP = 1008  # kWaveCandCap (csrc/kernels.h)


def _clouds(n):
    tgt = np.random.default_rng(20_000).random((N_TGT, 3))
    src = np.random.default_rng(1_000 + n).random((n, 3))
    return tgt, src


def _box_counts(tgt, q, width):
    """Target points inside the bounding box of each full run of `width` queries within a wave."""
    out = []
    for w in range(len(q) // 64):
        for h in range(64 // width):
            b = q[64 * w + width * h: 64 * w + width * (h + 1)]
            out.append(int(np.all((tgt >= b.min(0)) & (tgt <= b.max(0)), axis=1).sum()))
    return out


def _assert_buckets_overflow(icp, tgt, src):
    """Every full wave and every half of it, in the host query order (the iterate) and in the
    caller's order (nn), bounds more target points than a wave's candidate list takes."""
    for q in (src[icp.source_shard_order(src)], src):
        assert min(_box_counts(tgt, q, 64)) > CAND_CAP
        assert min(_box_counts(tgt, q, 32)) > CAND_CAP


@pytest.fixture(scope="module")
def reference(icp):
    """Per source size: the clouds and the reference-order kernel's answers (first iterate, nn)."""
    out = {}
    for n in SIZES:
        tgt, src = _clouds(n)
        _assert_buckets_overflow(icp, tgt, src)
        with icp.Context(0, icp.config(search=icp.SEARCH_REFERENCE, no_warmup=1)) as ctx:
            ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
            ctx.set_source(src)
            ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)
            answers = (*ctx.get_correspondences(), *ctx.nn(src))
        for a in (tgt, src, *answers):
            a.setflags(write=False)
        out[n] = (tgt, src, answers)
    return out


def _expected(full, halves_on, wide_on):
    return {"overflow_waves": full * (3 if halves_on else 1),
            "halves": 2 * full if halves_on else 0,
            "wide_entries": (2 * full if halves_on else full) if wide_on else 0}


@pytest.mark.parametrize("n,overflow_halves,wide_pass", list(itertools.product(SIZES, (0, 1), (0, 1))))
def test_lists_filled_to_capacity(icp, reference, n, overflow_halves, wide_pass):
    tgt, src, (ridx, rd, rnn_idx, rnn_d) = reference[n]
    cfg = icp.config(no_warmup=1, debug_counters=1, query_order=1, overflow_halves=overflow_halves,
                     wide_pass=wide_pass)
    with icp.Context(0, cfg) as ctx:
        ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
        ctx.set_source(src)
        ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)
        idx, d = ctx.get_correspondences()
        first = ctx.debug_counters()
        nn_idx, nn_d = ctx.nn(src)
        both = ctx.debug_counters()  # nn() adds to the iterate's counters
    np.testing.assert_array_equal(idx, ridx, err_msg="first iterate")
    np.testing.assert_array_equal(d, rd, err_msg="first iterate")
    np.testing.assert_array_equal(nn_idx, rnn_idx, err_msg="nn")
    np.testing.assert_array_equal(nn_d, rnn_d, err_msg="nn")
    want = _expected(n // 64, overflow_halves == 1, wide_pass == 0)
    for name, c, times in (("first iterate", first, 1), ("first iterate + nn", both, 2)):
        got = {"overflow_waves": c["overflow_waves"], "halves": c["halves"],
               "wide_entries": c["wide_waves"] + c["wide_stack"]}
        print(name, n, overflow_halves, wide_pass, got, "wide_waves", c["wide_waves"], "wide_stack", c["wide_stack"])
        assert got == {k: times * v for k, v in want.items()}, name
