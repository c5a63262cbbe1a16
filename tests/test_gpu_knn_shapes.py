"""icp_hip_knn at the shapes where its launch changes (knn_kernels.hip, ctx_plane.cpp), indices and
fl(d2) by bytes against plane_fixtures.knn_brute: the three block tiers of knn_block_threads with
their exact 64 KiB edges, trees of 20, 40 and 60 levels, query counts around a block, k equal to
the target size, non-finite and overflowing queries, georeferenced clouds, and one call longer than
the 2^22-query slice of knn_core in the host and the device form."""
import numpy as np
import pytest

import plane_fixtures as pf
import plane_reference as R

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    gi, gd = got
    wi, wd = want
    assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == wi.shape
    assert np.array_equal(gi, wi), f"{what}: {np.count_nonzero(gi != wi)} indices differ"
    assert gd.tobytes() == np.ascontiguousarray(wd).tobytes(), what


def _cols(want, rows, k):
    return want[0][rows, :k].copy(), want[1][rows, :k].copy()


@pytest.fixture(scope="module")
def blob(icp):
    tgt, src, _ = icp.synth_pair(20000, 513)  # 513 queries: two 256-thread blocks and one thread
    return tgt, src, pf.knn_brute(src, tgt, 32)  # the first k columns are the answer for every k <= 32


@pytest.fixture(scope="module")
def copies():
    """The deep-copies target with 40 + 473 queries (the copies, then points around them) and the
    brute-force answer at k = 32; the same whatever depth the tree is built to."""
    tgt, where = R.deep_copies()
    rng = np.random.default_rng(17)
    q = np.concatenate([tgt[where], tgt[where[0]] + rng.normal(size=(473, 3)) * np.logspace(-12, 0, 473)[:, None]])
    want = pf.knn_brute(q, tgt, 32)
    assert (want[1][:40] == 0.0).all() and np.array_equal(want[0][0], np.sort(where)[:32])
    return tgt, q, want


@pytest.fixture(scope="module")
def ctxs(icp, blob, copies):
    """One context per target, made when first asked for: ctxs("blob"), and ctxs(20), ctxs(40),
    ctxs(60) for the copies in trees of that many levels."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = icp.Context(0)
            if name == "blob":
                made[name].set_target(blob[0])
            else:
                made[name].set_target(copies[0], max_depth=name)
        return made[name]

    try:
        yield get
    finally:
        for c in made.values():
            c.close()


TIER_CASES = [  # (target, k, block threads, bytes per thread where the edge is exact)
    ("blob", 7, 256, None), (20, 8, 256, 256), (20, 9, 128, None), (40, 16, 128, 512), (40, 17, 64, None),
    (20, 32, 64, None), (40, 32, 64, None), (60, 32, 64, 864)]


@pytest.mark.parametrize("name,k,bs,per", TIER_CASES, ids=[f"{c[0]}-k{c[1]}-bs{c[2]}" for c in TIER_CASES])
def test_block_tiers(icp, ctxs, blob, copies, name, k, bs, per):
    ctx = ctxs(name)
    _, q, want = blob if name == "blob" else copies
    info = ctx.target_info()
    if name != "blob":
        assert info["max_depth"] == name and info["stack_levels"] == name
    got_per, got_bs = R.knn_tier(info["stack_levels"], k)
    assert got_bs == bs and got_per * bs <= 65536, (info, got_per)
    if per is not None:
        assert got_per == per
    for n in (1, bs - 1, bs, bs + 1, 2 * bs + 1):
        _same(ctx.knn(q[:n], k), _cols(want, slice(0, n), k), f"n = {n}")
    # the last rows alone: the copies are not always the first block
    _same(ctx.knn(q[-(bs + 1):], k), _cols(want, slice(len(q) - bs - 1, len(q)), k), "tail")
    n = 2 * bs + 1
    wi, wd = _cols(want, slice(0, n), k)
    with ctx.to_device(q[:n]) as d_q, ctx.device_buffer(4 * n * k) as b_idx, ctx.device_buffer(8 * n * k) as b_d2:
        ctx.knn_device(d_q, n, k, b_idx, b_d2)
        assert b_idx.download(np.int32).tobytes() == wi.tobytes()
        assert b_d2.download(np.float64).tobytes() == wd.tobytes()


@pytest.mark.parametrize("n_tgt", [1, 5, 32])
def test_k_equal_to_the_target_size(icp, n_tgt):
    tgt = np.random.default_rng(30 + n_tgt).normal(size=(n_tgt, 3))
    q = np.concatenate([tgt, np.random.default_rng(31).normal(size=(70, 3))])
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        want = pf.knn_brute(q, tgt, n_tgt)
        assert (np.sort(want[0], 1) == np.arange(n_tgt)).all()  # every point, in order of distance
        _same(ctx.knn(q, n_tgt), want)


def test_non_finite_and_overflowing_queries(ctxs, blob):
    tgt, src, _ = blob
    k = 4
    rows, kind = [], []
    for c in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            r = src[len(rows)].copy()
            r[c] = bad
            rows += [r, src[100 + len(rows)]]
            kind += ["bad", "fine"]
        for big in (1e200, -1e200):
            r = src[len(rows)].copy()
            r[c] = big
            rows += [r, src[100 + len(rows)]]
            kind += ["over", "fine"]
    rows.append(np.array([1e200, -1e200, 1e200]))
    kind.append("over")
    q, kind = np.array(rows), np.array(kind)
    ctx = ctxs("blob")
    gi, gd = ctx.knn(q, k)
    bad = kind == "bad"
    assert (gi[bad] == -1).all() and np.isnan(gd[bad]).all()
    with np.errstate(over="ignore"):
        wi, wd = pf.knn_brute(q[~bad], tgt, k)
    over = kind[~bad] == "over"
    assert np.array_equal(wi[over], np.tile(np.arange(k, dtype=np.int32), (over.sum(), 1))) and np.isinf(wd[over]).all()
    assert np.isfinite(wd[~over]).all()
    _same((gi[~bad], gd[~bad]), (wi, wd))
    # the same rows alone and through the device form
    n = len(q)
    with ctx.to_device(q) as d_q, ctx.device_buffer(4 * n * k) as b_idx, ctx.device_buffer(8 * n * k) as b_d2:
        ctx.knn_device(d_q, n, k, b_idx, b_d2)
        assert b_idx.download(np.int32).tobytes() == gi.tobytes()
        assert b_d2.download(np.float64).tobytes() == gd.tobytes()  # NaN rows included: one NaN pattern


@pytest.mark.parametrize("where", ["geo", "far"])
def test_georeferenced(icp, blob, where):
    tgt, q = blob[0] + R.OFFSETS[where], blob[1] + R.OFFSETS[where]
    want = pf.knn_brute(q, tgt, 32)
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        for k in (1, 7, 32):
            _same(ctx.knn(q, k), _cols(want, slice(None), k), f"k = {k}")


def test_more_queries_than_a_slice(ctxs, blob):
    """2^22 + 65 queries, k = 2: the second slice of knn_core starts at query 2^22 and writes one
    64-thread wave and one thread more; 1021 distinct rows repeated, so the brute force stays small."""
    tgt, src, want = blob
    ctx = ctxs("blob")
    k, n = 2, (1 << 22) + 65
    rep = np.arange(n) % 1021
    base = np.concatenate([src, src[:508] + 0.25])
    wb = pf.knn_brute(base[513:], tgt, k)
    wi = np.concatenate([want[0][:, :k], wb[0]])[rep]
    wd = np.concatenate([want[1][:, :k], wb[1]])[rep]
    q = base[rep]
    gi, gd = ctx.knn(q, k)
    assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.int64), wd.view(np.int64))
    del gi, gd
    with ctx.to_device(q) as d_q, ctx.device_buffer(4 * n * k) as b_idx, ctx.device_buffer(8 * n * k) as b_d2:
        ctx.knn_device(d_q, n, k, b_idx, b_d2)
        assert np.array_equal(b_idx.download(np.int32).reshape(n, k), wi)
        assert np.array_equal(b_d2.download(np.float64).view(np.int64).reshape(n, k), wd.view(np.int64))
