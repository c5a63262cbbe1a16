"""The structures the searches derive from the resident octree, read back with
icp_hip_copy_target_aux (tight boxes, cell tables) and target_separation (the copy flag, the sign
bit of TgtPt::sep), against plain numpy references computed from the host copy of the tree
(copy_target: node records and leaf-ordered points; the tree itself is pinned bit for bit by
test_gpu_octree_build.py). End-to-end parity practically never notices these going wrong: a box
rounded inwards by an ulp prunes the true neighbour only on a tie within that ulp, a wrong table
entry matters only to a query whose box starts there, a wrongly flagged point is silently never an
answer.

  * Tight boxes (k_tight_boxes). A node's point range is a leaf's own range, an inner node's the
    span of its children. lo is the fp64 minimum over the range rounded towards -inf to fp32, hi the
    maximum rounded towards +inf, exactly (an exactly representable extreme must not widen; a zero
    of either sign is a zero). Containment, every point of the range inside the box compared in
    fp64, is asserted on its own so that a failure names the property that broke.
  * Copy flags (k_mark_copies): a point is flagged iff one of the kCopyWindow = 32 points before it
    in leaf order has equal x, y and z (-0.0 == 0.0), with certify_prev on and off.
  * Cell tables (k_cell_table). (a) Every entry of every level against a plain descent of the host
    copy: (id << 5) | depth of the node at depth l or of the leaf above it, -1 when a child on the
    path is absent. (b) From the points alone: a point's cell at level l by the reference's midpoint
    rule from the root box (octree.cpp:97-108: mid = (min + max) / 2, x > mid sets bit 0, y bit 1,
    z bit 2; level 1 in the top three bits) must name a node whose range holds the point. An entry
    no point reaches is -1, or, below a leaf that ends above level l, that leaf (the documented
    rule: the table names the leaf for all of its cell, and the leaf's own cell is reached).
    The deepest level follows cell_table_depth's rule from the leaf count and the deepest inner
    node; without cell_starts there are no tables.

Both builders: the device one, and the host one through max_depth = 22 (and octree_builder = HOST
for the shallow tree).
"""
import functools

import numpy as np
import pytest

from conftest import KAT_CASES

pytestmark = pytest.mark.gpu

LEAF = np.uint32(0x80000000)
COPY_WINDOW = 32
SHAPES = ["rounded", "identical", "two", "plane", "slab_geo"]
# (max_points, max_depth, host builder)
TREES = [(10, 20, False), (3, 2, False), (64, 20, False), (10, 22, True), (3, 2, True), (64, 22, True)]
POP8 = np.array([bin(k).count("1") for k in range(256)], np.int32)
TINY = 2.0 ** -149


@functools.lru_cache(maxsize=None)
def _shape(name):
    rng = np.random.default_rng(7)
    if name == "rounded":  # many exact duplicates and points on split planes (the largest cloud here)
        t = np.round(rng.normal(size=(40_000, 3)), 1)
    elif name == "identical":  # one leaf at max depth holding every point
        t = np.ones((5000, 3)) * 0.25
    elif name == "two":  # the root is a leaf
        t = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    elif name == "plane":  # degenerate axis: z constant
        t = np.c_[rng.uniform(-1, 1, size=(30_000, 2)), np.zeros(30_000)]
    elif name == "slab_geo":  # georeferenced: the fp32 ulp is 0.03 m in x and 0.5 m in y
        t = np.c_[rng.uniform(0, 20, size=(5000, 2)), rng.normal(size=5000) * 0.05] + [4.5e5, 5.4e6, 300.0]
    elif name in ("edges", "edges_far"):
        # the edges of the outward rounding: fp32-exact coordinates, zeros of both signs, fp64
        # subnormals (which round out to +-2^-149), other values, and (edges_far) a point at 3e10
        tiny = rng.choice([0.0, -0.0, 1e-320, -1e-320, 5e-324, -5e-324], size=(12, 3))
        tiny[0], tiny[1] = [-1e-320] * 3, [1e-320] * 3
        exact = rng.uniform(1, 3, size=(30, 3)).astype(np.float32).astype(np.float64)
        other = rng.uniform(1, 3, size=(150, 3))
        t = np.concatenate([tiny, exact, other] + ([[[3e10, 3e10, 3e10]]] if name == "edges_far" else []))
        t = t[rng.permutation(len(t))]
    else:
        raise KeyError(name)
    t.setflags(write=False)
    return t


def _target(name, golden_nn):
    return golden_nn[f"{name}_target"] if name in KAT_CASES else _shape(name)


@pytest.fixture(scope="module")
def host_ctx(icp):
    ctx = icp.Context(0, {"octree_builder": icp.BUILD_HOST})
    yield ctx
    ctx.close()


def _build(icp, gpu_ctx, host_ctx, xyz, mp, md, host):
    ctx = host_ctx if host else gpu_ctx
    ctx.set_target(xyz, mp, md, icp.RULES_ENGINE)
    assert ctx.target_build_info()[0] == (not host)
    return ctx, ctx.copy_target(), ctx.copy_target_aux()


def node_ranges(t):
    """[start, end) in leaf order of every node: a leaf's own range, an inner node's the span of
    its children (children sit one level deeper: deepest first)."""
    first, meta, depth = t["first"].astype(np.int64), t["meta"], t["depth"]
    leaf = (meta & LEAF) != 0
    start = np.where(leaf, first, 0)
    end = np.where(leaf, first + (meta & ~LEAF).astype(np.int64), 0)
    for d in range(int(depth.max()), -1, -1):
        k = np.flatnonzero(~leaf & (depth == d))
        if len(k):
            nk = POP8[meta[k] & 0xFF]
            assert np.all(nk > 0)
            start[k], end[k] = start[first[k]], end[first[k] + nk - 1]
    return start, end, leaf


def range_extremes(pts, start, end):
    """fp64 minimum and maximum of pts over every [start, end) (non-empty ranges)."""
    idx = np.c_[start, end].reshape(-1)
    lo = np.minimum.reduceat(np.r_[pts, [[np.inf] * 3]], idx, axis=0)[::2]
    hi = np.maximum.reduceat(np.r_[pts, [[-np.inf] * 3]], idx, axis=0)[::2]
    return lo, hi


def f32_down(v):
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, np.float32(-np.inf)), f)


def f32_up(v):
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f)


def check_tight_boxes(t, aux):
    start, end, _ = node_ranges(t)
    assert np.all(end > start), "an empty node"
    lo, hi = range_extremes(t["pts"], start, end)
    tb = aux["tbox"]
    assert tb.shape == (len(start), 6)
    # containment first: it names the property a search relies on
    assert np.all(tb[:, :3].astype(np.float64) <= lo), "a point lies below its node's tight box"
    assert np.all(tb[:, 3:].astype(np.float64) >= hi), "a point lies above its node's tight box"
    # the rounding as documented: outwards, and not at all where the extreme is an fp32 value
    np.testing.assert_array_equal(tb[:, :3], f32_down(lo))
    np.testing.assert_array_equal(tb[:, 3:], f32_up(hi))
    return lo, hi, f32_down(lo), f32_up(hi)


def table_depth(n_leaves, max_inner_depth):
    l = 1
    while l < 9 and 8 ** l < 8 * n_leaves:
        l += 1
    return max(min(l, max_inner_depth + 1), 0)


def check_cell_tables(t, aux):
    first, meta, depth = t["first"].astype(np.int64), t["meta"], t["depth"]
    start, end, leaf = node_ranges(t)
    inner_depth = int(depth[~leaf].max()) if np.any(~leaf) else -1
    lmax = aux["cell_lmax"]
    assert lmax == table_depth(int(leaf.sum()), inner_depth)
    cells = aux["cells"]
    assert len(cells) == (8 ** (lmax + 1) - 1) // 7
    pts, root = t["pts"], t["box"][0]
    for l in range(lmax + 1):
        tab = cells[(8 ** l - 1) // 7:(8 ** (l + 1) - 1) // 7]
        e = np.arange(8 ** l, dtype=np.int64)
        # (a) the plain descent of the host copy
        node, d = np.zeros(8 ** l, np.int64), np.zeros(8 ** l, np.int64)
        live = np.ones(8 ** l, bool)  # still descending: neither at a leaf nor absent
        for step in range(l):
            k = np.flatnonzero(live & ~leaf[np.maximum(node, 0)])
            live[:] = False
            o = (e[k] >> (3 * (l - 1 - step))) & 7
            m = meta[node[k]] & 0xFF
            there = ((m >> o) & 1) != 0
            node[k[~there]] = -1
            kk, oo, mm = k[there], o[there], m[there]
            node[kk] = first[node[kk]] + POP8[mm & ((1 << oo) - 1)]
            d[kk] = step + 1
            live[kk] = True
        np.testing.assert_array_equal(tab, np.where(node < 0, -1, (node << 5) | d), err_msg=f"level {l}")
        # (b) from the points: the cell of every point by the midpoint rule from the root box
        lo, hi = np.tile(root[:3], (len(pts), 1)), np.tile(root[3:], (len(pts), 1))
        cell = np.zeros(len(pts), np.int64)
        for _ in range(l):
            mid = (lo + hi) / 2
            up = pts > mid
            cell = (cell << 3) | (up[:, 0] * 1 + up[:, 1] * 2 + up[:, 2] * 4)
            lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
        ent = tab[cell].astype(np.int64)
        assert np.all(ent >= 0), f"level {l}: the cell of a target point is marked empty"
        pos = np.arange(len(pts))
        assert np.all((start[ent >> 5] <= pos) & (pos < end[ent >> 5])), f"level {l}: an entry misses a point of its cell"
        assert np.all((ent & 31) == depth[ent >> 5]) and np.all((ent & 31) <= l)
        reached = np.zeros(8 ** l, bool)
        reached[cell] = True
        rest = np.flatnonzero(~reached & (tab >= 0))  # allowed only below a leaf that ends above l
        if len(rest):
            n_, d_ = tab[rest].astype(np.int64) >> 5, tab[rest].astype(np.int64) & 31
            assert np.all(leaf[n_] & (d_ < l) & (d_ == depth[n_])), f"level {l}: an unreached cell names an inner node"
            # the leaf's own cell (the prefix at the leaf's depth) holds its points
            top = cells[((np.int64(1) << (3 * d_)) - 1) // 7 + (rest >> (3 * (l - d_)))]
            np.testing.assert_array_equal(top, tab[rest], err_msg=f"level {l}: an unreached cell names a foreign leaf")


def copy_flags_expected(pts):
    exp = np.zeros(len(pts), bool)
    for m in range(1, min(COPY_WINDOW, len(pts) - 1) + 1):
        exp[m:] |= np.all(pts[m:] == pts[:-m], axis=1)
    return exp


def check_copy_flags(ctx, t):
    flags = np.signbit(ctx.target_separation())[t["orig"]]
    np.testing.assert_array_equal(flags, copy_flags_expected(t["pts"]))
    return flags


# --- tight boxes and cell tables
@pytest.mark.parametrize("mp,md,host", TREES)
@pytest.mark.parametrize("name", KAT_CASES + SHAPES)
def test_tight_boxes_and_cell_tables(icp, gpu_ctx, host_ctx, golden_nn, name, mp, md, host):
    _, t, aux = _build(icp, gpu_ctx, host_ctx, _target(name, golden_nn), mp, md, host)
    check_tight_boxes(t, aux)
    check_cell_tables(t, aux)
    if name == "two":  # the root is a leaf: a table of one entry
        assert aux["cell_lmax"] == 0 and list(aux["cells"]) == [0]
    if name == "identical" and md >= 20:  # one leaf below a chain of inner nodes
        assert t["n_leaves"] == 1 and aux["cell_lmax"] == 1


@pytest.mark.parametrize("mp,md,host", TREES)
@pytest.mark.parametrize("name", ["edges", "edges_far"])
def test_tight_boxes_round_outwards_at_the_edges(icp, gpu_ctx, host_ctx, name, mp, md, host):
    _, t, aux = _build(icp, gpu_ctx, host_ctx, _shape(name), mp, md, host)
    lo64, hi64, lo, hi = check_tight_boxes(t, aux)
    # the case holds what it is for: a subnormal minimum and (small leaves) maximum, rounded out ...
    assert np.any(lo == np.float32(-TINY))
    if mp < 12 and name == "edges":
        assert np.any(hi == np.float32(TINY))
    # ... extremes that are fp32 values and stay, extremes that are not and move
    if name == "edges":
        assert np.any((hi.astype(np.float64) == hi64) & (hi64 > 1)) and np.any(hi.astype(np.float64) > hi64)
    else:
        assert np.all(hi64[0] == 3e10) and np.all(hi[0].astype(np.float64) >= 3e10)


def test_no_cell_tables_without_cell_starts(icp, golden_nn):
    with icp.Context(0, {"cell_starts": 0}) as ctx:
        ctx.set_target(golden_nn["gauss_target"], 10, 20, icp.RULES_ENGINE)
        aux = ctx.copy_target_aux()
        assert aux["cell_lmax"] == -1 and len(aux["cells"]) == 0
        check_tight_boxes(ctx.copy_target(), aux)


def test_copy_target_aux_arguments(icp, gpu_ctx, golden_nn):
    import ctypes as C
    L = icp.lib()
    with icp.Context(0) as fresh:
        assert L.icp_hip_copy_target_aux(fresh.handle, None, None, 0, None) == icp.ENOTREADY
    gpu_ctx.set_target(golden_nn["gauss_target"], 10, 20, icp.RULES_ENGINE)
    n = len(gpu_ctx.copy_target_aux()["cells"])
    small = np.empty(n - 1, np.int32)
    assert L.icp_hip_copy_target_aux(gpu_ctx.handle, None, small.ctypes.data_as(C.c_void_p), n - 1, None) == icp.EINVAL
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as grp:  # a group answers for member 0
        grp.set_target(golden_nn["gauss_target"], 10, 20, icp.RULES_ENGINE)
        a, b = grp.copy_target_aux(), gpu_ctx.copy_target_aux()
        np.testing.assert_array_equal(a["tbox"], b["tbox"])
        np.testing.assert_array_equal(a["cells"], b["cells"])


# --- copy flags
def _flag_cloud(name, golden_nn):
    rng = np.random.default_rng(11)
    if name == "rounded":
        return _shape("rounded")
    if name == "duplicates":
        return golden_nn["duplicates_target"]
    if name == "hundred":  # a leaf at maximum depth holding 100 identical points among others
        t = np.concatenate([rng.normal(size=(900, 3)), np.tile([[0.3, -0.2, 0.1]], (100, 1))])
        return t[rng.permutation(len(t))]
    if name == "distinct":
        return rng.normal(size=(5000, 3))
    if name == "zero_signs":  # two points that differ only in the sign of a zero
        return np.concatenate([[[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0]], rng.normal(size=(50, 3))])
    raise KeyError(name)


@pytest.fixture(scope="module")
def certify_ctx(icp):
    ctx = icp.Context(0, {"certify_prev": 3})
    yield ctx
    ctx.close()


@pytest.mark.parametrize("certify", [0, 1])
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("name", ["rounded", "duplicates", "hundred", "distinct", "zero_signs"])
def test_copy_flags(icp, gpu_ctx, certify_ctx, golden_nn, name, host, certify):
    ctx = certify_ctx if certify else gpu_ctx
    ctx.set_target(_flag_cloud(name, golden_nn), 10, 22 if host else 20, icp.RULES_ENGINE)
    assert ctx.target_build_info()[0] == (not host)
    t = ctx.copy_target()
    flags = check_copy_flags(ctx, t)
    if name == "hundred":  # every copy but the first is flagged: each has a twin one slot back
        same = np.all(t["pts"] == [0.3, -0.2, 0.1], axis=1)
        assert same.sum() == 100 and flags[same].sum() == 99 and flags.sum() == 99
    if name == "distinct":
        assert not flags.any()
    if name == "zero_signs":
        assert flags.sum() == 1
