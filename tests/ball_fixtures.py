"""Clouds and CPU pre-checks of the follow-up search's chain tests (a helper module, not a conftest;
the tests: test_gpu_ball_chain.py).

k_nn_ball's constants are restated below with their source lines. Every cloud is seeded and shared
read-only. A pre-check makes the link a fixture targets certain from the target's octree
(icp.octree_build's node arrays: the very tree the device searches) and the brute-force nearest
fl(d2) d*^2 of each query in numpy, without looking at a kernel's output:

  waves overflow   the bounding box of every full wave's queries, in the host query order and in the
                   caller's, holds more than CAND_CAP target points: the wave's search box (which
                   holds the box of its queries' balls) overflows the candidate list, and with the
                   half and wide passes off every query of the wave goes to the ball list
  chain (a)        the leaves with squared cell-box distance s <= d*^2 hold more than BALL_GPOINTS
                   points: the ball walk lists every leaf with s <= u (1 + 2^-47), u >= d*^2 for any
                   valid guess u, so its point list overflows (or its node stack does first)
  chain (b)        there are more than LANE_BUDGET such leaves: fast_dfs (nn_device.h) counts a node
                   visit each time it arrives at a node, pruned or not, and prunes only on
                   s > best (1 + 2^-47) >= d*^2, so it arrives at every one of them: over budget
  chain (c)        the tree has fewer than BB_NODES nodes: wave_bb pushes a node at most once per
                   pass (its start nodes head disjoint subtrees), so its stack cannot overflow
  chain (d)        more than CAND_CAP target points lie in the box q +- d*: a wave overflows even
                   when this query alone joins its box
  ties             at least two target points share the minimum fl(d2) of every query

Fixtures (targets; the sources of the shells are uniform in the cube of half-side SRC_HALF about
the shell's centre):
  uniform      the follow-lists clouds: 20 000 uniform target points, uniform sources
  shell        4000 points on the sphere of radius 0.5 about (0.5, 0.5, 0.5), radial jitter +-1e-3
  shell_deep   shell plus 12 distinct points in a row next to one shell point, CLUSTER_STEP apart.
               (A step of 2^-30 stops splitting at depth 27: eleven points span less than a depth-26
               cell. 2^-44 keeps all twelve in one cell down to depth 40, so the tree is 20 deep
               under max_depth 20 and 40 deep under max_depth 40, which is what the case is for.)
  shell_flat   shell under max_depth 3: leaves of up to 36 points
  shell_ties   a 2000-point half shell and its mirror image in the plane z = 0.5, the sources
               flattened into that plane: the shell's chain (a) to (d), and every query's nearest
               point ties with its image exactly, so the chain's wave_bb ends in a tie
  lattice      the 32^3 lattice of spacing 1/32; sources: distinct centres (i + 1/2)/32 of cells
               with all eight corners on the lattice (i <= 30); every coordinate is a multiple of
               2^-6, so the eight corners have the same fl(d2) exactly
"""
import functools

import numpy as np

BALL_GROUPS = 4       # kBallGroups (csrc/nn_ball.hip:67): queries per wave of the ball walk
BALL_GPOINTS = 256    # kBallGPoints = kBallPoints / kBallGroups (csrc/nn_ball.hip:70, 72)
BALL_GSTACK = 128     # kBallGStack = kBallStack / kBallGroups (csrc/nn_ball.hip:69, 71)
LANE_BUDGET = 64      # kLaneBudget = ICP_LANE_BUDGET (csrc/nn_ball.hip:120, 122)
BB_PTS = 256          # kBBPts (csrc/nn_ball.hip:124): leaf points wave_bb lists per round
BB_NODES = 2048 - BB_PTS  # kBBStack - kBBPts (csrc/nn_ball.hip:123, 227): wave_bb's node stack
BALL_MAX_BLOCKS = 8192    # launch_nn_follow's grid cap (csrc/nn_ball.hip:676)
BALL_LDS_FLOOR = 8192     # launch_nn_follow: max(kBallLdsBytes, kBBStack * 4) (csrc/nn_ball.hip:668, 670)
CAND_CAP = 1008       # kWaveCandCap (csrc/kernels.h:65)
GPU_BUILD_MAX_DEPTH = 21  # kGpuBuildMaxDepth (csrc/octree_gpu.h:15): deeper trees come from the host builder
LEAF_BIT = 0x80000000     # kLeafBit (csrc/icp_common.h:34)

CENTRE = np.array([0.5, 0.5, 0.5])
RADIUS, JITTER, SRC_HALF = 0.5, 1e-3, 0.01
CLUSTER_STEP = 2.0 ** -44
SIZES = (64, 65, 193)
LATTICE_SIZES = (64, 193)
N_LONG = 500_000


def _frozen(*arrays):
    out = tuple(np.ascontiguousarray(a, dtype=np.float64) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out if len(out) > 1 else out[0]


@functools.lru_cache(maxsize=None)
def uniform_target():
    return _frozen(np.random.default_rng(20_000).random((20_000, 3)))


@functools.lru_cache(maxsize=None)
def uniform_source(n):
    return _frozen(np.random.default_rng(1_000 + n).random((n, 3)))


@functools.lru_cache(maxsize=None)
def shell_target():
    rng = np.random.default_rng(5)
    v = rng.normal(size=(4000, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    r = RADIUS + rng.uniform(-JITTER, JITTER, 4000)
    return _frozen(CENTRE + v * r[:, None])


@functools.lru_cache(maxsize=None)
def shell_deep_target():
    t = shell_target()
    row = np.zeros((12, 3))
    row[:, 0] = CLUSTER_STEP * np.arange(1, 13)
    out = np.concatenate([t, t[17] + row])
    assert len(np.unique(out, axis=0)) == len(out)
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def shell_ties_target():
    """The upper half of a 2000-point shell (offsets from the centre on the 2^-20 grid, so that the
    centre plus or minus an offset is exact) and its mirror image in the plane z = 0.5."""
    rng = np.random.default_rng(6)
    v = rng.normal(size=(2000, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    v *= (RADIUS + rng.uniform(-JITTER, JITTER, 2000))[:, None]
    v[:, 2] = np.maximum(np.abs(v[:, 2]), 2.0 ** -10)
    v = np.round(v * 2.0 ** 20) / 2.0 ** 20
    return _frozen(np.concatenate([CENTRE + v, CENTRE + v * [1.0, 1.0, -1.0]]))


@functools.lru_cache(maxsize=None)
def shell_source(n):
    return _frozen(CENTRE + np.random.default_rng(100 + n).uniform(-SRC_HALF, SRC_HALF, (n, 3)))


@functools.lru_cache(maxsize=None)
def shell_ties_source(n):
    """shell_source flattened into the mirror plane: a query's dz to a point and to its image are
    +-vz exactly, dx and dy the same, so the two fl(d2) are equal."""
    q = np.array(shell_source(n))
    q[:, 2] = CENTRE[2]
    return _frozen(q)


@functools.lru_cache(maxsize=None)
def lattice_target():
    g = np.arange(32) / 32.0
    return _frozen(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def lattice_source(n):
    cells = np.random.default_rng(300 + n).choice(31 ** 3, n, replace=False)
    return _frozen((np.stack(np.unravel_index(cells, (31, 31, 31)), 1) + 0.5) / 32.0)


# name -> (target, source(n), max_points, max_depth)
FIXTURES = {
    "uniform": (uniform_target, uniform_source, 10, 20),
    "shell": (shell_target, shell_source, 10, 20),
    "shell_deep20": (shell_deep_target, shell_source, 10, 20),
    "shell_deep40": (shell_deep_target, shell_source, 10, 40),
    "shell_flat": (shell_target, shell_source, 10, 3),
    "shell_ties": (shell_ties_target, shell_ties_source, 10, 20),
    "lattice_ties": (lattice_target, lattice_source, 10, 20),
}


def clouds(name, n):
    """(target, source, max_points, max_depth) of a fixture at a source size."""
    tgt, src, mp, md = FIXTURES[name]
    return tgt(), src(n), mp, md


# ---- the pre-checks

def d2(points, q):
    """fl(d2) of each point from q, in the kernels' order of operations (no FMA)."""
    d = points - q
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def box_s(lo, hi, q):
    """Squared distance of q from each box [lo, hi] (nn_device.h box_s)."""
    a = np.maximum(0.0, np.maximum(lo - q, q - hi))
    return a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]


@functools.lru_cache(maxsize=None)
def tree_model(icp, name):
    """The fixture's octree as the searches see it: per leaf its cell box, the exact box of its
    points (the device's tight boxes are these rounded outwards to fp32) and its point count; the
    node count and the stack levels (max_inner_depth + 1)."""
    tgt, _, mp, md = FIXTURES[name]
    return tree_model_of(icp, tgt(), mp, md)


def tree_model_of(icp, tgt, mp, md):
    """tree_model of any target (a shifted fixture's: geo_fixtures.py)."""
    t = icp.octree_build(tgt, mp, md)
    leaf = (t["meta"] & np.uint32(LEAF_BIT)) != 0
    cnt = (t["meta"][leaf] & np.uint32(LEAF_BIT - 1)).astype(np.int64)
    first = t["first"][leaf].astype(np.int64)
    order = np.argsort(first, kind="stable")
    assert np.array_equal(np.cumsum(cnt[order]) - cnt[order], first[order]) and cnt.sum() == len(t["pts"])
    keep = order[cnt[order] > 0]
    tlo, thi = np.empty((leaf.sum(), 3)), np.empty((leaf.sum(), 3))
    tlo[:], thi[:] = np.inf, -np.inf
    tlo[keep] = np.minimum.reduceat(t["pts"], first[keep], axis=0)
    thi[keep] = np.maximum.reduceat(t["pts"], first[keep], axis=0)
    return {"lo": t["box"][leaf, :3], "hi": t["box"][leaf, 3:], "tlo": tlo, "thi": thi, "cnt": cnt,
            "n_nodes": len(t["meta"]), "max_depth": int(t["max_depth"]), "levels": int(t["max_inner_depth"]) + 1}


def wave_box_counts(tgt, q):
    """Target points inside the bounding box of each full wave (64 consecutive queries) of q."""
    return [int(np.all((tgt >= q[64 * w: 64 * w + 64].min(0)) & (tgt <= q[64 * w: 64 * w + 64].max(0)), axis=1).sum())
            for w in range(len(q) // 64)]


def check_waves_overflow(icp, tgt, src):
    """Every full wave overflows, in the host query order (the iterates) and the caller's (nn).
    Returns the smallest count."""
    counts = wave_box_counts(tgt, src[icp.source_shard_order(src)]) + wave_box_counts(tgt, src)
    assert min(counts) > CAND_CAP, counts
    return min(counts)


def check_chain(model, tgt, q):
    """Pre-checks (a) to (d) for every query of q; returns their minima (and the node count)."""
    assert model["n_nodes"] < BB_NODES, model["n_nodes"]                      # (c)
    pts_a, leaves_b, in_box = [], [], []
    for p in q:
        best = d2(tgt, p).min()
        live = box_s(model["lo"], model["hi"], p) <= best
        pts_a.append(int(model["cnt"][live].sum()))
        leaves_b.append(int(live.sum()))
        in_box.append(int(np.all(np.abs(tgt - p) <= np.sqrt(best), axis=1).sum()))
    assert min(pts_a) > BALL_GPOINTS, min(pts_a)                               # (a)
    assert min(leaves_b) > LANE_BUDGET, min(leaves_b)                          # (b)
    assert min(in_box) > CAND_CAP, min(in_box)                                 # (d)
    return {"a_points": min(pts_a), "b_leaves": min(leaves_b), "c_nodes": model["n_nodes"], "d_in_box": min(in_box)}


def check_chain_in_cube(model, tgt):
    """(a) to (d) for every query of the shells' source cube at once (the 500 000 queries of the long
    case): every target point lies within [RADIUS - JITTER, RADIUS + JITTER] of the centre (checked)
    and a query within e = sqrt(3) SRC_HALF of it, so d* >= dlo = RADIUS - JITTER - e
    - 2^-40; a box's distance from q is at most its distance from the centre plus e (point-to-set
    distances are 1-Lipschitz), so a leaf within dlo - e of the centre has s <= d*^2 for every such q,
    and the cube centre +- (dlo - SRC_HALF) lies inside every q +- d*. 2^-20 covers the rounding."""
    assert model["n_nodes"] < BB_NODES, model["n_nodes"]
    e = np.sqrt(3.0) * SRC_HALF
    dlo = RADIUS - JITTER - e - 2.0 ** -40
    r = np.sqrt(d2(tgt, CENTRE))
    assert r.min() >= RADIUS - JITTER - 2.0 ** -40 and r.max() <= RADIUS + JITTER + 2.0 ** -40
    live = np.sqrt(box_s(model["lo"], model["hi"], CENTRE)) <= dlo - e - 2.0 ** -20
    out = {"a_points": int(model["cnt"][live].sum()), "b_leaves": int(live.sum()), "c_nodes": model["n_nodes"],
           "d_in_box": int(np.all(np.abs(tgt - CENTRE) <= dlo - SRC_HALF - 2.0 ** -20, axis=1).sum())}
    assert out["a_points"] > BALL_GPOINTS and out["b_leaves"] > LANE_BUDGET and out["d_in_box"] > CAND_CAP, out
    return out


def listed_points(model, tgt, q):
    """A lower bound of the leaf points wave_bb lists over the queries of q: a leaf whose points'
    exact box has s <= d*^2 passes the live test at any bound the search can hold (the device's tight
    box is no smaller, the bound no less than d*^2 (1 + 2^-47)), and so do its ancestors' cells."""
    return sum(int(model["cnt"][box_s(model["tlo"], model["thi"], p) <= d2(tgt, p).min()].sum()) for p in q)


def check_flat_rounds(model):
    """shell_flat: some 64 leaves (one step's pops) together hold more than BB_PTS points, so a
    step can list more than one round. Returns the 64 fullest leaves' points."""
    top = int(np.sort(model["cnt"])[-64:].sum())
    assert top > BB_PTS, top
    return top


def check_ties(tgt, q):
    """Every query has at least two target points at its minimum fl(d2). Returns the fewest."""
    ties = []
    for p in q:
        v = d2(tgt, p)
        ties.append(int((v == v.min()).sum()))
    assert min(ties) >= 2, min(ties)
    return min(ties)
