"""Clouds and CPU checks of the georeferenced search tests (a helper module, not a conftest; the
tests: test_geo_fixtures.py on the CPU, test_gpu_geo_search.py on the GPU).

Every fixture exists at four places: plane_reference.OFFSETS (origin, geo, far) and ecef, whose z is
large as well (amax is a maximum over the axes and box_lo / box_hi act per axis: with geo and far
alone the z margins are never large). At (4.5e5, 5.4e6, 300) an fp32 ulp is 0.03 m in x and 0.5 m in
y and an fp64 ulp 1e-9 m: every rounding term of the certified search that is ~1e-13 at the origin
is within reach of the data there.

Three references, none of them the code under test:
  brute       numpy's fl(dx*dx + dy*dy + dz*dz) over every target point, first index of the minimum
  the oracle  oracle_py's octree nn() (the reference's visit order), equal to the brute force
              wherever no other point lies in the 2^-48 window of the nearest one
  shifting    a pair is shiftable when (cloud + o) - o == cloud bit for bit at every offset, for
              the target and the source: then every difference p - q is the same number at either
              place and an untransformed search returns the origin's indices and residual bits
              wherever no query lies in the tie window (the octree's midpoints never shift
              exactly: tree_shift()). Every offset is an integer
              below 2^23, so a cloud on the 2^-20 grid within a few metres of 0 qualifies
              (ulp(2^23) = 2^-29); a continuous cloud does not, and shifted it is a fixture of
              its own whose expected values are the oracle's at that place.

Fixtures (name -> target, source, max_points, max_depth at an offset: clouds()):
  slab_cont_N   a 2.5-D surface of 8000 points 4 m wide; N queries on the same surface turned by
                1 degree about the slab's centre and moved by a few millimetres
  slab_mm_N     the same, both clouds snapped to the 1 mm grid after the shift, as LAS data is
  slab_grid_N   the same on the 2^-20 grid before the shift: the shiftable slab
  blob          synth_pair(8000, 2048), shifted
  near_tie      1024 queries next to the bisector plane of their two nearest target points: the two
                distances differ by a few fp64 ulps of the coordinates, far less than the fp32 scan
                resolves (scan32_lower_bound's e_abs), far more than the 2^-48 window
  near_tie_close  4096 such queries 8 mm from a target pair of their own, in waves metres wide
  follow_N      the uniform clouds of test_gpu_follow_lists.py (every wave overflows), shifted
  the ball-chain fixtures of ball_fixtures.py by their names (uniform, shell, shell_flat), shifted,
  and shell_grid, the shell on the 2^-20 grid (shiftable); shell_deep* stay at the origin (CLUSTER_STEP = 2^-44 is below the fp64 ulp
  of 2^-30 at 5e6: the twelve points collapse into one)
"""
import functools

import numpy as np

import ball_fixtures as bf
import plane_reference as R

OFFSETS = dict(R.OFFSETS)
OFFSETS["ecef"] = np.array([-2.7e6, -4.3e6, 3.85e6])
PLACES = tuple(OFFSETS)  # origin first: the control
WINDOW = 2.0 ** -48      # kWindow (csrc/nn_device.h)
GRID = 2.0 ** -20
SLAB_TGT = 8000
SLAB_SIZES = (64, 65, 193, 2048)
SLAB_SIDE = 4.0
NEAR_TIE_Q = 1024
U32 = 2.0 ** -24
TIE_CAP_MM = 0.02        # share of a 1 mm fixture's queries inside the window where a certified path is asserted


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


def shift(cloud, where):
    return _frozen(np.asarray(cloud) + OFFSETS[where])


def conjugate(T, where):
    """The rigid motion T of the origin's frame as it acts at an offset: x -> o + T(x - o)."""
    o = OFFSETS[where]
    out = np.array(T, dtype=np.float64)
    out[:3, 3] = T[:3, 3] + o - T[:3, :3] @ o
    return out


# ---- shiftability

def exactly_shiftable(cloud):
    """(cloud + o) - o == cloud, bit for bit, at every offset."""
    cloud = np.asarray(cloud)
    return all(((cloud + o) - o).tobytes() == cloud.tobytes() for o in OFFSETS.values())


def shiftable(tgt, src):
    """Target and source both shift exactly: every p - q, hence every fl(d2), is the same number at
    every offset, and the brute-force answer with it."""
    return exactly_shiftable(tgt) and exactly_shiftable(src)


def tree_shift(icp, tgt, mp=10, md=20):
    """(the octree's boxes shift exactly, the tree has the origin's structure) over the offsets.
    The root box is the bounding box widened by eps = 0.001 (octree_build.cpp), and fl(min - 0.001)
    is on no binary grid: the boxes and midpoints of a shifted tree differ from the origin's by up
    to an fp64 ulp of the offset (1e-9), for every cloud. The structure (nodes, leaf order, point
    order) is the same unless a point lies that close to a splitting plane. So no fixture meets
    the midpoint condition; the answers of an untransformed search are still the origin's bits
    wherever no query lies in the tie window, because there the oracle's answer is the brute
    force's, which no tree enters. Inside the window the visit order decides and the tree counts."""
    base = icp.octree_build(tgt, mp, md)
    boxes, same = True, True
    for o in OFFSETS.values():
        t = icp.octree_build(np.asarray(tgt) + o, mp, md)
        if t["box"].shape != base["box"].shape:
            return False, False
        boxes &= (t["box"] - np.concatenate([o, o])).tobytes() == base["box"].tobytes()
        same &= all(t[k].tobytes() == base[k].tobytes() for k in ("first", "meta", "depth", "orig"))
    return boxes, same


# ---- the brute force

def brute(tgt, q):
    """Per query: the first index of the smallest fl(d2), sqrt of it, and whether another point's
    fl(d2) lies within the 2^-48 window of it (certified()'s test, csrc/nn_device.h)."""
    idx = np.empty(len(q), np.int32)
    d = np.empty(len(q))
    tie = np.zeros(len(q), bool)
    for k, p in enumerate(q):
        v = bf.d2(tgt, p)
        i = int(np.argmin(v))
        idx[k], d[k] = i, np.sqrt(v[i])
        tie[k] = int((v <= v[i] * (1.0 + WINDOW)).sum()) > 1
    return idx, d, tie


# ---- the slab and the blob

def _surface(xy):
    return 0.08 * np.sin(1.7 * xy[:, 0]) * np.cos(1.3 * xy[:, 1]) + 0.02 * np.sin(9.0 * xy[:, 0] + 4.0 * xy[:, 1])


@functools.lru_cache(maxsize=None)
def _slab_origin(n):
    rng = np.random.default_rng([7, n])
    txy = rng.uniform(0.0, SLAB_SIDE, (SLAB_TGT, 2))
    tgt = np.c_[txy, _surface(txy) + rng.normal(scale=0.003, size=SLAB_TGT)]
    sxy = rng.uniform(0.3, SLAB_SIDE - 0.3, (n, 2))
    s = np.c_[sxy, _surface(sxy) + rng.normal(scale=0.003, size=n)]
    a = np.radians(1.0)
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    c = np.array([SLAB_SIDE / 2, SLAB_SIDE / 2, 0.0])
    src = (s - c) @ rot.T + c + np.array([0.004, -0.003, 0.002])
    return _frozen(tgt), _frozen(src)


@functools.lru_cache(maxsize=None)
def slab(kind, n, where):
    """kind "cont", "mm" (snapped to 1 mm after the shift) or "grid" (2^-20 before it)."""
    tgt, src = _slab_origin(n)
    if kind == "grid":
        tgt, src = np.round(tgt / GRID) * GRID, np.round(src / GRID) * GRID
    tgt, src = tgt + OFFSETS[where], src + OFFSETS[where]
    if kind == "mm":
        tgt, src = np.round(tgt * 1000.0) / 1000.0, np.round(src * 1000.0) / 1000.0
    return _frozen(tgt), _frozen(src)


@functools.lru_cache(maxsize=None)
def blob(icp, where):
    tgt, src, _ = icp.synth_pair(8000, 2048)
    return shift(tgt, where), shift(src, where)


# ---- the near tie

def scan32_e_abs(ext):
    """e_abs of scan32_lower_bound (csrc/nn_kernels.hip) as k_nn_wave calls it, ext (1 + 2^-19):
    what the bound subtracts from the square root of the second-smallest fp32 value."""
    ext = ext * (1.0 + 2.0 ** -19)
    return 1.7320509 * 2.0 * ext * (U32 * (1.0 + 2.0 ** -20)) * (1.0 + U32) * (1.0 + 2.0 ** -40)


@functools.lru_cache(maxsize=None)
def near_tie(where):
    """4000 target points on a sparse surface (spacing ~0.35 m) and 1024 queries, each next to the
    bisector plane of two neighbouring target points A, B: q = the midpoint, moved within the plane,
    then nudged along B - A by a few nanometres until, in fp64 at this place, fl(d2) to A and to B
    differ by more than 2^-38 relative (far outside the 2^-48 window) and the distances by less than
    a tenth of e_abs (see check_near_tie). check_near_tie() verifies it, and that A and B are the two nearest points."""
    o = OFFSETS[where]
    rng = np.random.default_rng(11)
    side = 20.0
    txy = rng.uniform(0.0, side, (4000, 2))
    tgt = np.c_[txy, 0.3 * np.sin(0.5 * txy[:, 0]) + rng.normal(scale=0.02, size=4000)] + o
    qs = []
    order = rng.permutation(4000)
    for a in order:
        if len(qs) == NEAR_TIE_Q:
            break
        A = tgt[a]
        if not (2.0 < A[0] - o[0] < side - 2.0 and 2.0 < A[1] - o[1] < side - 2.0):
            continue
        v = bf.d2(tgt, A)
        v[a] = np.inf
        b = int(np.argmin(v))
        B = tgt[b]
        n = (B - A) / np.sqrt(v[b])
        mid = 0.5 * (A + B)
        for step in sorted(range(-24, 25), key=abs):
            q = mid + n * (step * 0.5e-9)
            w = bf.d2(tgt, q)
            two = np.partition(w, 2)[:3]
            if w[a] == w[b] or max(w[a], w[b]) != two[1] or min(w[a], w[b]) != two[0]:
                continue
            rel = two[1] / two[0] - 1.0
            gap = np.sqrt(two[1]) - np.sqrt(two[0])
            if rel > 2.0 ** -38 and gap < scan32_e_abs(np.sqrt(two[0])) / 10.0 and two[2] > two[1] * 1.02:
                qs.append(q)
                break
    assert len(qs) == NEAR_TIE_Q, len(qs)
    return _frozen(tgt), _frozen(np.array(qs))


CLOSE_Q, CLOSE_D, CLOSE_SIDE = 4096, 0.008, 20.0


@functools.lru_cache(maxsize=None)
def near_tie_close(where):
    """4096 queries on a 20 m square, each with a target pair of its own 8 mm away on either side
    (8192 target points), nudged off the pair's bisector plane as near_tie()'s are. A wave of the
    host query order spans more than a metre, so ext is over a hundred times the nearest distance:
    the slack that the selection key's cleared low bits leave (up to 2^-19 of the distance) is far
    below e_abs here, and the certificate rests on e_abs itself."""
    o = OFFSETS[where]
    rng = np.random.default_rng(12)
    tgt, qs = [], []
    seen = np.empty((CLOSE_Q, 2))
    while len(qs) < CLOSE_Q:
        xy = rng.uniform(0.0, CLOSE_SIDE, 2)
        if len(qs) and np.abs(seen[:len(qs)] - xy).max(axis=1).min() < 0.1:
            continue  # pairs stay 0.1 m apart: a query's third-nearest point is ten times farther
        seen[len(qs)] = xy
        c = np.array([xy[0], xy[1], 0.3 * np.sin(0.5 * xy[0])]) + o
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        A, B = c + CLOSE_D * n, c - CLOSE_D * n
        u = (B - A) / np.sqrt(bf.d2(B[None], A)[0])
        for step in sorted(range(-24, 25), key=abs):
            q = 0.5 * (A + B) + u * (step * 0.5e-9)
            wa, wb = bf.d2(A[None], q)[0], bf.d2(B[None], q)[0]
            lo, hi = min(wa, wb), max(wa, wb)
            if hi / lo - 1.0 > 2.0 ** -38 and np.sqrt(hi) - np.sqrt(lo) < 6e-9:
                tgt += [A, B]
                qs.append(q)
                break
    return _frozen(np.array(tgt)), _frozen(np.array(qs))


def wave_ext_floor(icp, q):
    """Per query, a lower bound of its wave's ext in the host query order (query_order = 1): half
    the largest extent of the bounding box of the wave's 64 queries (B holds every joined query,
    and ext is the largest distance from the frame's centre to a face of B)."""
    order = icp.source_shard_order(q)
    out = np.empty(len(q))
    for w in range(0, len(q), 64):
        i = order[w:w + 64]
        out[i] = 0.5 * np.ptp(q[i], axis=0).max()
    return out


def check_near_tie(tgt, q, ext=None):
    """Per query: the two smallest fl(d2) are outside the window of each other (relative gap above
    2^-40, third point 1 % away), and the distances' gap is below an eighth of e_abs at the smallest
    ext the wave's frame can have. ext is the largest half-extent of the box of the wave's balls,
    at least the query's own radius >= its nearest distance D1. scan32_lower_bound takes e_abs off
    the square root of the second-smallest fp32 value, which exceeds D2 by at most the rounding the
    bound allows for (e_abs + 2.5 u D2, every rounding at its worst and one way); with D2 - D1 below
    e_abs / 8 the bound ends below fl(d2)_1 (1 + 2^-48) unless seven eighths of that worst case
    occur, and the wave re-scans in fp64 when a single lane is left so. Returns the extremes."""
    rels, ratios = [], []
    for k, p in enumerate(q):
        w = np.sort(bf.d2(tgt, p))[:3]
        assert w[1] > w[0] * (1.0 + 2.0 ** -40) and w[2] > w[1] * 1.01, w
        gap = np.sqrt(w[1]) - np.sqrt(w[0])
        e = scan32_e_abs(np.sqrt(w[0]) if ext is None else ext[k])  # ext: wave_ext_floor's bound
        assert gap < e / 8.0, (gap, e)
        rels.append(w[1] / w[0] - 1.0)
        ratios.append(gap / e)
    return {"min_rel_gap": min(rels), "max_gap_over_e_abs": max(ratios)}


# ---- the follow-lists and ball-chain clouds

BALL_NAMES = ("uniform", "shell", "shell_flat", "shell_grid")
ORIGIN_ONLY = ("shell_deep20", "shell_deep40")  # CLUSTER_STEP = 2^-44: below the fp64 ulp at the offsets


def follow(n, where):
    """test_gpu_follow_lists.py's clouds (ball_fixtures' uniform pair: the same seeds), shifted."""
    return shift(bf.uniform_target(), where), shift(bf.uniform_source(n), where)


def ball(name, n, where):
    """A ball-chain fixture of ball_fixtures.py, shifted. shell_grid: the shell, target and source
    rounded to the 2^-20 grid before the shift (the shiftable one)."""
    if name == "shell_grid":
        tgt, src, mp, md = bf.clouds("shell", n)
        tgt, src = np.round(tgt / GRID) * GRID, np.round(src / GRID) * GRID
    else:
        tgt, src, mp, md = bf.clouds(name, n)
    return shift(tgt, where), shift(src, where), mp, md


@functools.lru_cache(maxsize=None)
def ball_model(icp, name, where):
    """ball_fixtures.tree_model of the shifted target: the pre-checks and counter expectations at
    an offset come from the tree the device searches there."""
    tgt, _, mp, md = ball(name, bf.SIZES[0], where)
    return bf.tree_model_of(icp, tgt, mp, md)


def clouds(icp, name, where):
    """(target, source, max_points, max_depth) of a named fixture at an offset."""
    kind, _, n = name.rpartition("_")
    if kind.startswith("slab_"):
        return (*slab(kind[5:], int(n), where), 10, 20)
    if name == "blob":
        return (*blob(icp, where), 10, 20)
    if name == "near_tie":
        return (*near_tie(where), 10, 20)
    if name == "near_tie_close":
        return (*near_tie_close(where), 10, 20)
    if kind == "follow":
        return (*follow(int(n), where), 10, 20)
    return ball(kind, int(n), where)


# what test_gpu_geo_search.py compares with the oracle; the CPU test proves each at every offset
SEARCH_FIXTURES = (["slab_cont_%d" % n for n in SLAB_SIZES] + ["slab_mm_%d" % n for n in SLAB_SIZES]
                   + ["slab_grid_193", "slab_grid_2048", "blob", "near_tie", "near_tie_close"]
                   + ["follow_%d" % n for n in bf.SIZES]
                   + ["%s_%d" % (name, n) for name in BALL_NAMES[1:] for n in bf.SIZES])  # uniform_N is follow_N
# where shiftable() holds (test_geo_fixtures.py asserts this list is the whole of it)
SHIFTABLE = ("slab_grid_193", "slab_grid_2048") + tuple("shell_grid_%d" % n for n in bf.SIZES)


def tie_cap(name):
    """The largest share of queries inside the tie window on a fixture where a test asserts that a
    certified path ran: none on the continuous and the shiftable fixtures, 2 % on the 1 mm grid."""
    return TIE_CAP_MM if name.startswith("slab_mm_") else 0.0
