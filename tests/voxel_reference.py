"""The numpy model of voxel-grid down-sampling (a helper module, not a conftest) and
the clouds the host and the GPU tests share.

Cells c_a = floor((x_a - o_a) / h) in fp64 as written, key = cz << 42 | cy << 21 | cx, voxels in
ascending key order, a voxel's points in ascending original index. The centroid of a voxel of m
points: d_i = x_i - o, rows of 64 added in order into 64 partials that start from +0.0, the fold
s_l += s_{l+w} for w = 32, 16, .., 1, the point o + s_0 / m. The origin is an argument."""
import math

import numpy as np

CENTROID, FIRST = 0, 1
CELLS = 1 << 21


def keys_of(xyz, h, origin):
    c = np.floor((np.asarray(xyz, np.float64) - np.asarray(origin, np.float64)) / h)
    assert (c >= 0).all() and (c < CELLS).all(), "a cell index outside [0, 2^21)"
    c = c.astype(np.uint64)
    return (c[:, 2] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 0]


def model(xyz, h, origin, mode=CENTROID):
    """(points (m, 3), first (m,) int32, count (m,) int32, members): members[r] = the original
    indices of voxel r, ascending."""
    xyz = np.ascontiguousarray(xyz, np.float64)
    o = np.asarray(origin, np.float64)
    key = keys_of(xyz, h, o)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    ends = np.r_[starts[1:], len(ks)]
    m = len(starts)
    pts = np.empty((m, 3))
    first = np.empty(m, np.int32)
    count = np.empty(m, np.int32)
    members = []
    for r in range(m):  # a plain loop over the runs
        ids = order[starts[r]:ends[r]]
        members.append(ids)
        first[r], count[r] = ids[0], len(ids)
        if mode == FIRST:
            pts[r] = xyz[ids[0]]
            continue
        d = xyz[ids] - o
        s = np.zeros((64, 3))
        for row in range(0, len(ids), 64):
            blk = d[row:row + 64]
            s[:len(blk)] = s[:len(blk)] + blk
        for w in (32, 16, 8, 4, 2, 1):
            s[:w] = s[:w] + s[w:2 * w]
        pts[r] = o + s[0] / len(ids)
    return pts, first, count, members


def fsum_means(xyz, members):
    """Per voxel and axis the mean of its points from their exactly rounded sum (math.fsum): (m, 3)."""
    out = np.empty((len(members), 3))
    for r, ids in enumerate(members):
        for a in range(3):
            out[r, a] = math.fsum(xyz[ids, a]) / len(ids)
    return out


def centroid_bound(xyz, members, origin):
    """(count + 2) · 2^-52 · (Σ|d_i| / count + |o|) per voxel and axis: any summation order of the
    d_i plus the two final roundings."""
    o = np.asarray(origin, np.float64)
    out = np.empty((len(members), 3))
    for r, ids in enumerate(members):
        d = np.abs(xyz[ids] - o)
        out[r] = (len(ids) + 2) * 2.0 ** -52 * (d.sum(0) / len(ids) + np.abs(o))
    return out


RUN_LENGTHS = (63, 64, 65, 128, 129, 4097)
CASE_NAMES = ["n1", *[f"run{n}" for n in RUN_LENGTHS], "run17_16", "lattice_faces", "lattice_rounding", "own_voxel",
              "blob", "blob_coarse", "blob_georef", "copies", "origin_below", "blob_first"]
_CASES = {}


def cases(icp):
    """name -> (xyz, h, origin or None, mode). The arrays are shared: do not write to them."""
    if _CASES:
        return _CASES
    rng = np.random.default_rng(2024)
    blob = icp.synth_pair(20000)[0]
    c = {"n1": (np.array([[1.5, -2.25, 3.0]]), 0.5, None, CENTROID)}
    for n in RUN_LENGTHS:  # all in one voxel
        c[f"run{n}"] = (rng.uniform(0.0, 0.4, (n, 3)) + [10.0, -3.0, 2.0], 1.0, None, CENTROID)
    a = rng.uniform(0.0, 0.4, (17, 3))
    b = rng.uniform(0.0, 0.4, (16, 3)) + [1.5, 0.0, 0.0]
    c["run17_16"] = (rng.permutation(np.concatenate([a, b])), 1.0, None, CENTROID)  # the packing boundary
    g = np.arange(16, dtype=np.float64)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    c["lattice_faces"] = (rng.permutation(lat * 0.25), 0.5, None, CENTROID)  # every point on a cell face
    c["lattice_rounding"] = (rng.permutation(lat * 0.1), 0.1, None, CENTROID)  # the division's rounding decides
    cell = rng.choice(100 ** 3, 5000, replace=False)
    own = np.stack([cell % 100, cell // 100 % 100, cell // 10000], -1) + rng.uniform(0.1, 0.9, (5000, 3))
    c["own_voxel"] = (own, 1.0, (0.0, 0.0, 0.0), CENTROID)
    c["blob"] = (blob, 0.5, None, CENTROID)
    c["blob_coarse"] = (blob, 2.0, None, CENTROID)  # runs of hundreds beside runs of one: mixed waves
    c["blob_georef"] = (blob + [5.4e6, 4.1e5, 300.0], 0.05, None, CENTROID)
    copies = blob[:1040].copy()
    copies[rng.choice(1040, 40, replace=False)] = copies[7]
    c["copies"] = (copies, 0.25, None, CENTROID)
    sub = blob[:3000]
    c["origin_below"] = (sub, 0.5, tuple(sub.min(0) - [0.3, 1.7, 0.05]), CENTROID)
    c["blob_first"] = (blob, 0.5, None, FIRST)
    for v in c.values():
        v[0].setflags(write=False)
    _CASES.update(c)
    return _CASES


_EXPECTED = {}


def expected(icp, name):
    """The model on a case, about the origin the definition gives it (the minimum, zeros as +0.0),
    computed once: (points, first, count, members, origin)."""
    if name not in _EXPECTED:
        xyz, h, origin, mode = cases(icp)[name]
        o = np.asarray(origin, np.float64) if origin is not None else xyz.min(0) + 0.0
        _EXPECTED[name] = model(xyz, h, o, mode) + (o,)
    return _EXPECTED[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
