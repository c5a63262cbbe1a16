"""The source's kd query order as the device builds it (query_order_gpu.hip), read back with
icp_hip_copy_query_order and compared element for element with a numpy model written from the
algorithm in that file's header comment (not from its kernels):

  * the segments of every level come from the sizes alone (split_at);
  * one origin per cloud: per axis the median (index count / 2 of the sorted finite values) of the
    strided sample 0, stride, 2 stride, ..., stride = ceil(n / 1024);
  * c = float32((finite(v) ? v : 0) - origin) + 0.0f, the subtraction in fp64 (a zero is +0.0:
    -0.0 and +0.0 tie, as they do on the host);
  * per splitting segment the longest axis of the fp32 bounding box of c, ties to the lower axis;
  * the new order is a stable sort of the segment's current order by the order-preserving image of
    c's bits on that axis; finished segments keep their order.

A stable radix sort is deterministic, so the bar is exact. End-to-end parity cannot see this
structure: the search is exact under any permutation, a wrong axis or a collapsed key only makes
the waves less compact. So the compactness is asserted as well, against the host order
(icp_source_shard_order, query_order.cpp: fp64 keys): the median bounding-box diagonal of the 64- and
the 8-query buckets is at most 1.05 x the host order's. The 1.05 is a condition: fp32 keys relative
to the cloud's origin resolve 2^-24 of the cloud's extent, which reorders only near-ties, while
absolute fp32 keys at georeferenced magnitudes (ulp 0.03 m at 4.5e5, 0.5 m at 5.4e6) gave 1.08 to
1.50 (64 queries) and 1.19 to 2.58 (8 queries) on the georeferenced slabs below
(profiles/query_order_origin/ratios_parent_head.txt).

Sizes: one lane, a bucket, a bucket and one, the wave edges, three waves and one, 4097, kChunk and
kChunk + 1 (a big segment whose second chunk holds one slot), 40000 (two levels of big segments,
three chunks each, the last one short).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUCKET = 8
SAMPLE = 1024
GEO_A = (4.5e5, 5.4e6, 300.0)
GEO_B = (-7.3e6, 2.1e6, -40.0)
ALL_SIZES = (1, 8, 9, 63, 64, 65, 127, 128, 129, 193, 4097, 16384, 16385, 40000)
FAR = np.array([[-3e10, -3e10, -3e10], [3e10, -2e10, 1e10], [-1e10, 3e10, -2e10], [2e10, 1e10, 3e10]])


# --- the clouds
def _slab(rng, n, offset=(0.0, 0.0, 0.0)):
    """x and y uniform on a square (2 m up to 4097 points, 20 m above), z normal with sigma 0.05."""
    side = 2.0 if n <= 4097 else 20.0
    return np.c_[rng.uniform(0, side, size=(n, 2)), rng.normal(size=n) * 0.05] + np.asarray(offset)


def _make(cloud, n):
    rng = np.random.default_rng([len(cloud), n])
    if cloud == "slab":
        return _slab(rng, n)
    if cloud == "slab_geo_a":
        return _slab(rng, n, GEO_A)
    if cloud == "slab_geo_b":
        return _slab(rng, n, GEO_B)
    if cloud == "rounded":  # many exact ties on every axis: the sort's stability decides
        return np.round(rng.normal(size=(n, 3)), 1)
    if cloud == "constant_axis":
        return np.c_[rng.uniform(-1, 1, size=n), np.full(n, 0.75), rng.uniform(-3, 3, size=n)]
    if cloud == "identical":
        return np.full((n, 3), 0.25)
    if cloud == "nonfinite":  # NaN, +inf and -inf coordinates sprinkled in: they count as 0
        x = rng.normal(size=(n, 3)) * [4, 4, 1]
        k = rng.integers(0, n, size=(max(3, n // 10), 2))
        x[k[:, 0], k[:, 1] % 3] = rng.choice([np.nan, np.inf, -np.inf], size=len(k))
        return x
    if cloud == "signed_zeros":  # the split axis (x, the long one) holds zeros of both signs
        x = np.c_[rng.uniform(-10, 10, size=n), rng.normal(size=(n, 2)) * 0.1]
        z = rng.random(n) < 0.6
        x[z, 0] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
        return x
    if cloud == "outliers_geo":  # four 3e10 outliers in front of a georeferenced slab
        return np.concatenate([FAR, _slab(rng, n - 4, GEO_A)])
    raise KeyError(cloud)


CASES = (
    [("slab", n) for n in ALL_SIZES]
    + [("slab_geo_a", n) for n in (9, 65, 193, 4097, 16385, 40000)]
    + [("slab_geo_b", n) for n in (193, 4097, 16384, 40000)]
    + [("rounded", n) for n in (129, 4097, 16385)]
    + [("constant_axis", n) for n in (193, 4097)]
    + [("identical", n) for n in (65, 4097)]
    + [("nonfinite", n) for n in (65, 193, 4097, 16385)]
    + [("signed_zeros", n) for n in (64, 193, 4097)]
    + [("outliers_geo", n) for n in (193, 4097, 40000)]
)
NO_QUALITY = ("identical", "nonfinite")


# --- the model
def split_at(n, bucket):
    unit = 64 if n > 64 else bucket
    h = ((n // 2 + unit - 1) // unit) * unit
    return n - unit if h >= n else h


def model_origin(xyz):
    stride = -(-len(xyz) // SAMPLE)
    sample = xyz[::stride]
    o = np.zeros(3)
    for a in range(3):
        v = np.sort(sample[np.isfinite(sample[:, a]), a])
        if len(v):
            o[a] = v[len(v) // 2]
    return o


def model_order(xyz, bucket=BUCKET):
    n = len(xyz)
    perm = np.arange(n, dtype=np.int32)
    if n <= bucket:
        return perm
    with np.errstate(over="ignore"):
        c = (np.where(np.isfinite(xyz), xyz, 0.0) - model_origin(xyz)).astype(np.float32) + np.float32(0.0)
    bits = c.view(np.uint32)
    key = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))
    segs = [(0, n)]
    while any(sz > bucket for _, sz in segs):
        nxt = []
        for st, sz in segs:
            if sz <= bucket:
                nxt.append((st, sz))
                continue
            idx = perm[st:st + sz]
            cc = c[idx]
            ext = cc.max(axis=0) - cc.min(axis=0)  # float32
            ax = 0
            for a in (1, 2):
                if ext[a] > ext[ax]:
                    ax = a
            perm[st:st + sz] = idx[np.argsort(key[idx, ax], kind="stable")]
            h = split_at(sz, bucket)
            nxt += [(st, h), (st + h, sz - h)]
        segs = nxt
    return perm


def bucket_diagonals(xyz, order, size):
    p = xyz[order]
    d = [np.linalg.norm(np.ptp(p[k:k + size], axis=0)) for k in range(0, len(p), size)]
    return float(np.median(d))


@functools.lru_cache(maxsize=None)
def _case(cloud, n):
    xyz = _make(cloud, n)
    xyz.setflags(write=False)
    model = model_order(xyz)
    model.setflags(write=False)
    return xyz, model


def assert_order(icp, xyz, got, model, cloud, quality=True):
    n = len(xyz)
    # (a) a permutation
    assert got.shape == (n,)
    np.testing.assert_array_equal(np.sort(got), np.arange(n), err_msg="not a permutation of 0..n-1")
    # (b) the model's, element for element
    np.testing.assert_array_equal(got, model)
    # (c) as compact as the host order
    if quality and n >= 193 and cloud not in NO_QUALITY:
        host = icp.source_shard_order(xyz)
        for size in (64, 8):
            dev, ref = bucket_diagonals(xyz, got, size), bucket_diagonals(xyz, host, size)
            print(f"{cloud} n={n} {size}-query buckets: median diagonal device {dev:.6g} host {ref:.6g} "
                  f"ratio {dev / ref if ref > 0 else float('nan'):.4f}")
            assert dev <= 1.05 * ref, (cloud, n, size, dev, ref)


@pytest.mark.parametrize("cloud,n", CASES)
def test_device_order_equals_model(icp, gpu_ctx, cloud, n):
    xyz, model = _case(cloud, n)
    gpu_ctx.set_source(xyz)
    assert_order(icp, xyz, gpu_ctx.query_order(), model, cloud)


@pytest.mark.parametrize("n", (65, 193, 4097))
def test_routes_install_the_same_order(icp, gpu_ctx, n):
    """set_source from host memory, set_source_device and a two-member group on devices (0, 0):
    the single context's order; the group's is the order of the whole cloud."""
    xyz, model = _case("slab_geo_a", n)
    gpu_ctx.set_source(xyz)
    single = gpu_ctx.query_order()
    assert_order(icp, xyz, single, model, "slab_geo_a")
    with gpu_ctx.to_device(xyz) as d_xyz:
        gpu_ctx.set_source_device(d_xyz, n)
        np.testing.assert_array_equal(gpu_ctx.query_order(), single)
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as grp:
        grp.set_source(xyz)
        whole = grp.query_order()
    assert_order(icp, xyz, whole, model, "slab_geo_a", quality=False)
    np.testing.assert_array_equal(whole, single)


@pytest.mark.parametrize("n", (65, 4097))
def test_host_route_installs_the_host_order(icp, n):
    xyz, _ = _case("slab_geo_a", n)
    with icp.Context(0, {"query_order": 1}) as ctx:
        ctx.set_source(xyz)
        np.testing.assert_array_equal(ctx.query_order(), icp.source_shard_order(xyz))


def test_no_source_is_not_ready(icp):
    with icp.Context(0) as ctx:
        with pytest.raises(icp.IcpError) as e:
            ctx.query_order()
        assert e.value.code == icp.ENOTREADY
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as grp:
        with pytest.raises(icp.IcpError) as e:
            grp.query_order()
        assert e.value.code == icp.ENOTREADY
