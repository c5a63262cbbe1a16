"""Device-resident clouds (icp_hip_*_device, include/icp_hip.h): a context fed and read through
buffers in HBM against one fed and read through the host calls. The host path is the
specification, so every comparison is exact: icp_iter_stats bytes, correspondences, residuals and
the moved source, bit for bit.

Buffers come from the library's own icp_hip_dev_alloc / icp_hip_dev_copy (DeviceBuffer): no other
HIP runtime is brought into the process.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TARGETS = [1, 10, 11, 5000]       # 10 / 11: the first leaf split (max_points 10)
SOURCES = [1, 63, 64, 65, 4097]   # around one wave, around one 4096-query moments part


def _transform():
    a = np.deg2rad(1.0)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = [0.1, -0.05, 0.02]
    return T


T_STEP = _transform()


def _cloud(n, seed):
    return np.random.default_rng(seed).normal(size=(n, 3)) * [20.0, 20.0, 5.0]


def _stats_bytes(st):
    return bytes(memoryview(st))


def _three_iterates(icp, ctx):
    """Three iterates, the second and third with a transform applied; everything a caller can read."""
    out = []
    for it in range(3):
        st = ctx.iterate(None if it == 0 else T_STEP, it, icp.RULES_ENGINE, 3.0)
        out.append(_stats_bytes(st))
    return out


@pytest.fixture(scope="module")
def ctxs(icp):
    with icp.Context(0) as host, icp.Context(0) as dev:
        yield host, dev


@pytest.mark.parametrize("n_src", SOURCES)
@pytest.mark.parametrize("n_tgt", TARGETS)
def test_iterates_match_host_calls(icp, ctxs, n_tgt, n_src):
    host, dev = ctxs
    tgt, src = _cloud(n_tgt, 1), _cloud(n_src, 2)
    host.set_target(tgt, 10, 20, icp.RULES_ENGINE)
    host.set_source(src)
    d_tgt, d_src = dev.to_device(tgt), dev.to_device(src)
    dev.set_target_device(d_tgt, n_tgt, 10, 20, icp.RULES_ENGINE)
    dev.set_source_device(d_src, n_src)
    # inputs are never written and never retained
    assert d_tgt.download(np.float64).tobytes() == tgt.tobytes()
    assert d_src.download(np.float64).tobytes() == src.tobytes()
    d_tgt.free()
    d_src.free()
    assert host.target_info() == dev.target_info()
    assert dev.target_build_info()[0] is True

    assert _three_iterates(icp, host) == _three_iterates(icp, dev)
    h_idx, h_d = host.get_correspondences()
    h_moved = host.get_source()
    # host getters of the device-fed context
    idx, d = dev.get_correspondences()
    assert np.array_equal(idx, h_idx) and d.tobytes() == h_d.tobytes()
    assert dev.get_source().tobytes() == h_moved.tobytes()
    # device getters, downloaded with dev_copy
    with dev.device_buffer(24 * n_src) as b_xyz, dev.device_buffer(4 * n_src) as b_idx, \
            dev.device_buffer(8 * n_src) as b_d:
        dev.get_source_device(b_xyz)
        assert b_xyz.download(np.float64).tobytes() == h_moved.tobytes()
        dev.get_correspondences_device(b_idx, b_d)
        assert np.array_equal(b_idx.download(np.int32), h_idx)
        assert b_d.download(np.float64).tobytes() == h_d.tobytes()
        # either output may be null: the other is written, the absent one untouched
        b_idx.upload(np.full(n_src, -7, np.int32))
        b_d.upload(np.full(n_src, -7.0))
        dev.get_correspondences_device(None, b_d)
        assert np.all(b_idx.download(np.int32) == -7) and b_d.download(np.float64).tobytes() == h_d.tobytes()
        b_d.upload(np.full(n_src, -7.0))
        dev.get_correspondences_device(b_idx, None)
        assert np.array_equal(b_idx.download(np.int32), h_idx) and np.all(b_d.download(np.float64) == -7.0)
        # and on the host-fed context as well
        host.get_source_device(b_xyz)
        assert b_xyz.download(np.float64).tobytes() == h_moved.tobytes()


@pytest.mark.parametrize("n_q", [1, 64, 1000])
def test_nn_device_matches_nn(icp, ctxs, n_q):
    host, dev = ctxs
    tgt = _cloud(5000, 3)
    rng = np.random.default_rng(4)
    q = np.ascontiguousarray(rng.permutation(_cloud(1000, 5))[:n_q])
    host.set_target(tgt, 10, 20, icp.RULES_ENGINE)
    with dev.to_device(tgt) as d_tgt:
        dev.set_target_device(d_tgt, len(tgt), 10, 20, icp.RULES_ENGINE)
    h_idx, h_d = host.nn(q)
    with dev.to_device(q) as d_q, dev.device_buffer(4 * n_q) as b_idx, dev.device_buffer(8 * n_q) as b_d:
        dev.nn_device(d_q, n_q, b_idx, b_d)
        assert np.array_equal(b_idx.download(np.int32), h_idx)
        assert b_d.download(np.float64).tobytes() == h_d.tobytes()
        assert d_q.download(np.float64).tobytes() == q.tobytes()
        b_idx.upload(np.full(n_q, -7, np.int32))
        b_d.upload(np.full(n_q, -7.0))
        dev.nn_device(d_q, n_q, None, b_d)
        assert np.all(b_idx.download(np.int32) == -7) and b_d.download(np.float64).tobytes() == h_d.tobytes()
        b_d.upload(np.full(n_q, -7.0))
        dev.nn_device(d_q, n_q, b_idx, None)
        assert np.array_equal(b_idx.download(np.int32), h_idx) and np.all(b_d.download(np.float64) == -7.0)
        dev.nn_device(d_q, n_q, None, None)
        # the host-fed context searches device queries too
        host.nn_device(d_q, n_q, b_idx, b_d)
        assert np.array_equal(b_idx.download(np.int32), h_idx)
        assert b_d.download(np.float64).tobytes() == h_d.tobytes()


def _run_all(icp, ctx, tgt, src, max_depth, device):
    """Set, three iterates, every getter; through the device entry points or the host ones."""
    n_t, n_s = len(tgt), len(src)
    if device:
        with ctx.to_device(tgt) as d_tgt, ctx.to_device(src) as d_src:
            ctx.set_target_device(d_tgt, n_t, 10, max_depth, icp.RULES_ENGINE)
            ctx.set_source_device(d_src, n_s)
            assert d_tgt.download(np.float64).tobytes() == tgt.tobytes()
            assert d_src.download(np.float64).tobytes() == src.tobytes()
    else:
        ctx.set_target(tgt, 10, max_depth, icp.RULES_ENGINE)
        ctx.set_source(src)
    stats = _three_iterates(icp, ctx)
    q = np.ascontiguousarray(src[:100])
    if device:
        with ctx.device_buffer(24 * n_s) as b_xyz, ctx.device_buffer(4 * n_s) as b_idx, \
                ctx.device_buffer(8 * n_s) as b_d, ctx.to_device(q) as d_q:
            ctx.get_source_device(b_xyz)
            ctx.get_correspondences_device(b_idx, b_d)
            moved, idx, d = b_xyz.download(np.float64, (n_s, 3)), b_idx.download(np.int32), b_d.download(np.float64)
            ctx.nn_device(d_q, len(q), b_idx, b_d)
            nn_idx, nn_d = b_idx.download(np.int32, (len(q),)), b_d.download(np.float64, (len(q),))
    else:
        moved = ctx.get_source()
        idx, d = ctx.get_correspondences()
        nn_idx, nn_d = ctx.nn(q)
    return stats, idx.tobytes(), d.tobytes(), moved.tobytes(), nn_idx.tobytes(), nn_d.tobytes(), ctx.target_build_info()[0]


@pytest.mark.parametrize("route", ["build_host", "max_depth_22", "query_order_host", "group_0_0"])
def test_host_staged_routes_match_host_calls(icp, route):
    """The routes that need the cloud in host memory stage the device buffer down: same outputs."""
    tgt, src = _cloud(5000, 6), _cloud(4097, 7)
    cfg, max_depth, devices = None, 20, None
    if route == "build_host":
        cfg = {"octree_builder": icp.BUILD_HOST}
    elif route == "max_depth_22":
        max_depth = 22
    elif route == "query_order_host":
        cfg = {"query_order": 1}
    else:
        devices = [0, 0]
    results = []
    for device in (False, True):
        if devices is None:
            ctx = icp.Context(0, cfg)
        else:
            ctx = icp.Context(devices=devices, transport=icp.XPORT_HOST)
        with ctx:
            results.append(_run_all(icp, ctx, tgt, src, max_depth, device))
    assert results[0] == results[1]
    assert results[1][-1] is (route in ("query_order_host", "group_0_0"))  # which builder made the tree


def _iterate_ok(icp, ctx, mirror):
    """One more iterate on the context: it is still usable, and computes what a context fed through
    the host calls computes after as many iterates (mirror, stepped along with it)."""
    assert _stats_bytes(ctx.iterate(None, 1, icp.RULES_ENGINE, 3.0)) == \
        _stats_bytes(mirror.iterate(None, 1, icp.RULES_ENGINE, 3.0))


def test_rejected_arguments_leave_the_context_usable(icp):
    L = icp.lib()
    tgt, src = _cloud(5000, 8), _cloud(1000, 9)
    with icp.Context(0) as host, icp.Context(0) as ctx, icp.Context(0) as mirror:
        d_tgt, d_src = ctx.to_device(tgt), ctx.to_device(src)
        ctx.set_target_device(d_tgt, len(tgt))
        ctx.set_source_device(d_src, len(src))
        mirror.set_target(tgt)
        mirror.set_source(src)
        _iterate_ok(icp, ctx, mirror)
        h = ctx.handle
        b_idx, b_d = ctx.device_buffer(4 * len(src) + 8), ctx.device_buffer(8 * len(src) + 8)
        host_arr = np.zeros((len(src), 3))  # pageable host memory: not a device pointer
        host_ptr = C.c_void_p(host_arr.ctypes.data)
        off4 = lambda b: C.c_void_p(b.ptr + 4)  # noqa: E731
        off2 = lambda b: C.c_void_p(b.ptr + 2)  # noqa: E731
        P = lambda b: C.c_void_p(b.ptr)  # noqa: E731
        n_t, n_s = len(tgt), len(src)
        bad_calls = {
            "set_target null": lambda: L.icp_hip_set_target_device(h, None, n_t, 10, 20, 0),
            "set_target n<0": lambda: L.icp_hip_set_target_device(h, P(d_tgt), -1, 10, 20, 0),
            "set_target n=0": lambda: L.icp_hip_set_target_device(h, P(d_tgt), 0, 10, 20, 0),
            "set_target depth": lambda: L.icp_hip_set_target_device(h, P(d_tgt), n_t, 10, 61, 0),
            "set_target +4": lambda: L.icp_hip_set_target_device(h, off4(d_tgt), n_t - 1, 10, 20, 0),
            "set_target host": lambda: L.icp_hip_set_target_device(h, host_ptr, n_s, 10, 20, 0),
            "set_source null": lambda: L.icp_hip_set_source_device(h, None, n_s),
            "set_source n<0": lambda: L.icp_hip_set_source_device(h, P(d_src), -1),
            "set_source 2^29": lambda: L.icp_hip_set_source_device(h, P(d_src), 1 << 29),
            "set_source +4": lambda: L.icp_hip_set_source_device(h, off4(d_src), n_s - 1),
            "set_source host": lambda: L.icp_hip_set_source_device(h, host_ptr, n_s),
            "get_source null": lambda: L.icp_hip_get_source_device(h, None),
            "get_source +4": lambda: L.icp_hip_get_source_device(h, off4(d_src)),
            "get_source host": lambda: L.icp_hip_get_source_device(h, host_ptr),
            "get_corr idx +2": lambda: L.icp_hip_get_correspondences_device(h, off2(b_idx), None),
            "get_corr dist +4": lambda: L.icp_hip_get_correspondences_device(h, None, off4(b_d)),
            "get_corr host": lambda: L.icp_hip_get_correspondences_device(h, host_ptr, None),
            "nn null": lambda: L.icp_hip_nn_device(h, None, n_s, P(b_idx), P(b_d)),
            "nn n<0": lambda: L.icp_hip_nn_device(h, P(d_src), -1, P(b_idx), P(b_d)),
            "nn +4": lambda: L.icp_hip_nn_device(h, off4(d_src), n_s - 1, P(b_idx), P(b_d)),
            "nn host": lambda: L.icp_hip_nn_device(h, host_ptr, n_s, P(b_idx), P(b_d)),
            "nn host out": lambda: L.icp_hip_nn_device(h, P(d_src), n_s, P(b_idx), host_ptr),
        }
        for name, call in bad_calls.items():
            assert call() == icp.EINVAL, name
            assert L.icp_hip_last_error(), name
            _iterate_ok(icp, ctx, mirror)
        # nothing above reached a kernel or a copy: the buffers hold what was uploaded
        assert d_tgt.download(np.float64).tobytes() == tgt.tobytes()
        assert d_src.download(np.float64).tobytes() == src.tobytes()

        # A non-finite coordinate is found by the device builder: the same code and message as the
        # host call's, and, as after the host call, the context is left without a target.
        bad = tgt.copy()
        bad[1234, 1] = np.nan
        with pytest.raises(icp.IcpError) as e_host:
            host.set_target(bad)
        with ctx.to_device(bad) as d_bad, pytest.raises(icp.IcpError) as e_dev:
            ctx.set_target_device(d_bad, n_t)
        assert e_dev.value.code == e_host.value.code == icp.EINVAL
        assert str(e_dev.value) == str(e_host.value)
        # without a target as a whole: no nodes, and no build to report
        assert ctx.target_info()["n_nodes"] == 0
        with pytest.raises(icp.IcpError) as e_info:
            ctx.target_build_info()
        assert e_info.value.code == icp.ENOTREADY
        with pytest.raises(icp.IcpError) as e_it:
            ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)
        assert e_it.value.code == icp.ENOTREADY
        ctx.set_target_device(d_tgt, n_t)
        mirror.set_target(tgt)
        _iterate_ok(icp, ctx, mirror)
        for b in (d_tgt, d_src, b_idx, b_d):
            b.free()


def test_dev_copy_round_trip_and_directions(icp, gpu_ctx):
    a = np.arange(1000, dtype=np.float64)
    with gpu_ctx.to_device(a) as src, gpu_ctx.device_buffer(a.nbytes) as dst:
        L = icp.lib()
        assert L.icp_hip_dev_copy(gpu_ctx.handle, C.c_void_p(dst.ptr), C.c_void_p(src.ptr), a.nbytes, icp.COPY_D2D) == 0
        assert np.array_equal(dst.download(np.float64), a)
        assert L.icp_hip_dev_copy(gpu_ctx.handle, C.c_void_p(dst.ptr), C.c_void_p(src.ptr), a.nbytes, 3) == icp.EINVAL
        assert L.icp_hip_dev_free(gpu_ctx.handle, None) == 0
