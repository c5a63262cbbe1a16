"""The calls that own device memory for their own length (csrc/dev_scratch.h), repeated on one
context: set_target, set_source, an iterate, get_source, get_correspondences, nn / nn_device with
each output null in turn, knn / knn_device with k = 1 and 16, estimate_target_normals,
set_target_normals / get_target_normals in host and device forms, plane_sums, and the cloud filters
voxel_downsample and outlier_filter (statistical with k = 1 and min(16, n - 1), radius) with their
_device forms, each output null in turn and all null.

A second pass of the sequence on a context that has already run it must return the bytes of the
first pass, and both the bytes of a fresh context: a scratch buffer released before the work that
uses it, or a result read before its copy has landed, shows as a difference (freed memory is handed
out again by the next allocation of the sequence). Every host output is filled with a sentinel
before its call. Nothing here is compared with a tolerance: the three runs are the same
computation.

Target: 1000 points; sources and query sets of 1, 63, 64, 65 and 193 points (one lane, a wave less
one, a wave, a wave and one, three waves and one: the wave and follow-list edges of
test_gpu_follow_lists.py). The same on a two-member group on device 0 with the host transport, for
the routes staged through host memory; there a source of one point and plane_sums are usage errors
by the interface (one point per device at least; the sums are not exchanged), which is asserted.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TGT = 1000
SIZES = (1, 63, 64, 65, 193)
KS = (1, 16)


def _clouds(n):
    scale = [20.0, 20.0, 5.0]
    tgt = np.random.default_rng(1000).normal(size=(N_TGT, 3)) * scale
    src = np.random.default_rng(2000 + n).normal(size=(n, 3)) * scale
    q = np.random.default_rng(3000 + n).normal(size=(n, 3)) * scale
    return tgt, src, q


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _d(b):
    return None if b is None else C.c_void_p(b.ptr)


def _kept_untouched(m, cap_arrays, want):
    """Past m, and wherever it was not asked for, an output still holds its sentinel."""
    for a, w in zip(cap_arrays, want):
        rest = a[m if w else 0:]
        assert np.isnan(rest).all() if a.dtype.kind == "f" else (rest == -7).all()


def _filters(icp, ctx, q, n, out):
    """The voxel grid and the outlier filters on q, host and device forms, every choice of outputs."""
    L, h = icp.lib(), ctx.handle
    choices = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0))
    sent = (np.full((n, 3), np.nan), np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, np.nan))
    modes = (("sor 1", icp.OUTLIER_STATISTICAL, 1, 1.0), (f"sor {min(16, n - 1)}", icp.OUTLIER_STATISTICAL, min(16, n - 1), 1.0),
             ("radius", icp.OUTLIER_RADIUS, 1, 5.0))
    with ctx.to_device(q) as d_q, ctx.device_buffer(24 * n) as d_p, ctx.device_buffer(4 * n) as d_a, \
            ctx.device_buffer(4 * n) as d_b, ctx.device_buffer(8 * n) as d_s:
        def fill():
            for buf, a in zip((d_p, d_a, d_b, d_s), sent):
                buf.upload(a)
            return [a.copy() for a in sent]

        def down():
            return [d_p.download(np.float64, (n, 3)), d_a.download(np.int32, (n,)), d_b.download(np.int32, (n,)),
                    d_s.download(np.float64, (n,))]

        for want in choices:
            name = "voxel " + "".join(map(str, want))
            p, f, k, _ = fill()
            m, org = C.c_int64(-1), np.full(3, np.nan)
            assert L.icp_hip_voxel_downsample(h, _p(q), n, 5.0, None, icp.VOXEL_CENTROID, n, _p(p) if want[0] else None,
                                              _p(f) if want[1] else None, _p(k) if want[2] else None, C.byref(m),
                                              _p(org)) == 0
            assert 1 <= m.value <= n
            _kept_untouched(m.value, (p, f, k), want)
            out[name] = bytes(m) + org.tobytes() + p.tobytes() + f.tobytes() + k.tobytes()
            m, org = C.c_int64(-1), np.full(3, np.nan)
            assert L.icp_hip_voxel_downsample_device(h, _d(d_q), n, 5.0, None, icp.VOXEL_CENTROID, n,
                                                     _d(d_p) if want[0] else None, _d(d_a) if want[1] else None,
                                                     _d(d_b) if want[2] else None, C.byref(m), _p(org)) == 0
            p, f, k, _ = down()
            out[name + " device"] = bytes(m) + org.tobytes() + p.tobytes() + f.tobytes() + k.tobytes()
            assert out[name + " device"] == out[name]
        for label, mode, k, param in modes if n >= 2 else ():
            for want in choices:
                name = f"outlier {label} " + "".join(map(str, want))
                p, ix, _, sc = fill()
                m, st = C.c_int64(-1), icp.OutlierStats()
                assert L.icp_hip_outlier_filter(h, _p(q), n, mode, k, param, n, _p(p) if want[0] else None,
                                                _p(ix) if want[1] else None, _p(sc) if want[2] else None, C.byref(m),
                                                C.byref(st)) == 0
                assert 0 <= m.value <= n and st.n == n and st.kept == m.value
                _kept_untouched(m.value, (p, ix), want)
                assert np.isnan(sc).all() if not want[2] else not np.isnan(sc).any()
                out[name] = bytes(m) + bytes(st) + p.tobytes() + ix.tobytes() + sc.tobytes()
                m, st = C.c_int64(-1), icp.OutlierStats()
                assert L.icp_hip_outlier_filter_device(h, _d(d_q), n, mode, k, param, n, _d(d_p) if want[0] else None,
                                                       _d(d_a) if want[1] else None, _d(d_s) if want[2] else None,
                                                       C.byref(m), C.byref(st)) == 0
                p, ix, _, sc = down()
                out[name + " device"] = bytes(m) + bytes(st) + p.tobytes() + ix.tobytes() + sc.tobytes()
                assert out[name + " device"] == out[name]
        if n < 2:  # a usage error by the interface, in both forms; m is reported as 0
            for call, cloud, outs in ((L.icp_hip_outlier_filter, _p(q), (_p(sent[0].copy()), None, None)),
                                      (L.icp_hip_outlier_filter_device, _d(d_q), (_d(d_p), None, None))):
                m = C.c_int64(-1)
                assert call(h, cloud, n, icp.OUTLIER_STATISTICAL, 1, 1.0, n, *outs, C.byref(m), None) == icp.EINVAL
                assert m.value == 0
        assert d_q.download(np.float64).tobytes() == q.tobytes()  # inputs are never written


def _sequence(icp, ctx, n, group):
    """One pass; every output as bytes, by name."""
    L, h = icp.lib(), ctx.handle
    tgt, src, q = _clouds(n)
    out = {}
    ctx.set_target(tgt, 10, 20, icp.RULES_ENGINE)
    if group and n < 2:
        with pytest.raises(icp.IcpError) as e:
            ctx.set_source(src)
        assert e.value.code == icp.EINVAL
    else:
        ctx.set_source(src)
        out["stats"] = bytes(memoryview(ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)))
        moved = np.full((n, 3), np.nan)
        assert L.icp_hip_get_source(h, _p(moved)) == 0
        out["source"] = moved.tobytes()
        for name, wi, wd in (("both", 1, 1), ("idx", 1, 0), ("dist", 0, 1)):
            i, d = np.full(n, -7, np.int32), np.full(n, np.nan)
            assert L.icp_hip_get_correspondences(h, _p(i) if wi else None, _p(d) if wd else None) == 0
            out["corr " + name] = i.tobytes() + d.tobytes()
    with ctx.to_device(q) as d_q, ctx.device_buffer(4 * n * max(KS)) as d_i, ctx.device_buffer(8 * n * max(KS)) as d_d:
        for name, wi, wd in (("both", 1, 1), ("idx", 1, 0), ("dist", 0, 1)):
            i, d = np.full(n, -7, np.int32), np.full(n, np.nan)
            assert L.icp_hip_nn(h, _p(q), n, _p(i) if wi else None, _p(d) if wd else None) == 0
            out["nn " + name] = i.tobytes() + d.tobytes()
            d_i.upload(np.full(n, -7, np.int32))
            d_d.upload(np.full(n, np.nan))
            assert L.icp_hip_nn_device(h, _d(d_q), n, _d(d_i) if wi else None, _d(d_d) if wd else None) == 0
            out["nn_device " + name] = d_i.download(np.int32, (n,)).tobytes() + d_d.download(np.float64, (n,)).tobytes()
            assert out["nn_device " + name] == out["nn " + name]
        for k in KS:
            i, d2 = np.full((n, k), -7, np.int32), np.full((n, k), np.nan)
            assert L.icp_hip_knn(h, _p(q), n, k, _p(i), _p(d2)) == 0
            out[f"knn {k}"] = i.tobytes() + d2.tobytes()
            d_i.upload(np.full(n * k, -7, np.int32))
            d_d.upload(np.full(n * k, np.nan))
            assert L.icp_hip_knn_device(h, _d(d_q), n, k, _d(d_i), _d(d_d)) == 0
            out[f"knn_device {k}"] = d_i.download(np.int32, (n * k,)).tobytes() + d_d.download(np.float64, (n * k,)).tobytes()
            assert out[f"knn_device {k}"] == out[f"knn {k}"]
        assert d_q.download(np.float64).tobytes() == q.tobytes()  # inputs are never written
    ctx.estimate_target_normals(16)
    est = np.full((N_TGT, 3), np.nan)
    assert L.icp_hip_get_target_normals(h, _p(est)) == 0
    out["normals estimated"] = est.tobytes()
    given = np.roll(est, 1, axis=0)  # unit length or zero, and not what the context holds
    ctx.set_target_normals(given)
    with ctx.device_buffer(24 * N_TGT) as d_n:
        d_n.upload(np.full(3 * N_TGT, np.nan))
        ctx.get_target_normals(d_n)
        out["normals set host, get device"] = d_n.download(np.float64).tobytes()
        assert out["normals set host, get device"] == given.tobytes()
        ctx.estimate_target_normals(16)  # something else in between
        ctx.set_target_normals(d_n)
    back = np.full((N_TGT, 3), np.nan)
    assert L.icp_hip_get_target_normals(h, _p(back)) == 0
    out["normals set device, get host"] = back.tobytes()
    assert back.tobytes() == given.tobytes()
    if group:
        with pytest.raises(icp.IcpError) as e:
            ctx.plane_sums()
        assert e.value.code == icp.EINVAL
    elif "stats" in out:
        out["plane_sums"] = bytes(memoryview(ctx.plane_sums(src.mean(0))))
    _filters(icp, ctx, q, n, out)
    return out


def _check_passes(icp, make, n, group):
    with make() as ctx:
        first = _sequence(icp, ctx, n, group)
        second = _sequence(icp, ctx, n, group)
    with make() as fresh:
        third = _sequence(icp, fresh, n, group)
    assert first.keys() == second.keys() == third.keys()
    for name in first:
        assert second[name] == first[name], f"{name}: the second pass differs from the first"
        assert third[name] == first[name], f"{name}: a fresh context differs"
    return first


@pytest.mark.parametrize("n", SIZES)
def test_repeated_calls_return_the_same_bytes(icp, n):
    out = _check_passes(icp, lambda: icp.Context(0), n, False)
    assert "plane_sums" in out and "knn_device 16" in out
    assert "voxel 000 device" in out and ("outlier radius 110 device" in out) == (n >= 2)


@pytest.mark.parametrize("n", SIZES)
def test_repeated_calls_on_a_group_of_two(icp, n):
    out = _check_passes(icp, lambda: icp.Context(devices=[0, 0], transport=icp.XPORT_HOST), n, True)
    assert ("stats" in out) == (n >= 2) and "knn_device 16" in out
    assert "voxel 000 device" in out and ("outlier radius 110 device" in out) == (n >= 2)
