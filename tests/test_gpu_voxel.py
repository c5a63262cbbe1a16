"""Voxel-grid down-sampling on the device (icp_hip_voxel_downsample and its _device variant): every
shared case of tests/voxel_reference.py bit-identical to the numpy model and to the host function,
one voxel of 200 000 points (a serial run would show), determinism, the device-pointer contract, the
rejected inputs, and a context whose resident clouds and iterate the call leaves alone."""
import numpy as np
import pytest

import voxel_reference as vr

pytestmark = pytest.mark.gpu


def _einval(icp, call, text=None):
    with pytest.raises(icp.IcpError) as e:
        call()
    assert e.value.code == icp.EINVAL, str(e.value)
    if text:
        assert text in str(e.value), str(e.value)
    return e.value


@pytest.mark.parametrize("name", vr.CASE_NAMES)
def test_context_matches_model_and_host(icp, gpu_ctx, name):
    xyz, h, origin, mode = vr.cases(icp)[name]
    p, f, k, o = gpu_ctx.voxel_downsample(xyz, h, origin=origin, mode=mode)
    ep, ef, ek, _, eo = vr.expected(icp, name)
    assert np.array_equal(o, eo)
    assert len(p) == len(ep) and vr.same_bits(f, ef) and vr.same_bits(k, ek)
    assert vr.same_bits(p, ep), f"{np.count_nonzero(p != ep)} coordinates differ from the model"
    hp, hf, hk, ho = icp.voxel_downsample(xyz, h, origin=origin, mode=mode)
    assert vr.same_bits(p, hp) and vr.same_bits(f, hf) and vr.same_bits(k, hk) and vr.same_bits(o, ho)


def test_one_voxel_of_200000_points(icp, gpu_ctx):
    xyz = np.random.default_rng(77).uniform(0.0, 0.9, (200000, 3)) + [5.4e6, 4.1e5, 300.0]
    p, f, k, o = gpu_ctx.voxel_downsample(xyz, 1.0)
    ep, ef, ek, _ = vr.model(xyz, 1.0, o)
    assert list(k) == [200000] and list(f) == [0] and vr.same_bits(k, ek) and vr.same_bits(f, ef)
    assert vr.same_bits(p, ep)


def test_two_calls_give_the_same_bytes(icp, gpu_ctx):
    xyz, h, _, _ = vr.cases(icp)["blob_coarse"]
    a = gpu_ctx.voxel_downsample(xyz, h)
    b = gpu_ctx.voxel_downsample(xyz, h)
    assert all(vr.same_bits(u, v) for u, v in zip(a, b))


@pytest.fixture(scope="module")
def dev_case(icp, gpu_ctx):
    """The coarse blob resident in HBM with the host variant's answer."""
    xyz, h, _, _ = vr.cases(icp)["blob_coarse"]
    want = gpu_ctx.voxel_downsample(xyz, h)
    buf = gpu_ctx.to_device(xyz)
    yield xyz, h, want, buf
    buf.free()


def test_device_variant_matches_the_host_variant(icp, gpu_ctx, dev_case):
    xyz, h, (p, f, k, o), buf = dev_case
    n, m = len(xyz), len(p)
    cap = m + 5
    dp, df, dk = gpu_ctx.device_buffer(24 * cap), gpu_ctx.device_buffer(4 * cap), gpu_ctx.device_buffer(4 * cap)
    for b in (dp, df, dk):
        b.upload(np.full(b.nbytes, 0xA5, np.uint8))
    got_m, got_o = gpu_ctx.voxel_downsample_device(buf, n, h, cap=cap, d_xyz_out=dp, d_first_out=df, d_count_out=dk)
    assert got_m == m and vr.same_bits(got_o, o)
    assert vr.same_bits(dp.download(np.float64, (cap, 3))[:m], p)
    assert vr.same_bits(df.download(np.int32)[:m], f) and vr.same_bits(dk.download(np.int32)[:m], k)
    assert (dp.download(np.uint8)[24 * m:] == 0xA5).all() and (df.download(np.uint8)[4 * m:] == 0xA5).all()
    assert vr.same_bits(buf.download(np.float64, (n, 3)), xyz)  # the input is never written
    for b in (dp, df, dk):
        b.free()


def test_device_variant_honours_null_outputs(icp, gpu_ctx, dev_case):
    xyz, h, (p, f, k, o), buf = dev_case
    n, m = len(xyz), len(p)
    assert gpu_ctx.voxel_downsample_device(buf, n, h)[0] == m  # count only, whatever cap says
    dk = gpu_ctx.device_buffer(4 * m)
    assert gpu_ctx.voxel_downsample_device(buf, n, h, cap=m, d_count_out=dk)[0] == m
    assert vr.same_bits(dk.download(np.int32), k)
    dp = gpu_ctx.device_buffer(24 * m)
    assert gpu_ctx.voxel_downsample_device(buf, n, h, mode=icp.VOXEL_FIRST, cap=m, d_xyz_out=dp)[0] == m
    assert vr.same_bits(dp.download(np.float64, (m, 3)), xyz[f])
    dk.free()
    dp.free()


def test_device_variant_capacity_and_pointer_checks(icp, gpu_ctx, dev_case):
    xyz, h, (p, f, k, o), buf = dev_case
    n, m = len(xyz), len(p)
    dp = gpu_ctx.device_buffer(24 * m)
    dp.upload(np.full(dp.nbytes, 0xA5, np.uint8))
    e = _einval(icp, lambda: gpu_ctx.voxel_downsample_device(buf, n, h, cap=m - 1, d_xyz_out=dp), "capacity")
    assert e.m == m
    assert (dp.download(np.uint8) == 0xA5).all()  # untouched
    host = np.zeros((m, 3))
    _einval(icp, lambda: gpu_ctx.voxel_downsample_device(xyz.ctypes.data, n, h))
    _einval(icp, lambda: gpu_ctx.voxel_downsample_device(buf, n, h, cap=m, d_xyz_out=host.ctypes.data))
    _einval(icp, lambda: gpu_ctx.voxel_downsample_device(buf.ptr + 4, n - 1, h))  # not 8-byte aligned
    _einval(icp, lambda: gpu_ctx.voxel_downsample_device(None, n, h))
    dp.free()


def test_rejected_inputs_through_the_context(icp, gpu_ctx):
    blob = vr.cases(icp)["blob"][0][:500]
    for h in (0.0, -1.0, float("nan"), float("inf")):
        _einval(icp, lambda: gpu_ctx.voxel_downsample(blob, h))
    _einval(icp, lambda: gpu_ctx.voxel_downsample(np.empty((0, 3)), 0.5))
    bad = blob.copy()
    bad[3, 1] = np.nan
    bad[9, 0] = np.inf
    _einval(icp, lambda: gpu_ctx.voxel_downsample(bad, 0.5), "2 non-finite")
    _einval(icp, lambda: gpu_ctx.voxel_downsample(blob, 0.5, origin=blob.min(0) + [0.0, 0.1, 0.0]), "below")
    _einval(icp, lambda: gpu_ctx.voxel_downsample(blob, 0.5, mode=2), "mode")
    h = 0.5
    two = np.array([[0.0, 1.0, 0.0], [0.0, 1.0 + 2 ** 21 * h, 0.0]])
    _einval(icp, lambda: gpu_ctx.voxel_downsample(two, h), "too fine")
    two[1, 1] = 1.0 + (2 ** 21 - 1) * h
    p, f, k, _ = gpu_ctx.voxel_downsample(two, h)
    assert len(p) == 2 and list(f) == [0, 1] and list(k) == [1, 1]
    m, _ = gpu_ctx.voxel_downsample(blob, 0.5, count_only=True)
    e = _einval(icp, lambda: gpu_ctx.voxel_downsample(blob, 0.5, cap=m - 1), "capacity")
    assert e.m == m == len(icp.voxel_downsample(blob, 0.5)[0])


def test_resident_clouds_and_iterate_are_unaffected(icp):
    tgt, src, _ = icp.synth_pair(5000, yaw_deg=3.0)
    with icp.Context(0) as ctx:
        ctx.set_target(tgt)
        ctx.set_source(src)
        st = ctx.iterate(None, 0, icp.RULES_ENGINE, 3.0)
        ctx.iterate(icp.best_fit_from_stats(st), 1, icp.RULES_ENGINE, 3.0)
        idx0, d0 = ctx.get_correspondences()
        moved0 = ctx.get_source()
        p, f, k, _ = ctx.voxel_downsample(tgt, 0.5)
        assert vr.same_bits(p, icp.voxel_downsample(tgt, 0.5)[0])
        idx1, d1 = ctx.get_correspondences()
        assert vr.same_bits(idx0, idx1) and vr.same_bits(d0, d1) and vr.same_bits(moved0, ctx.get_source())
        st2 = ctx.iterate(None, 2, icp.RULES_ENGINE, 3.0)  # and the context still iterates
        assert st2.n == len(src)


def test_multi_device_context_answers_as_a_plain_one(icp, gpu_ctx):
    xyz, h, _, _ = vr.cases(icp)["blob"]
    want = gpu_ctx.voxel_downsample(xyz, h)
    with icp.Context(devices=[0, 0], transport=icp.XPORT_HOST) as ctx:
        got = ctx.voxel_downsample(xyz, h)
        assert all(vr.same_bits(u, v) for u, v in zip(got, want))
        m = len(want[0])
        buf, dp = ctx.to_device(xyz), ctx.device_buffer(24 * m)
        assert ctx.voxel_downsample_device(buf, len(xyz), h, cap=m, d_xyz_out=dp)[0] == m
        assert vr.same_bits(dp.download(np.float64, (m, 3)), want[0])
        buf.free()
        dp.free()
