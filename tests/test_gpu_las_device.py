"""LAS records decoded and encoded on the device (icp_hip_*_las, include/icp_las.h) against the
host reader and writers (lasio.cpp), which are the specification: points bit for bit, files byte
for byte, no tolerance anywhere.

Decode inputs. X, Y, Z alternate between draws over the whole int32 range (INT32_MIN, INT32_MAX, 0
and -1 first) and values within 4096 steps of -offset / scale, where X * scale cancels against
the offset. The second half is what makes the comparison see a contracted kernel: over whole-range
draws alone, a fused multiply-add gives the host reader's bits in all but 0.02 % of the
coordinates (the product's rounding error vanishes below the sum's last bit); with the
cancelling half, exact rational arithmetic rounded once (= an FMA) differs from the plain fp64
X * scale + offset in 47.7 % of the coordinates (49.9 / 45.7 / 47.5 % for the three axes' scale
and offset, measured on 2000 draws per axis with numpy and fractions.Fraction).

The staging chunks are set to their minimum (64 KiB) so that the 10001- and 20007-record files
cross chunk boundaries as well as the host reader's 10000-record batches.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALE = (0.001, 0.01, 0.00025)
OFFSET = (512.0, -256.0, 10.0)
RECORD_LENGTHS = [12, 13, 20, 21, 26, 28, 34]
POINT_OFFSETS = [227, 230, 375]
COUNTS = [1, 63, 64, 65, 10001, 20007]
I32 = np.iinfo(np.int32)


def _strides(n):
    return [1, 2, 7, 50, n + 3]


@pytest.fixture(scope="module")
def ctx(icp):
    with icp.Context(0) as c:
        c.set_las_chunk_bytes(1 << 16)
        yield c


@pytest.fixture(scope="module")
def header(icp, tmp_path_factory):
    """The 227 header bytes of a file made by the existing writer."""
    p = tmp_path_factory.mktemp("las_hdr") / "one.las"
    icp.las_write_cli(p, np.zeros((1, 3)), SCALE, OFFSET)
    return p.read_bytes()[:227]


def _xyz_ints(n, rng):
    v = rng.integers(I32.min, int(I32.max) + 1, (n, 3), dtype=np.int64)
    for a in range(3):
        centre = int(round(-OFFSET[a] / SCALE[a]))
        v[1::2, a] = centre + rng.integers(-4096, 4097, len(v[1::2]))
    special = [I32.min, I32.max, 0, -1]
    for k in range(0, min(n, 8), 2):  # even rows: the odd ones hold the cancelling values
        v[k] = np.roll(special, k // 2)[:3]
    return v.astype(np.int32)


def _las_file(path, header, n, record_length, point_offset, rng, claim=None):
    """A LAS file with odd geometry: the writer's header patched at 96 / 105 / 107."""
    h = bytearray(header)
    h[96:100] = int(point_offset).to_bytes(4, "little")
    h[105:107] = int(record_length).to_bytes(2, "little")
    h[107:111] = int(n if claim is None else claim).to_bytes(4, "little")
    rec = rng.integers(0, 256, (n, record_length), dtype=np.uint8)
    ints = _xyz_ints(n, rng)
    if record_length >= 12:
        rec[:, :12] = ints.view(np.uint8).reshape(n, 12)
    gap = rng.integers(0, 256, point_offset - 227, dtype=np.uint8)
    path.write_bytes(bytes(h) + gap.tobytes() + rec.tobytes())
    return ints


def _device_read(ctx, path, rules, max_points, stride):
    buf, n, hdr = ctx.read_las_device(path, rules, max_points, stride)
    with buf:
        return buf.download(np.float64, (n, 3)), hdr


def _same_header(a, b):
    def fields(h):
        return (h.offset_to_points, h.num_points, h.record_length,
                np.array([h.scale[:], h.offset[:], h.max[:], h.min[:]]).tobytes())
    return fields(a) == fields(b)


@pytest.mark.parametrize("point_offset", POINT_OFFSETS)
@pytest.mark.parametrize("record_length", RECORD_LENGTHS)
def test_decode_matches_host_reader(icp, ctx, header, tmp_path, record_length, point_offset):
    rng = np.random.default_rng(1000 * record_length + point_offset)
    for n in COUNTS:
        path = tmp_path / f"r{record_length}_o{point_offset}_n{n}.las"
        ints = _las_file(path, header, n, record_length, point_offset, rng)
        ref, ref_hdr = icp.las_read(path, icp.LAS_CLI)
        assert len(ref) == n
        # the host reader itself: one multiply, one add (numpy does not fuse)
        want = ints.astype(np.float64) * np.array(SCALE) + np.array(OFFSET)
        assert ref.tobytes() == want.tobytes()
        for stride in _strides(n):
            got, hdr = _device_read(ctx, path, icp.LAS_CLI, 0, stride)
            assert ctx.last_las_path() == 1
            assert _same_header(hdr, ref_hdr)
            assert got.shape == ref[::stride].shape
            assert got.tobytes() == np.ascontiguousarray(ref[::stride]).tobytes(), (n, stride)


@pytest.mark.parametrize("n", COUNTS)
def test_decode_core_rules_max_points(icp, ctx, header, tmp_path, n):
    rng = np.random.default_rng(77 + n)
    path = tmp_path / f"core_n{n}.las"
    _las_file(path, header, n, 13, 230, rng)
    for max_points in (0, 1, n - 1, n + 5):
        ref, ref_hdr = icp.las_read(path, icp.LAS_CORE, max_points)
        for stride in (1, 7):
            got, hdr = _device_read(ctx, path, icp.LAS_CORE, max_points, stride)
            assert ctx.last_las_path() == 1 and _same_header(hdr, ref_hdr)
            assert got.tobytes() == np.ascontiguousarray(ref[::stride]).tobytes(), (max_points, stride)
    # CLI rules read the whole file whatever max_points says
    got, _ = _device_read(ctx, path, icp.LAS_CLI, 1, 1)
    assert got.tobytes() == icp.las_read(path, icp.LAS_CLI)[0].tobytes()


def test_decode_with_default_chunks(icp, header, tmp_path):
    rng = np.random.default_rng(5)
    path = tmp_path / "default_chunks.las"
    _las_file(path, header, 20007, 34, 375, rng)
    ref, _ = icp.las_read(path, icp.LAS_CLI)
    with icp.Context(0) as c:
        for stride in (1, 3, 50):
            got, _ = _device_read(c, path, icp.LAS_CLI, 0, stride)
            assert c.last_las_path() == 1
            assert got.tobytes() == np.ascontiguousarray(ref[::stride]).tobytes()


@pytest.mark.parametrize("case", ["five_records_short", "mid_record", "record_length_8"])
def test_decode_fallbacks_match_host_reader(icp, ctx, header, tmp_path, case):
    rng = np.random.default_rng(9)
    n = 10001
    path = tmp_path / f"{case}.las"
    if case == "record_length_8":
        _las_file(path, header, n, 8, 227, rng)
    else:
        _las_file(path, header, n, 26, 230, rng)
        blob = path.read_bytes()
        path.write_bytes(blob[:-5 * 26] if case == "five_records_short" else blob[:-11])
    ref, ref_hdr = icp.las_read(path, icp.LAS_CLI)
    assert len(ref) == n
    for stride in (1, 7):
        got, hdr = _device_read(ctx, path, icp.LAS_CLI, 0, stride)
        assert ctx.last_las_path() == 0
        assert _same_header(hdr, ref_hdr)
        assert got.tobytes() == np.ascontiguousarray(ref[::stride]).tobytes()


def test_decode_rejects_what_the_host_reader_rejects(icp, ctx, header, tmp_path):
    rng = np.random.default_rng(3)
    bad_sig = tmp_path / "bad_signature.las"
    _las_file(bad_sig, b"XXXX" + header[4:], 10, 20, 227, rng)
    empty = tmp_path / "claims_zero.las"
    _las_file(empty, header, 10, 20, 227, rng, claim=0)
    for path, rules in ((bad_sig, icp.LAS_CORE), (empty, icp.LAS_CLI), (tmp_path / "missing.las", icp.LAS_CLI)):
        with pytest.raises(icp.IcpError) as e:
            ctx.read_las_device(path, rules)
        assert e.value.code == icp.EINVAL
    with pytest.raises(icp.IcpError):
        ctx.read_las_device(bad_sig, icp.LAS_CLI, 0, 0)  # stride 0


def test_set_clouds_from_las_match_host_route(icp, ctx, header, tmp_path):
    """set_target_las / set_source_las against icp_las_read + the host setters, at a stride."""
    tgt, src, _ = icp.synth_pair(20007, 10001, yaw_deg=2.0)
    pt, ps = tmp_path / "t.las", tmp_path / "s.las"
    icp.las_write_cli(pt, tgt, (0.001,) * 3, (0.0,) * 3)
    icp.las_write_cli(ps, src, (0.001,) * 3, (0.0,) * 3)
    with icp.Context(0) as host:
        host.set_target(np.ascontiguousarray(icp.las_read(pt)[0][::3]), 10, 20, icp.RULES_CLI)
        host.set_source(np.ascontiguousarray(icp.las_read(ps)[0][::3]))
        n_t, _ = ctx.set_target_las(pt, icp.LAS_CLI, 0, 3, 10, 20, icp.RULES_CLI)
        n_s, _ = ctx.set_source_las(ps, icp.LAS_CLI, 0, 3)
        assert (n_t, n_s) == (6669, 3334) and ctx.last_las_path() == 1
        for it in range(2):
            a = host.iterate(None, it, icp.RULES_CLI, 3.0)
            b = ctx.iterate(None, it, icp.RULES_CLI, 3.0)
            assert bytes(memoryview(a)) == bytes(memoryview(b))
        assert host.get_source().tobytes() == ctx.get_source().tobytes()


# ------------------------------------------------------------------------------------ encode

def _boundary_cloud(n, scale, offset, rng):
    """Coordinates on truncation boundaries (offset + k * scale, k of both signs) and one ulp
    either side of them, so below the offset too (negative quotients truncate toward zero)."""
    k = rng.integers(-200000, 200001, (n, 3)).astype(np.float64)
    k[:4] = [[0, 1, -1], [1, -1, 0], [-1, 0, 1], [2, -2, 3]][: min(n, 4)] if n >= 4 else k[:4]
    v = k * np.array(scale) + np.array(offset)
    side = rng.integers(0, 3, (n, 3))
    v = np.where(side == 1, np.nextafter(v, np.inf), np.where(side == 2, np.nextafter(v, -np.inf), v))
    return np.ascontiguousarray(v)


def _write_both(icp, ctx, tmp_path, xyz, flavour, scale=None, offset=None, bounds=None, tag=""):
    """(device file bytes, host file bytes, route of the device call)."""
    dev_p, host_p = tmp_path / f"dev{tag}.las", tmp_path / f"host{tag}.las"
    with ctx.to_device(xyz) as d:
        ctx.write_las_device(dev_p, d, len(xyz), flavour, scale, offset, bounds)
        route = ctx.last_las_path()
        assert d.download(np.float64).tobytes() == xyz.tobytes()  # the input is not written
    if flavour == icp.LAS_CLI:
        icp.las_write_cli(host_p, xyz, scale, offset)
    else:
        icp.las_write_core(host_p, xyz, bounds)
    return dev_p.read_bytes(), host_p.read_bytes(), route


@pytest.mark.parametrize("n", [1, 64, 65, 10001])
def test_encode_matches_host_writers(icp, ctx, tmp_path, n):
    rng = np.random.default_rng(40 + n)
    xyz = _boundary_cloud(n, SCALE, OFFSET, rng)
    dev, host, route = _write_both(icp, ctx, tmp_path, xyz, icp.LAS_CLI, SCALE, OFFSET, tag="_cli")
    assert route == 1 and dev == host and len(dev) == 227 + 20 * n
    # core flavour: scale 0.001, offset = the cloud's minimum (boundaries of that grid)
    core = _boundary_cloud(n, (0.001,) * 3, (0.0,) * 3, rng) + 300.0
    dev, host, route = _write_both(icp, ctx, tmp_path, core, icp.LAS_CORE, tag="_core")
    assert route == 1 and dev == host
    # the caller's bounds as they stand: they do not contain the points (coordinates below the offset)
    bounds = np.array([core[:, 0].mean(), core[:, 0].mean() + 1.0, 299.5, 299.75, 1000.0, -1000.0])
    dev, host, route = _write_both(icp, ctx, tmp_path, core, icp.LAS_CORE, bounds=bounds, tag="_bounds")
    assert route == 1 and dev == host
    # the resident source, in the caller's order
    ctx.set_source(xyz)
    for flavour, kw in ((icp.LAS_CLI, dict(scale=SCALE, offset=OFFSET)), (icp.LAS_CORE, {}),
                        (icp.LAS_CORE, dict(bounds=bounds))):
        p = tmp_path / "src.las"
        ctx.write_source_las(p, flavour, **kw)
        assert ctx.last_las_path() == 1
        q = tmp_path / "src_host.las"
        if flavour == icp.LAS_CLI:
            icp.las_write_cli(q, xyz, SCALE, OFFSET)
        else:
            icp.las_write_core(q, xyz, kw.get("bounds"))
        assert p.read_bytes() == q.read_bytes()


@pytest.mark.parametrize("first", ["minus_zero_first", "plus_zero_first"])
@pytest.mark.parametrize("n", [2, 10001])
def test_encode_header_keeps_the_host_loops_zero(icp, ctx, tmp_path, n, first):
    """Minimum and maximum of an axis are -0.0 and +0.0: which one the header holds depends on the
    order the host loop met them in; the zeros sit in different runs of the device reduction."""
    a, b = (-0.0, 0.0) if first == "minus_zero_first" else (0.0, -0.0)
    xyz = np.zeros((n, 3))
    xyz[:, 0] = a
    xyz[n // 2:, 0] = b
    xyz[:, 1] = b
    xyz[-1, 1] = a
    xyz[:, 2] = np.linspace(-1.0, 1.0, n)
    for flavour, kw in ((icp.LAS_CLI, dict(scale=(0.001,) * 3, offset=(0.0,) * 3)), (icp.LAS_CORE, {})):
        dev, host, route = _write_both(icp, ctx, tmp_path, xyz, flavour, tag=f"_{flavour}", **kw)
        assert route == 1 and dev == host
        assert dev[179:227] == host[179:227]  # max / min x, y, z: the sign bits included


@pytest.mark.parametrize("what", ["nan", "inf", "quotient_3e9", "nan_first_point"])
@pytest.mark.parametrize("n", [65, 10001])
def test_encode_fallbacks_match_host_writers(icp, ctx, tmp_path, n, what):
    rng = np.random.default_rng(60 + n)
    xyz = _boundary_cloud(n, SCALE, OFFSET, rng)
    if what == "nan":
        xyz[n - 2, 1] = np.nan
    elif what == "inf":
        xyz[n // 2, 2] = -np.inf
    elif what == "nan_first_point":
        xyz[0, 0] = np.nan
    else:
        xyz[n // 3, 0] = OFFSET[0] + 3e9 * SCALE[0]
    dev, host, route = _write_both(icp, ctx, tmp_path, xyz, icp.LAS_CLI, SCALE, OFFSET, tag="_cli")
    assert route == 0 and dev == host
    dev, host, route = _write_both(icp, ctx, tmp_path, xyz, icp.LAS_CORE, tag="_core")
    assert route == 0 and dev == host
    ctx.set_source(xyz)
    p, q = tmp_path / "src.las", tmp_path / "src_host.las"
    ctx.write_source_las(p, icp.LAS_CLI, SCALE, OFFSET)
    icp.las_write_cli(q, xyz, SCALE, OFFSET)
    assert ctx.last_las_path() == 0 and p.read_bytes() == q.read_bytes()


def test_encode_rejects_bad_arguments(icp, ctx, tmp_path):
    xyz = np.zeros((4, 3))
    with ctx.to_device(xyz) as d:
        for args in ((d, 0, icp.LAS_CLI, SCALE, OFFSET), (d, 4, icp.LAS_CLI, None, OFFSET), (d, 4, 2, SCALE, OFFSET),
                     (None, 4, icp.LAS_CLI, SCALE, OFFSET), (xyz.ctypes.data, 4, icp.LAS_CLI, SCALE, OFFSET)):
            with pytest.raises(icp.IcpError) as e:
                ctx.write_las_device(tmp_path / "never.las", *args)
            assert e.value.code == icp.EINVAL
    assert not (tmp_path / "never.las").exists()
