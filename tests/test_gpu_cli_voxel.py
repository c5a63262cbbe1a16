"""The CLI's --voxel (icp_registration_main.cpp) on a LAS pair of the corner fixture: the default flow
and the --device-io flow write the same files byte for byte, the sampled files hold as many points
as the model finds voxels in the decoded clouds, a bad edge is a usage error, and the option
composes with --metric plane."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import plane_fixtures as pf
import voxel_reference as vr

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "iterativeclosestpoint_amd" / "bin" / "icp_registration"
OUTPUTS = ["sampled_source.las", "sampled_target.las", "registered_source.las", "registered_target.las",
           "icp_transformation.txt"]
N = 6000
VOXEL = 0.1


@pytest.fixture(scope="module")
def las_pair(icp, tmp_path_factory):
    d = tmp_path_factory.mktemp("voxel_pair")
    tgt, src, _ = pf.pair(N)
    icp.las_write_cli(d / "source.las", src)
    icp.las_write_cli(d / "target.las", tgt)
    return d


def _run(las_pair, outdir, *flags):
    outdir.mkdir()
    return subprocess.run([str(EXE), "--source", str(las_pair / "source.las"), "--target", str(las_pair / "target.las"),
                           "--max-iters", "20", "--outdir", str(outdir), *flags],
                          capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def runs(las_pair, tmp_path_factory):
    base = tmp_path_factory.mktemp("voxel_runs")
    return {name: (_run(las_pair, base / name, "--voxel", str(VOXEL), *flags), base / name)
            for name, flags in {"host": [], "device_io": ["--device-io"], "plane": ["--metric", "plane"]}.items()}


def test_both_flows_write_the_same_files(runs):
    for name in ("host", "device_io"):
        r = runs[name][0]
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
        assert "voxel grid (0.1 m)" in r.stdout
    for name in OUTPUTS:
        a, b = (runs["host"][1] / name).read_bytes(), (runs["device_io"][1] / name).read_bytes()
        assert len(a) > 0 and a == b, name


def test_sampled_files_hold_the_models_voxels(icp, las_pair, runs):
    assert runs["host"][0].returncode == 0
    for which in ("source", "target"):
        xyz, _ = icp.las_read(las_pair / f"{which}.las")  # the stride is 1 when only --voxel is given
        assert len(xyz) == N
        m = len(np.unique(vr.keys_of(xyz, VOXEL, xyz.min(0))))
        got, _ = icp.las_read(runs["host"][1] / f"sampled_{which}.las")
        assert len(got) == m and 0 < m < N
        assert f"{which}: {N} -> {m} points" in runs["host"][0].stdout


@pytest.mark.parametrize("edge", ["0", "nan", "-1", "inf", "0.1x"])
def test_bad_edge_is_a_usage_error(las_pair, tmp_path, edge):
    r = _run(las_pair, tmp_path / "out", "--voxel", edge)
    assert r.returncode == 2 and "usage" in r.stderr
    assert not any((tmp_path / "out").iterdir())


def test_composes_with_the_plane_metric(runs):
    r, d = runs["plane"]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "point-to-plane" in r.stdout and "voxel grid" in r.stdout
    for name in OUTPUTS:
        assert (d / name).stat().st_size > 0
    for name in ("sampled_source.las", "sampled_target.las"):  # the same voxel clouds go in
        assert (d / name).read_bytes() == (runs["host"][1] / name).read_bytes()
