"""The CLI's --trim and --max-dist (icp_registration_main.cpp) on a LAS pair of the partial-overlap
fixture (1 mm grid): with --metric plane the trimmed rule registers where the reference's cull ends
worse than it started; the flags' usage errors; and without the flags nothing changes: the five files
of the commands the CLI had before are the same byte for byte whichever way they are asked for."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import reject_fixtures as rf

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "iterativeclosestpoint_amd" / "bin" / "icp_registration"
OUTPUTS = ["sampled_source.las", "sampled_target.las", "registered_source.las", "registered_target.las",
           "icp_transformation.txt"]


@pytest.fixture(scope="module")
def las_pair(icp, tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_pair")
    tgt, src, _, _ = rf.overlap_pair()
    icp.las_write_cli(d / "source.las", src)
    icp.las_write_cli(d / "target.las", tgt)
    return d


def _run(las_pair, outdir, flags, iters="20", tolerance="0"):
    return subprocess.run([str(EXE), "--source", str(las_pair / "source.las"), "--target", str(las_pair / "target.las"),
                           "--sample-rate", "1", "--max-iters", iters, "--tolerance", tolerance, "--outdir", str(outdir),
                           *flags], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def runs(las_pair, tmp_path_factory):
    """Each flag set run once: name -> (CompletedProcess, output directory)."""
    base = tmp_path_factory.mktemp("reject_runs")
    out = {}
    for name, flags in {"plain": [], "point": ["--metric", "point"], "plain_device_io": ["--device-io"],
                        "plane": ["--metric", "plane", "--normals-k", "12"],
                        "plane_trim": ["--metric", "plane", "--normals-k", "12", "--trim", "0.5"],
                        "plane_trim_device_io": ["--metric", "plane", "--normals-k", "12", "--trim", "0.5", "--device-io"],
                        "trim": ["--trim", "0.5"], "max_dist": ["--max-dist", "0.1"]}.items():
        d = base / name
        d.mkdir()
        out[name] = (_run(las_pair, d, flags), d)
    return out


def _last_cumulative(report: Path):
    """The last iteration's cumulative transform of icp_transformation.txt (10 significant digits)."""
    text = report.read_text(encoding="utf-8")
    blocks = text.split("--- ")
    assert len(blocks) > 2, text[:400]
    rows = re.findall(r"\[([^\]]*)\]", blocks[-1])[:4]
    T = np.eye(4)
    T[:3, :3] = np.array([[float(v) for v in row.split(",")] for row in rows[:3]])
    T[:3, 3] = [float(v) for v in rows[3].split(",")]
    return T


def test_every_run_exits_zero(runs):
    for name, (r, _) in runs.items():
        assert r.returncode == 0, name + r.stdout[-2000:] + r.stderr[-2000:]
    assert "rejector: trimmed" in runs["plane_trim"][0].stdout and "rejector" not in runs["plain"][0].stdout
    assert "rejector: pairs within" in runs["max_dist"][0].stdout


def test_trimmed_plane_registers_the_partial_overlap(runs):
    """--metric plane --trim 0.5 reaches at most 1e-3 (simulation on the rounded clouds: 6.8e-5); the
    same command without --trim is at least 1e-2 (8.5e-2)."""
    T_true = rf.overlap_pair()[2]
    err = {name: rf.t_rmse(_last_cumulative(runs[name][1] / "icp_transformation.txt"), T_true)
           for name in ("plane", "plane_trim", "plane_trim_device_io", "trim", "max_dist", "plain")}
    print("t_rmse of the last cumulative transform: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err["plane_trim"] <= 1e-3 and err["plane_trim_device_io"] <= 1e-3
    assert err["plane"] >= 1e-2


def test_device_io_writes_the_same_files(runs):
    for name in OUTPUTS:
        assert (runs["plane_trim_device_io"][1] / name).read_bytes() == (runs["plane_trim"][1] / name).read_bytes(), name


@pytest.mark.parametrize("flags", [["--trim", "0.5", "--max-dist", "0.1"], ["--max-dist", "0.1", "--trim", "0.5"],
                                   ["--trim", "0"], ["--trim", "1.5"], ["--trim", "nan"], ["--trim", "x"],
                                   ["--max-dist", "-1"], ["--max-dist", "0"], ["--max-dist", "inf"], ["--trim"],
                                   ["--trim", "0.5", "--devices", "0,0"], ["--max-dist", "0.1", "--devices", "0,0"]])
def test_usage_errors(las_pair, tmp_path, flags):
    r = _run(las_pair, tmp_path, flags)
    assert r.returncode == 2 and "usage" in r.stderr, flags
    assert not any(tmp_path.iterdir())


def test_no_flag_means_no_change(runs):
    """The commands of the CLI as it was (no flag, --metric point, --device-io) write the same five
    files; a rejector leaves the sampled clouds and the target as they are."""
    for name in OUTPUTS:
        plain = (runs["plain"][1] / name).read_bytes()
        assert len(plain) > 0
        assert (runs["point"][1] / name).read_bytes() == plain, name
        assert (runs["plain_device_io"][1] / name).read_bytes() == plain, name
        if name.startswith("sampled") or name == "registered_target.las":
            for other in ("trim", "max_dist", "plane_trim"):
                assert (runs[other][1] / name).read_bytes() == plain, (other, name)
    assert (runs["trim"][1] / "icp_transformation.txt").read_bytes() != (runs["plain"][1] / "icp_transformation.txt").read_bytes()
