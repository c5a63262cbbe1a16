"""The CLI's --metric gicp and --gicp-epsilon (icp_registration_main.cpp) on a LAS pair of the
partial-overlap fixture on its 1 mm grid: with --trim 0.5 it registers the pair, in the default flow
and the --device-io flow, which write the same files; the flags' usage errors; and without the flag
nothing changes: the commands the CLI had before write the same five files whichever way they are
asked for."""
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
    d = tmp_path_factory.mktemp("gicp_pair")
    tgt, src, _, _ = rf.overlap_pair(grid=1e-3)
    icp.las_write_cli(d / "source.las", src)
    icp.las_write_cli(d / "target.las", tgt)
    return d


def _run(las_pair, outdir, flags):
    return subprocess.run([str(EXE), "--source", str(las_pair / "source.las"), "--target", str(las_pair / "target.las"),
                           "--sample-rate", "1", "--max-iters", "20", "--tolerance", "0", "--outdir", str(outdir),
                           *flags], capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def runs(las_pair, tmp_path_factory):
    """Each flag set run once: name -> (CompletedProcess, output directory)."""
    base = tmp_path_factory.mktemp("gicp_runs")
    out = {}
    for name, flags in {"plain": [], "plain_reordered": ["--normals-k", "12", "--metric", "point"],
                        "gicp_trim": ["--metric", "gicp", "--trim", "0.5"],
                        "gicp_trim_device_io": ["--device-io", "--trim", "0.5", "--metric", "gicp"],
                        "gicp_trim_eps": ["--metric", "gicp", "--trim", "0.5", "--gicp-epsilon", "0.0625"]}.items():
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
    assert "generalized ICP, epsilon 0.001" in runs["gicp_trim"][0].stdout
    assert "generalized ICP, epsilon 0.0625" in runs["gicp_trim_eps"][0].stdout
    assert "generalized ICP" not in runs["plain"][0].stdout


def test_trimmed_gicp_registers_the_partial_overlap(runs):
    """--metric gicp --trim 0.5, 20 iterations, ends at or below 1e-3 (the numpy loop on the rounded
    clouds: 1.4e-4)."""
    T_true = rf.overlap_pair()[2]
    err = {name: rf.t_rmse(_last_cumulative(runs[name][1] / "icp_transformation.txt"), T_true)
           for name in ("gicp_trim", "gicp_trim_device_io", "gicp_trim_eps", "plain")}
    print("t_rmse of the last cumulative transform: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err["gicp_trim"] <= 1e-3 and err["gicp_trim_device_io"] <= 1e-3


def test_device_io_writes_the_same_files(runs):
    for name in OUTPUTS:
        assert (runs["gicp_trim_device_io"][1] / name).read_bytes() == (runs["gicp_trim"][1] / name).read_bytes(), name
    # another epsilon is another registration
    assert (runs["gicp_trim_eps"][1] / "icp_transformation.txt").read_bytes() != \
        (runs["gicp_trim"][1] / "icp_transformation.txt").read_bytes()


def test_no_flag_means_no_change(runs):
    for name in OUTPUTS:
        plain = (runs["plain"][1] / name).read_bytes()
        assert len(plain) > 0
        assert (runs["plain_reordered"][1] / name).read_bytes() == plain, name
        if name.startswith("sampled") or name == "registered_target.las":
            assert (runs["gicp_trim"][1] / name).read_bytes() == plain, name  # the inputs are the inputs


@pytest.mark.parametrize("flags", [["--metric", "gicp", "--gicp-epsilon", "0"], ["--metric", "gicp", "--gicp-epsilon", "1.5"],
                                   ["--gicp-epsilon", "nan"], ["--gicp-epsilon", "x"], ["--gicp-epsilon", "1e-7"],
                                   ["--gicp-epsilon"], ["--metric", "gicp", "--normals-k", "2"],
                                   ["--metric", "gicp", "--devices", "0,0"], ["--metric", "gicpx"]])
def test_usage_errors(las_pair, tmp_path, flags):
    r = _run(las_pair, tmp_path, flags)
    assert r.returncode == 2, flags
    assert "usage" in r.stderr or "--normals-k" in r.stderr, flags
    if "--gicp-epsilon" in flags and len(flags) > 1:
        assert "--gicp-epsilon must be" in r.stderr
    if "--devices" in flags:
        assert "--metric gicp runs on one GPU" in r.stderr
    assert not any(tmp_path.iterdir())
