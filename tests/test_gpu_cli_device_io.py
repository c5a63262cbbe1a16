"""The CLI's --device-io mode (icp_registration_main.cpp): both clouds resident on the GPU from
file to file, LAS records decoded, sampled and encoded by kernels. Its five output files are the
default flow's byte for byte; with more than one device it is a usage error."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "iterativeclosestpoint_amd" / "bin" / "icp_registration"
OUTPUTS = ["sampled_source.las", "sampled_target.las", "registered_source.las", "registered_target.las",
           "icp_transformation.txt"]


@pytest.fixture(scope="module")
def las_pair(icp, tmp_path_factory):
    d = tmp_path_factory.mktemp("device_io_pair")
    tgt, src, _ = icp.synth_pair(20000, yaw_deg=3.0)
    # a georeferenced-looking scale / offset: the sampled and registered files all carry the source's
    icp.las_write_cli(d / "source.las", src, (0.001, 0.001, 0.0005), (-3.0, 2.0, 0.5))
    icp.las_write_cli(d / "target.las", tgt, (0.002, 0.001, 0.001), (0.0, 0.0, 0.0))
    return d


def _run(las_pair, outdir, *flags):
    outdir.mkdir()
    return subprocess.run([str(EXE), "--source", str(las_pair / "source.las"), "--target", str(las_pair / "target.las"),
                           "--sample-rate", "3", "--outdir", str(outdir), *flags],
                          capture_output=True, text=True, timeout=120)


def test_device_io_writes_the_default_flows_files(las_pair, tmp_path):
    plain = _run(las_pair, tmp_path / "plain")
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    dev = _run(las_pair, tmp_path / "device_io", "--device-io")
    assert dev.returncode == 0, dev.stdout[-2000:] + dev.stderr[-2000:]
    for name in OUTPUTS:
        a, b = (tmp_path / "plain" / name).read_bytes(), (tmp_path / "device_io" / name).read_bytes()
        assert len(a) > 0 and a == b, name
    assert len((tmp_path / "plain" / "sampled_source.las").read_bytes()) == 227 + 20 * 6667


def test_device_io_rejects_a_device_group(las_pair, tmp_path):
    r = _run(las_pair, tmp_path / "group", "--device-io", "--devices", "0,0")
    assert r.returncode == 2 and "usage" in r.stderr
    assert not any((tmp_path / "group").iterdir())
