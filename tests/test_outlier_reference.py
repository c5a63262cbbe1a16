"""The numpy statement of the outlier filters (tests/outlier_reference.py) on hand-computed cases, the
conditions of the fixture cloud that tests/test_gpu_outlier.py leans on, and the new symbols and the
stats struct's layout against the header (no GPU)."""
import ctypes
import re
from fractions import Fraction
from pathlib import Path

import numpy as np

import outlier_reference as orf

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "icp_hip.h"


def _line(xs):
    p = np.zeros((len(xs), 3))
    p[:, 0] = xs
    return p


def test_four_points_written_out():
    """x = 0, 1, 3, 7 on a line, k = 2: the scores are (1+3)/2, (1+2)/2, (2+3)/2, (4+6)/2."""
    p = _line([0.0, 1.0, 3.0, 7.0])
    idx, d2 = orf.neighbours(p, 2)
    assert idx.tolist() == [[1, 2], [0, 2], [1, 0], [2, 1]]
    assert d2.tolist() == [[1.0, 9.0], [1.0, 4.0], [4.0, 9.0], [16.0, 36.0]]
    ref = orf.reference(p, orf.STATISTICAL, 2, 1.0)
    assert ref["score"].tolist() == [2.0, 1.5, 2.5, 5.0]
    assert ref["mean"] == Fraction(11, 4) and ref["var"] == Fraction(29, 16)
    assert abs(ref["threshold"] - (2.75 + 1.8125 ** 0.5)) < 1e-15
    assert ref["kept"].tolist() == [True, True, True, False]
    # std_ratio 0: the threshold is the mean; a negative ratio is allowed
    assert orf.reference(p, orf.STATISTICAL, 2, 0.0)["kept"].tolist() == [True, True, True, False]
    assert orf.reference(p, orf.STATISTICAL, 2, -0.5)["kept"].tolist() == [True, True, False, False]  # 2.75 - 0.673


def test_ties_go_to_the_lower_index_and_self_is_excluded_by_index():
    p = _line([0.0, 1.0, 2.0])
    idx, d2 = orf.neighbours(p, 1)
    assert idx[:, 0].tolist() == [1, 0, 1] and d2[:, 0].tolist() == [1.0, 1.0, 1.0]
    idx, _ = orf.neighbours(p, 2)  # k = n - 1: every other point
    assert idx.tolist() == [[1, 2], [0, 2], [1, 0]]


def test_a_row_of_copies():
    """Five copies among three other points: each copy's four nearest are the other copies, at 0;
    the copies' own indices never appear in their rows."""
    p = _line([5.0, 1.0, 5.0, 5.0, 9.0, 5.0, 5.0, 2.0])
    copies = [0, 2, 3, 5, 6]
    idx, d2 = orf.neighbours(p, 4)
    for i in copies:
        assert idx[i].tolist() == [j for j in copies if j != i] and (d2[i] == 0.0).all()
    s = orf.knn_scores(p, 4)
    assert (s[copies] == 0.0).all() and (s[[1, 4, 7]] > 0.0).all()
    c = orf.radius_scores(p, 0.5, 4)
    assert c.tolist() == [4.0, 0.0, 4.0, 4.0, 0.0, 4.0, 4.0, 0.0]


def test_lattice_radius_is_inclusive():
    p, interior = orf.lattice8()
    assert interior.sum() == 216
    ref = orf.reference(p, orf.RADIUS, 6, 1.0)
    assert np.array_equal(ref["kept"], interior)  # six neighbours at exactly d2 == r2
    assert set(ref["score"][~interior].tolist()) == {3.0, 4.0, 5.0}
    none = orf.reference(p, orf.RADIUS, 6, np.nextafter(1.0, 0.0))
    assert not none["kept"].any() and (none["score"] == 0.0).all()
    sat = orf.radius_scores(p, 1.0, 4)  # saturation
    assert sat.max() == 4.0 and (sat[interior] == 4.0).all()
    # statistical at k = 6: the interior's score is exactly 1.0
    s = orf.knn_scores(p, 6)
    assert (s[interior] == 1.0).all() and (s[~interior] > 1.0).all()


def _shares(kept, injected):
    return float((~kept[injected]).mean()), float((~kept[~injected]).mean())


def test_fixture_statistical_k8():
    cloud, injected = orf.fixture_cloud()
    assert cloud.shape == (6150, 3) and injected.sum() == 150
    ref = orf.fixture_reference(orf.STATISTICAL, 8, 1.0)
    d_inj, d_surf = _shares(ref["kept"], injected)
    print(f"\n[fixture k=8 ratio=1] threshold {ref['threshold']:.6f} kept {int(ref['kept'].sum())} "
          f"injected dropped {d_inj:.4f} surface dropped {d_surf:.5f} gap {ref['gap']:.3e}")
    assert abs(ref["threshold"] - 0.2120) < 5e-4
    assert d_inj >= 0.85 and d_surf <= 0.01
    assert ref["gap"] >= 1e-6
    # np.mean / np.std agree with the reference's moments far inside the gap
    s = ref["score"]
    assert abs(s.mean() + s.std() - ref["threshold"]) <= 1e-12


def test_fixture_statistical_k16():
    _, injected = orf.fixture_cloud()
    ref = orf.fixture_reference(orf.STATISTICAL, 16, 2.0)
    d_inj, d_surf = _shares(ref["kept"], injected)
    print(f"\n[fixture k=16 ratio=2] threshold {ref['threshold']:.6f} kept {int(ref['kept'].sum())} "
          f"injected dropped {d_inj:.4f} surface dropped {d_surf:.5f} gap {ref['gap']:.3e}")
    assert d_surf <= 0.01  # (a ratio of 2 keeps more of the strays: the 85 % belong to ratio 1)
    assert ref["gap"] >= 1e-6


def test_fixture_radius():
    _, injected = orf.fixture_cloud()
    ref = orf.fixture_reference(orf.RADIUS, 4, 0.15)
    d_inj, d_surf = _shares(ref["kept"], injected)
    print(f"\n[fixture radius 0.15 min 4] kept {int(ref['kept'].sum())} injected dropped {d_inj:.4f} "
          f"surface dropped {d_surf:.5f}")
    assert d_inj >= 0.85 and d_surf <= 0.05
    assert set(np.unique(ref["score"]).tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0}


def test_stats_bounds_hold_for_plain_float_sums():
    """The bounds contain what a plain fp64 evaluation of the device's formula gives (a sanity
    check of the bounds' form; the device's tree is checked on the GPU)."""
    s = orf.fixture_reference(orf.STATISTICAL, 8, 1.0)["score"]
    c = s[0]
    d = s - c
    m1 = d.sum() / len(s)
    var = (d * d).sum() / len(s) - m1 * m1
    mean, vref = orf.sr.moments_ref(s)
    b_mean, b_var = orf.stats_bounds(s)
    assert abs(Fraction(float(c + m1)) - mean) <= b_mean
    assert abs(Fraction(float(np.sqrt(var))) ** 2 - vref) <= b_var


# ---- the C ABI

def _header():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_symbols_and_constants(icp):
    text = _header()
    lib = ctypes.CDLL(str(icp.LIB_PATH))
    for name in ("icp_hip_outlier_filter", "icp_hip_outlier_filter_device", "icp_hip_outlier_last_timing"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in icp._lib.SIGNATURES
    assert re.search(r"#define\s+ICP_OUTLIER_STATISTICAL\s+0\b", text) and icp.OUTLIER_STATISTICAL == 0
    assert re.search(r"#define\s+ICP_OUTLIER_RADIUS\s+1\b", text) and icp.OUTLIER_RADIUS == 1
    assert (orf.STATISTICAL, orf.RADIUS) == (icp.OUTLIER_STATISTICAL, icp.OUTLIER_RADIUS)
    for name in ("outlier_filter", "OutlierStats"):
        assert hasattr(icp, name)
    for name in ("outlier_filter", "outlier_filter_device", "outlier_last_timing"):
        assert hasattr(icp.Context, name)
    # the config struct and its version are as they were
    assert icp.config().config_version == 3


def test_stats_struct_layout(icp):
    m = re.search(r"typedef\s+struct\s+icp_outlier_stats\s*\{(.*?)\}\s*icp_outlier_stats\s*;", _header(), re.S)
    assert m
    fields = [tuple(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == [("int64_t", "n"), ("int64_t", "kept"), ("double", "mean"), ("double", "std"),
                      ("double", "threshold")]
    ctype = {"int64_t": ctypes.c_int64, "double": ctypes.c_double}
    assert [(n, t) for n, t in icp.OutlierStats._fields_] == [(n, ctype[t]) for t, n in fields]
    assert ctypes.sizeof(icp.OutlierStats) == 40
    assert [getattr(icp.OutlierStats, n).offset for _, n in fields] == [0, 8, 16, 24, 32]


def test_argument_errors_need_no_device(icp):
    """A null context or m_out is refused before anything else."""
    L = icp.lib()
    m = ctypes.c_int64(7)
    xyz = np.zeros((4, 3))
    assert L.icp_hip_outlier_filter(None, xyz.ctypes.data_as(ctypes.c_void_p), 4, 0, 1, 1.0, 4, None, None, None,
                                    ctypes.byref(m), None) == icp.EINVAL
    assert L.icp_hip_outlier_last_timing(None, None) == icp.EINVAL
