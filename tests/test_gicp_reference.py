"""What the generalized-ICP GPU tests rely on, proved on the CPU (tests/gicp_reference.py): the
numpy mirror of the per-pair terms agrees with the definition, the exact case is exact in any order,
the numpy loop beats the point metric on the corner fixture and registers the partial overlap, and
the header's constants and the sums' layout are the binding's."""
import ctypes
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import gicp_reference as G
import plane_fixtures as pf
import reject_fixtures as rf

ROOT = Path(__file__).resolve().parents[1]


def _definition_sums(a, b, n0, nb, R, eps, origin):
    """A, g, sum_r2 from the textbook definition in numpy (any operation order)."""
    A, g, r2 = np.zeros((6, 6)), np.zeros(6), 0.0
    for i in range(len(a)):
        na = R @ n0[i]
        S = 2.0 * np.eye(3) - (1.0 - eps) * (np.outer(na, na) + np.outer(nb[i], nb[i]))
        M = np.linalg.inv(S)
        p = a[i] - origin
        X = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        J = np.concatenate([-X, np.eye(3)], axis=1)
        r = a[i] - b[i]
        A += J.T @ M @ J
        g += J.T @ M @ r
        r2 += r @ M @ r
    return A, g, r2


def test_terms_agree_with_the_definition():
    rng = np.random.default_rng(3)
    m = 200
    a, b = rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
    n0 = rng.normal(size=(m, 3))
    n0 /= np.linalg.norm(n0, axis=1, keepdims=True)
    nb = rng.normal(size=(m, 3))
    nb /= np.linalg.norm(nb, axis=1, keepdims=True)
    n0[::7] = 0.0
    nb[::11] = 0.0
    R = pf._rot(2, 25.0) @ pf._rot(0, -40.0)
    origin = np.array([0.3, -0.2, 0.1])
    for eps in (1e-3, 2.0 ** -20, 1.0):
        A, g, r2, absA, absg, absr2 = G.gicp_sums_numpy(a, b, n0, nb, R, eps, origin)
        wA, wg, wr2 = _definition_sums(a, b, n0, nb, R, eps, origin)
        assert np.array_equal(A, A.T)
        # the inverse's conditioning is 1 / epsilon
        tol = 1e-13 / eps
        assert (np.abs(A - wA) <= tol * absA).all() and (np.abs(g - wg) <= tol * absg).all()
        assert abs(r2 - wr2) <= tol * absr2
        assert (absA >= np.abs(A)).all() and absr2 == r2 > 0.0  # r^T M r is a positive form


def test_epsilon_one_is_the_isotropic_metric():
    rng = np.random.default_rng(4)
    a, b, n0, nb = (rng.normal(size=(50, 3)) for _ in range(4))
    n0 /= np.linalg.norm(n0, axis=1, keepdims=True)
    nb /= np.linalg.norm(nb, axis=1, keepdims=True)
    t = G.gicp_terms(a, b, n0, nb, np.eye(3), 0.0, np.zeros(3))
    assert (t[:, [15, 18, 20]] == 0.5).all() and (t[:, [16, 17, 19]] == 0.0).all()  # M = I / 2 exactly


@pytest.mark.parametrize("n_src", [63, 4097, 6000])
def test_exact_case_sums_are_exact_in_any_order(n_src):
    case = G.exact_gicp_case(n_src)
    nb = case["nrm"][case["j"]]
    assert np.array_equal(case["n0"].any(1), nb.any(1))
    assert np.array_equal(np.abs(case["n0"] @ case["R"].T), np.abs(nb))  # R n0 = +-nb
    assert (case["n0"] @ case["R"].T == -nb).any() and (case["n0"] @ case["R"].T == nb).any()
    det_R = np.linalg.det(case["R"])
    assert det_R == 1.0 and np.array_equal(case["R"] @ case["R"].T, np.eye(3))
    a, b = case["src"], case["tgt"][case["j"]]
    t = G.gicp_terms(a, b, case["n0"], nb, case["R"], 1.0 - case["epsilon"], case["origin"])
    # every term is a multiple of 2^-13, and the sum of all magnitudes stays far inside 53 bits: any
    # partial sum in any order is then an exactly representable multiple of 2^-13
    scaled = t * 8192.0
    assert (scaled == np.rint(scaled)).all()
    total = sum(int(v) for v in np.abs(scaled).sum(0).astype(np.int64))
    assert np.abs(scaled).max() < 2.0 ** 28 and total < 2 ** 45
    # M is dyadic: 32 along the shared normal, 1/2 across it, 1/2 I for an isotropic pair
    Mdiag = t[:, [15, 18, 20]]
    iso = ~nb.any(1)
    assert (Mdiag[iso] == 0.5).all() and (np.sort(Mdiag[~iso], axis=1) == [0.5, 0.5, 32.0]).all()
    assert (t[:, [16, 17, 19]] == 0.0).all()
    # the fp64 terms are the exact rational terms of the definition (a sample of the pairs)
    for i in np.random.default_rng(n_src).choice(n_src, min(n_src, 40), replace=False):
        want = G.exact_terms_fraction(case, int(i))
        assert [Fraction(float(v)) for v in t[i]] == want, i
    # numpy's pairwise sums and a sequential sum in a shuffled order: the same numbers
    everything = np.ones(n_src, bool)
    A, g, r2, n, iso_src, iso_tgt = G.exact_sums(case, everything)
    assert n == n_src and iso_src == iso_tgt == int(iso.sum())
    order = np.random.default_rng(n_src + 1).permutation(n_src)
    seq = np.zeros(28)
    for i in order[:600]:
        seq = seq + t[i]
    seq = seq + t[order[600:]].sum(0)
    As, gs, rs = G._unpack(seq)
    assert np.array_equal(As, A) and np.array_equal(gs, g) and rs == r2
    if n_src >= 4097:
        assert np.linalg.cond(A) < 1e5, np.linalg.cond(A)


@pytest.fixture(scope="module")
def corner_errors():
    """n -> (GICP after each of 5 iterations, point-to-point after each of 30)."""
    out = {}
    for n in (6000, 20000):
        tgt, src, T = pf.pair(n)
        out[n] = (G.numpy_gicp(tgt, src, T, 5), rf.numpy_icp(tgt, src, T, 30))
    return out


@pytest.mark.parametrize("n", [6000, 20000])
def test_numpy_gicp_beats_point_to_point(corner_errors, n):
    gicp, point = corner_errors[n]
    print(f"n={n}: GICP after 5 iterations {gicp[-1]:.3e}; point best of 30 {min(point):.3e}")
    assert gicp[-1] < min(point)


def test_numpy_gicp_registers_the_partial_overlap():
    tgt, src, T, _ = rf.overlap_pair()
    errs = G.numpy_gicp(tgt, src, T, 5, trim=0.5)
    print(f"overlap_pair, trim 0.5: GICP after 5 iterations {errs[-1]:.3e}")
    assert errs[-1] <= 1e-3


def test_symbols_constants_and_layout(icp):
    hip = (ROOT / "include" / "icp_hip.h").read_text()
    eng = (ROOT / "include" / "icp_engine.h").read_text()
    lib = ctypes.CDLL(str(icp.LIB_PATH))
    for name, text in (("icp_hip_estimate_source_normals", hip), ("icp_hip_set_source_normals", hip),
                       ("icp_hip_set_source_normals_device", hip), ("icp_hip_get_source_normals", hip),
                       ("icp_hip_get_source_normals_device", hip), ("icp_hip_gicp_sums", hip),
                       ("icp_hip_gicp_sums_at", hip), ("icp_gicp_solve", hip), ("icp_hip_set_gicp_epsilon", hip),
                       ("icp_session_last_gicp", eng)):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in icp._lib.SIGNATURES
    for k, name in enumerate(("POINT", "PLANE", "GICP")):
        assert re.search(r"#define\s+ICP_METRIC_" + name + r"\s+" + str(k) + r"\b", eng)
        assert getattr(icp, "METRIC_" + name) == k
    assert re.search(r"#define\s+ICP_RUN_OPTIONS_VERSION\s+1u?\b", eng) and ctypes.sizeof(icp.RunOptions) == 24
    body = re.search(r"typedef struct icp_gicp_sums \{(.*?)\} icp_gicp_sums;", hip, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", v).strip() for v in decl.split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in icp.GicpSums._fields_]
    S = icp.GicpSums
    assert ctypes.sizeof(S) == 400
    assert [getattr(S, f).offset for f in fields] == [0, 288, 336, 344, 352, 360, 368, 392]


def test_gicp_solve_is_the_plane_solve(icp):
    """icp_gicp_solve on A, g, n, origin: icp_plane_solve's bytes and refusals (host only)."""
    tgt, src, _ = pf.pair(600)
    a, b = src[:300], tgt[:300]
    nrm = np.zeros((300, 3))
    nrm[np.arange(300), np.arange(300) % 3] = 1.0
    origin = a.mean(0)
    A, g, r2 = G.gicp_sums_numpy(a, b, nrm, nrm, np.eye(3), 1e-3, origin)[:3]
    s = icp.GicpSums()
    s.A[:] = list(A.reshape(36))
    s.g[:] = list(g)
    s.sum_r2, s.n, s.epsilon = r2, 300, 1e-3
    s.origin[:] = list(origin)
    T, ok = icp.gicp_solve(s)
    Tp, okp = icp.plane_solve(pf.sums_struct(icp, A, g, r2, 300, origin))
    assert ok == okp == 1 and T.tobytes() == Tp.tobytes()
    assert np.abs(T - G.gicp_step(A, g, origin)).max() <= 1e-12
    s.n = 5
    T, ok = icp.gicp_solve(s)
    assert ok == 0 and np.isnan(T).all()
    s.n = 300
    s.A[0] = 0.0
    T, ok = icp.gicp_solve(s)
    assert ok == 0 and np.isnan(T).all()
