"""What the plane path's exact GPU tests rely on, proved on the CPU (tests/plane_reference.py): the
exact plane-sums case is exact and its nearest neighbours unique, the clusters are their own
neighbourhoods and lie on their side of the normals' rank rule under the model, the model agrees
with eigh where the eigenvector is well conditioned, and the k-NN block tiers of the shapes the GPU
tests use follow from knn_block_threads' formula."""
from pathlib import Path

import numpy as np
import pytest

import plane_fixtures as pf
import plane_reference as R

EXACT_N = [1, 2, 5, 6, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 16385]
CLUSTER_K = [3, 8, 32]
CLUSTER_WHERE = ["origin", "geo", "far"]
CLUSTER_SPREAD = [1.0, 0.01]


def _int_sums(case, take):
    """The sums in int64: J and r in units of 1/64."""
    a, b, nr = case["src"][take], case["tgt"][case["j"][take]], case["nrm"][case["j"][take]]
    J, r = pf.plane_terms(a, b, nr, case["origin"])
    J64, r64 = J * 64.0, r * 64.0
    assert (J64 == np.rint(J64)).all() and (r64 == np.rint(r64)).all()
    J64, r64 = J64.astype(np.int64), r64.astype(np.int64)
    return J64.T @ J64, J64.T @ r64, int((r64 * r64).sum())


@pytest.mark.parametrize("n_src", EXACT_N)
def test_exact_case_sums_are_exact_in_any_order(n_src):
    case = R.exact_plane_case(n_src)
    everything = np.ones(n_src, bool)
    A, g, r2, n, skipped = R.exact_sums(case, everything)
    take = case["nrm"][case["j"]].any(1)
    Ai, gi, r2i = _int_sums(case, take)
    assert n == take.sum() and skipped == n_src - n
    assert np.abs(Ai).max() < 2 ** 40 and abs(r2i) < 2 ** 40  # far inside fp64's 53 bits
    assert np.array_equal(A * 4096.0, Ai) and np.array_equal(g * 4096.0, gi) and r2 * 4096.0 == r2i
    # the numpy sums (pairwise) and a plain sequential sum in a shuffled order: the same numbers
    rng = np.random.default_rng(n_src)
    order = rng.permutation(np.flatnonzero(take))
    J, r = pf.plane_terms(case["src"][order], case["tgt"][case["j"][order]], case["nrm"][case["j"][order]],
                          case["origin"])
    As, gs, rs = np.zeros((6, 6)), np.zeros(6), 0.0
    for i in range(min(len(order), 600)):  # sequential over a prefix, the rest pairwise: another order again
        As, gs, rs = As + np.outer(J[i], J[i]), gs + J[i] * r[i], rs + r[i] * r[i]
    As = As + (J[600:, :, None] * J[600:, None, :]).sum(0)
    gs = gs + (J[600:] * r[600:, None]).sum(0)
    rs = rs + (r[600:] * r[600:]).sum()
    assert np.array_equal(As, A) and np.array_equal(gs, g) and rs == r2
    if n_src >= 65:
        assert np.linalg.cond(A) < 200.0, np.linalg.cond(A)


@pytest.mark.parametrize("n_src", [1, 257, 8193])
def test_exact_case_nearest_neighbours_are_unique(n_src):
    case = R.exact_plane_case(n_src)
    assert len(np.unique(case["tgt"], axis=0)) == 4096
    assert int(np.count_nonzero(~case["nrm"].any(1))) == 200
    off = case["src"] - case["tgt"][case["j"]]
    assert (off * 64.0 == np.rint(off * 64.0)).all() and np.abs(off).max() <= 0.25
    assert (off[::5] == 0.0).all()
    for lo in range(0, n_src, 512):
        D = pf.d2_rows(case["src"][lo:lo + 512], case["tgt"])
        assert np.array_equal(D.argmin(1), case["j"][lo:lo + 512])
        assert ((D == D.min(1, keepdims=True)).sum(1) == 1).all()


def _clusters(kind, k, where, spread):
    return (R.line_clusters if kind == "line" else R.strip_clusters)(k, where, spread)[0]


@pytest.mark.parametrize("spread", CLUSTER_SPREAD)
@pytest.mark.parametrize("where", CLUSTER_WHERE)
@pytest.mark.parametrize("k", CLUSTER_K)
def test_clusters_are_their_own_neighbourhoods_and_keep_their_side_of_the_rule(icp, k, where, spread):
    for kind in ("line", "strip"):
        tgt = _clusters(kind, k, where, spread)
        assert tgt.shape == (24 * k, 3) and len(np.unique(tgt, axis=0)) == 24 * k
        cen = tgt.reshape(24, k, 3).mean(1)
        gaps = np.linalg.norm(cen[:, None] - cen[None], axis=2)[~np.eye(24, dtype=bool)]
        assert gaps.min() >= 100.0 * spread
        assert np.linalg.norm(tgt.reshape(24, k, 3) - cen[:, None], axis=2).max() <= 0.75 * spread
        idx, _ = pf.knn_brute(tgt, tgt, k)
        assert np.array_equal(np.sort(idx, 1), (np.arange(24 * k) // k * k)[:, None] + np.arange(k))
        nrm, S = R.normals_model(tgt, idx, None, icp, with_s=True)
        assert (S[:, 0] > 0.0).all()
        ratio = S[:, 1] / S[:, 0]
        print(f"{kind} k={k} {where} spread={spread}: log2 S1/S0 in [{np.log2(ratio.min() + 1e-300):.1f}, "
              f"{np.log2(ratio.max() + 1e-300):.1f}], nonzero {np.count_nonzero(ratio)}")
        if kind == "line":
            assert (S[:, 1] <= 2.0 ** -29 * S[:, 0]).all()  # eight times below the rule
            assert (nrm == 0.0).all()
            # a rule of S[1] > 0 would take most of the random-direction lines for planes
            assert np.count_nonzero(S[12 * k:, 1] > 0.0) >= 0.9 * 12 * k
        else:
            assert (S[:, 1] >= 2.0 ** -22 * S[:, 0]).all()  # sixteen times above it
            assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-15


@pytest.mark.parametrize("view", [None, (2.0, 2.0, 2.0)], ids=["no_viewpoint", "viewpoint"])
@pytest.mark.parametrize("k", [8, 16])
def test_model_matches_eigh_on_the_corner(icp, k, view):
    tgt = pf.corner(600, 11)
    idx, _ = pf.knn_brute(tgt, tgt, k)
    view = None if view is None else np.array(view)
    nrm = R.normals_model(tgt, idx, view, icp)
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-14
    p = tgt[idx]
    d = p - p.mean(1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", d, d))
    good = w[:, 0] / w[:, 1] <= 0.1
    assert good.mean() >= 0.8
    ref = v[:, :, 0]
    angle = np.arctan2(np.linalg.norm(np.cross(nrm[good], ref[good]), axis=1),
                       np.abs(np.einsum("ni,ni->n", nrm[good], ref[good])))
    assert angle.max() <= 1e-9, angle.max()
    if view is None:
        assert (nrm[np.arange(600), np.abs(nrm).argmax(1)] > 0).all()
    else:
        assert (np.einsum("ni,ni->n", nrm, view - tgt) >= 0).all()


def test_tie_plane_under_the_model(icp):
    tgt, view = R.tie_plane()
    idx, _ = pf.knn_brute(tgt, tgt, 8)
    nrm = R.normals_model(tgt, idx, None, icp)
    assert (nrm[:, 0] == -nrm[:, 1]).all() and (nrm[:, 2] == 0.0).all()  # an exact tie of |nx| and |ny|
    assert (nrm[:, 0] > 0.0).all() and np.abs(nrm[:, 0] - np.sqrt(0.5)).max() <= 2.0 ** -52
    seen = R.normals_model(tgt, idx, view, icp)
    assert (np.abs(seen) == np.abs(nrm)).all()
    assert ((seen[:, 0] * (view[0] - tgt[:, 0]) + seen[:, 1] * (view[1] - tgt[:, 1])) + seen[:, 2] * (view[2] - tgt[:, 2]) == 0.0).all()


TIERS = [  # (levels, k, bytes per thread, block threads): the shapes of tests/test_gpu_knn_shapes.py
    (20, 8, 256, 256), (20, 9, 268, 128), (40, 16, 512, 128), (40, 17, 524, 64),
    (20, 32, 544, 64), (40, 32, 704, 64), (60, 32, 864, 64), (61, 32, 872, 64)]


@pytest.mark.parametrize("levels,k,per,bs", TIERS)
def test_tier_table(levels, k, per, bs):
    assert R.knn_tier(levels, k) == (per, bs)
    assert per * bs <= 65536
    if bs < 256:
        assert per * 2 * bs > 65536  # the next larger block would not fit
    # the two exact edges fill the 64 KiB to the byte
    if (levels, k) in ((20, 8), (40, 16)):
        assert per * bs == 65536


def test_tier_formula_is_the_launcher_s(icp):
    """knn_tier restates knn_block_threads; the text of the launcher is checked for the three
    comparisons so that a change there is met by a change here."""
    src = (Path(icp.__file__).parent / "csrc" / "knn_kernels.hip").read_text()
    assert "(size_t)levels * 8 + (size_t)k * 12" in src
    assert "per * 256 <= 65536" in src and "per * 128 <= 65536" in src
