"""References and fixtures of the generalized-ICP tests (a helper module, not a conftest): the numpy
mirror of gicp_pair_terms (gicp_kernels.hip) line for line, the sums with their terms' magnitudes, a
case whose every term is a small dyadic number (so every sum is exact in any order), and a numpy
loop with the engine's rules. tests/test_gicp_reference.py proves on the CPU what the GPU tests rely
on."""
import functools
from fractions import Fraction

import numpy as np

import plane_fixtures as pf
import plane_reference as PR
import reject_fixtures as rf

EXACT_EPS = 2.0 ** -6
# a signed permutation that is a rotation (a quarter turn about z): R n is exact for every n
EXACT_R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def gicp_terms(a, b, n0, nb, R, f, origin):
    """Per pair the 28 terms of gicp_pair_terms, (m, 28), in the kernel's operation order: every
    product is rounded before its add (numpy does not fuse). a, b, n0, nb: (m, 3); R (3, 3); f = 1 -
    epsilon; origin (3,)."""
    R = np.asarray(R, np.float64).reshape(9)
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
    n0x, n0y, n0z = n0[:, 0], n0[:, 1], n0[:, 2]
    nbx, nby, nbz = nb[:, 0], nb[:, 1], nb[:, 2]
    ox, oy, oz = (np.float64(v) for v in origin)
    f = np.float64(f)
    nax = (R[0] * n0x + R[1] * n0y) + R[2] * n0z
    nay = (R[3] * n0x + R[4] * n0y) + R[5] * n0z
    naz = (R[6] * n0x + R[7] * n0y) + R[8] * n0z
    s00 = 2.0 - f * (nax * nax + nbx * nbx)
    s11 = 2.0 - f * (nay * nay + nby * nby)
    s22 = 2.0 - f * (naz * naz + nbz * nbz)
    s01 = 0.0 - f * (nax * nay + nbx * nby)
    s02 = 0.0 - f * (nax * naz + nbx * nbz)
    s12 = 0.0 - f * (nay * naz + nby * nbz)
    c00 = s11 * s22 - s12 * s12
    c01 = s02 * s12 - s01 * s22
    c02 = s01 * s12 - s02 * s11
    c11 = s00 * s22 - s02 * s02
    c12 = s01 * s02 - s00 * s12
    c22 = s00 * s11 - s01 * s01
    det = (s00 * c00 + s01 * c01) + s02 * c02
    m00, m01, m02 = c00 / det, c01 / det, c02 / det
    m11, m12, m22 = c11 / det, c12 / det, c22 / det
    rx, ry, rz = ax - bx, ay - by, az - bz
    px, py, pz = ax - ox, ay - oy, az - oz
    yx = (m00 * rx + m01 * ry) + m02 * rz
    yy = (m01 * rx + m11 * ry) + m12 * rz
    yz = (m02 * rx + m12 * ry) + m22 * rz
    q00, q10, q20 = py * m02 - pz * m01, pz * m00 - px * m02, px * m01 - py * m00
    q01, q11, q21 = py * m12 - pz * m11, pz * m01 - px * m12, px * m11 - py * m01
    q02, q12, q22 = py * m22 - pz * m12, pz * m02 - px * m22, px * m12 - py * m02
    t = [
        py * q02 - pz * q01, pz * q00 - px * q02, px * q01 - py * q00, q00, q01, q02,
        pz * q10 - px * q12, px * q11 - py * q10, q10, q11, q12,
        px * q21 - py * q20, q20, q21, q22,
        m00, m01, m02, m11, m12, m22,
        py * yz - pz * yy, pz * yx - px * yz, px * yy - py * yx, yx, yy, yz,
        (rx * yx + ry * yy) + rz * yz,
    ]
    return np.stack([np.broadcast_to(v, ax.shape) for v in t], axis=1)


_UPPER = [(p, q) for p in range(6) for q in range(p, 6)]


def _unpack(v):
    """The 28 sums as (A (6, 6) symmetric, g (6,), sum_r2)."""
    A = np.zeros((6, 6))
    for m, (p, q) in enumerate(_UPPER):
        A[p, q] = A[q, p] = v[m]
    return A, np.array(v[21:27]), float(v[27])


def gicp_sums_numpy(a, b, n0, nb, R, epsilon, origin):
    """(A (6, 6), g (6,), sum_r2, and the sums of the terms' magnitudes absA, absg, absr2)."""
    t = gicp_terms(a, b, n0, nb, R, 1.0 - epsilon, origin)
    return _unpack(t.sum(0)) + _unpack(np.abs(t).sum(0))


def gicp_step(A, g, origin):
    """icp_gicp_solve in numpy: A x = -g, x = (w, t'), the Rodrigues rotation about the origin."""
    x = np.linalg.solve(A, -g)
    w, tp = x[:3], x[3:]
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Rm = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, origin + tp - Rm @ origin
    return T


def numpy_gicp(tgt, src, T_true, iterations, epsilon=1e-3, trim=None, k=16, sigma=3.0, nrm_tgt=None, nrm_src=None):
    """t_rmse of the cumulative transform after each iteration of the generalized-ICP loop with the
    engine's rules (reject_fixtures.numpy_icp's cull or trim): the normals of both clouds from k
    neighbours unless given, the source's in the frame of the start, R_src the rotation so far."""
    nearest = rf._nearest(tgt)
    nrm_tgt = rf._normals(tgt, k) if nrm_tgt is None else nrm_tgt
    nrm_src = rf._normals(np.asarray(src), k) if nrm_src is None else nrm_src
    cur, Tc, errs = np.array(src), np.eye(4), []
    for it in range(iterations):
        idx = nearest(cur)
        d = np.sqrt(((cur - tgt[idx]) ** 2).sum(1))
        if trim is None:
            mean, sd = d.mean(), d.std()
            thr = mean + (max(sigma * sd, 0.5 * mean) if it == 0 else sigma * sd)
        else:
            n = len(d)
            rank = max(min(3, n), min(n, int(trim * float(n))))
            thr = np.partition(d, rank - 1)[rank - 1]
        v = d <= thr
        a, b = cur[v], tgt[idx[v]]
        A, g = gicp_sums_numpy(a, b, nrm_src[v], nrm_tgt[idx[v]], Tc[:3, :3], epsilon, a.mean(0))[:2]
        T = gicp_step(A, g, a.mean(0))
        cur = cur @ T[:3, :3].T + T[:3, 3]
        Tc = T @ Tc
        errs.append(rf.t_rmse(Tc, T_true))
    return errs


# --- the exact case

@functools.lru_cache(maxsize=None)
def exact_gicp_case(n_src):
    """plane_reference.exact_plane_case(n_src) with one source normal per source row: R^T (+-nb) of
    its own match for R = EXACT_R (zero where nb is zero), so that R n0 = +-nb and S = C_a + C_b is
    diag(2 eps, 2, 2) up to the axis, or 2 I: with epsilon = 2^-6 M is dyadic (32 and 1/2) and every
    term a multiple of 2^-13 below 2^14. Shared: read only."""
    case = dict(PR.exact_plane_case(n_src))
    rng = np.random.default_rng(5000 + n_src)
    nb = case["nrm"][case["j"]]
    sign = rng.choice([-1.0, 1.0], n_src)[:, None]
    n0 = (sign * nb) @ EXACT_R  # rows R^T (+-nb)
    n0 = n0 + 0.0               # no negative zeros: the rows compare equal to what a context returns
    n0.setflags(write=False)
    case["n0"] = n0
    case["R"] = EXACT_R
    case["epsilon"] = EXACT_EPS
    return case


def exact_sums(case, use):
    """(A, g, sum_r2, n, n_iso_src, n_iso_tgt) of the case's pairs selected by the mask `use`, as the
    kernel defines them; exact whatever the order (tests/test_gicp_reference.py)."""
    a, b = case["src"][use], case["tgt"][case["j"][use]]
    n0, nb = case["n0"][use], case["nrm"][case["j"][use]]
    A, g, r2 = gicp_sums_numpy(a, b, n0, nb, case["R"], case["epsilon"], case["origin"])[:3]
    return A, g, r2, int(use.sum()), int((~n0.any(1)).sum()), int((~nb.any(1)).sum())


def exact_terms_fraction(case, i):
    """The 28 terms of pair i of the case in exact rational arithmetic, from the definition (not
    the kernel's order): S = C_a + C_b, M = S^-1 by Cramer's rule, J = [-[a']x | I]."""
    F = lambda v: Fraction(float(v))
    a = [F(v) for v in case["src"][i]]
    b = [F(v) for v in case["tgt"][case["j"][i]]]
    n0 = [F(v) for v in case["n0"][i]]
    nb = [F(v) for v in case["nrm"][case["j"][i]]]
    R = [[F(v) for v in row] for row in case["R"]]
    o = [F(v) for v in case["origin"]]
    f = 1 - F(case["epsilon"])
    na = [sum(R[p][q] * n0[q] for q in range(3)) for p in range(3)]
    S = [[(2 if p == q else 0) - f * (na[p] * na[q] + nb[p] * nb[q]) for q in range(3)] for p in range(3)]
    det = (S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) - S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0])
           + S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0]))
    cof = lambda p, q: (S[(p + 1) % 3][(q + 1) % 3] * S[(p + 2) % 3][(q + 2) % 3]
                        - S[(p + 1) % 3][(q + 2) % 3] * S[(p + 2) % 3][(q + 1) % 3])
    M = [[cof(q, p) / det for q in range(3)] for p in range(3)]
    r = [a[k] - b[k] for k in range(3)]
    p_ = [a[k] - o[k] for k in range(3)]
    X = [[0, -p_[2], p_[1]], [p_[2], 0, -p_[0]], [-p_[1], p_[0], 0]]  # [a']x
    J = [[-X[k][c] for c in range(3)] + [1 if c == k else 0 for c in range(3)] for k in range(3)]  # 3 x 6
    MJ = [[sum(M[k][l] * J[l][c] for l in range(3)) for c in range(6)] for k in range(3)]
    A = [[sum(J[k][p] * MJ[k][q] for k in range(3)) for q in range(6)] for p in range(6)]
    y = [sum(M[k][l] * r[l] for l in range(3)) for k in range(3)]
    g = [sum(J[k][p] * y[k] for k in range(3)) for p in range(6)]
    return [A[p][q] for p, q in _UPPER] + g + [sum(r[k] * y[k] for k in range(3))]
