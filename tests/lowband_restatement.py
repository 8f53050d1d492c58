"""CPU restatement (numpy, fp32) of the low-band spectral basis of csrc/lowband.hip: Chebyshev-filtered block subspace
iteration on the kNN Gaussian graph Laplacian, orthonormalised through the Gram matrix's own eigendecomposition (twice),
Rayleigh-Ritz, with a parallel cyclic Jacobi solver for the m x m problems. The schedule and every constant are read from
``ops.LOWBAND_DEFAULTS``; the launch sequence of ``pc3d_lowband_basis_f32`` is the sequence of calls in ``lowband_basis``.
The restatement follows the kernels' arithmetic (fp32 blocks, fp64 accumulation of the projected matrices, the same start
block, the same floors), not their summation order: it is a model of the method's accuracy, not a bit oracle."""
import os

import numpy as np

f32 = np.float32


def laplacian(pc, k=30):
    """pc [N,3] -> dense fp32 L = D - A of the symmetrised kNN-k Gaussian graph (TAOF_attack.py:31-52; self included in
    the k nearest, self-loops cancel)."""
    pc = np.asarray(pc, f32)
    n = pc.shape[0]
    d2 = ((pc[:, None, :] - pc[None, :, :]) ** 2).sum(-1).astype(f32)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :min(k, n)]
    mask = np.zeros((n, n), bool)
    mask[np.arange(n)[:, None], idx] = True
    mask |= mask.T
    np.fill_diagonal(mask, False)
    A = np.where(mask, np.exp(-d2), 0).astype(f32)
    return (np.diag(A.sum(1)) - A).astype(f32)


def block_size(n, lp, d):
    guard = max(int(d["guard_min"]), -(-lp // int(d["guard_div"])))
    return min(n, lp + guard)


def hash_unit(row, col, salt):
    """The counter-based start block: a murmur3 finaliser of (row, column, salt) -> [-1, 1). No cloud index: a cloud's
    basis does not depend on its place in the batch."""
    with np.errstate(over="ignore"):
        h = (np.asarray(row, np.uint32) * np.uint32(0x9E3779B1)) ^ (np.asarray(col, np.uint32) * np.uint32(0x85EBCA77)) \
            ^ (np.uint32(salt) * np.uint32(0xC2B2AE3D))
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return ((h >> np.uint32(8)).astype(f32) * f32(2.0 ** -23) - f32(1.0)).astype(f32)


def _pairs(mm, r):
    """Round r of the round-robin tournament on mm (even) players: mm / 2 disjoint pairs (p < q)."""
    k = np.arange(mm // 2)
    a = np.where(k == 0, mm - 1, (r + k) % (mm - 1))
    b = (r + mm - 1 - k) % (mm - 1)
    return np.minimum(a, b), np.maximum(a, b)


def jacobi_eigh(A, d):
    """Parallel cyclic Jacobi in fp32 on a symmetric m x m matrix: (eigenvalues ascending, eigenvectors in that order).
    Rotations below the threshold are skipped; the sweeps stop when one applies none."""
    A = np.array(A, f32)
    m = A.shape[0]
    mm = m + (m & 1)
    V = np.eye(m, dtype=f32)
    scale = f32(np.abs(np.diag(A)).max())
    rel, absf = f32(d["jacobi_rel"]), f32(d["jacobi_abs"]) * scale
    for sweep in range(int(d["jacobi_sweeps"])):
        rotated = False
        for r in range(mm - 1):
            p, q = _pairs(mm, r)
            ok = q < m
            p, q = p[ok], q[ok]
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            act = np.abs(apq) > rel * np.sqrt(np.abs(app * aqq)) + absf
            if not act.any():
                continue
            rotated = True
            with np.errstate(divide="ignore", invalid="ignore"):      # the angle in fp64, rounded once: c^2 + s^2 = 1 to an ulp
                tau = (aqq.astype(np.float64) - app) / (2.0 * apq)
                t = np.sign(tau) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                t = np.where(tau == 0, 1.0, t)
            t = np.where(act, t, 0.0)
            c64 = 1.0 / np.sqrt(1.0 + t * t)
            sn, tn = (t * c64).astype(f32), ((t * c64) / (1.0 + c64)).astype(f32)      # s and tan(phi / 2)
            t = t.astype(f32)
            # every update in the small-correction form x - s (y + tan(phi/2) x): its rounding error follows the size of
            # the change, so a nearly diagonal matrix stays as accurate as it arrived
            Ap, Aq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = Ap - sn * (Aq + tn * Ap), Aq + sn * (Ap - tn * Aq)
            Ap, Aq = A[p, :].copy(), A[q, :].copy()
            A[p, :], A[q, :] = Ap - sn[:, None] * (Aq + tn[:, None] * Ap), Aq + sn[:, None] * (Ap - tn[:, None] * Aq)
            A[p, p], A[q, q] = app - t * apq, aqq + t * apq
            A[p, q] = A[q, p] = np.where(act, f32(0), apq)
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = Vp - sn * (Vq + tn * Vp), Vq + sn * (Vp - tn * Vq)
        if not rotated:
            break
    w = np.diag(A).copy()
    order = np.argsort(w, kind="stable")
    return w[order], V[:, order]


def orthonormalise(Y, d):
    """One pass of the symmetric (Loewdin) form: G = Y^T Y (fp64 accumulation), scaled to a unit diagonal, G = Q S Q^T,
    Y <- Y D^-1/2 Q S^-1/2 Q^T with S floored. Multiplying back by Q^T keeps a nearly orthonormal block where it is (the
    eigenvectors of a nearly-identity G are arbitrary), so the projected matrix of the next Rayleigh-Ritz arrives nearly
    diagonal. Returns the block and the number of floored directions."""
    n, m = Y.shape
    G = Y.astype(np.float64).T @ Y.astype(np.float64)
    dg = np.diag(G).copy()
    dinv = np.where(dg > 0, 1.0 / np.sqrt(np.where(dg > 0, dg, 1.0)), 0.0)
    Gs = (G * dinv[:, None] * dinv[None, :]).astype(f32)
    Gs = ((Gs + Gs.T) * f32(0.5)).astype(f32)
    s, Q = jacobi_eigh(Gs, d)
    lost = int((s < f32(d["gram_floor"])).sum())
    si = (f32(1) / np.sqrt(np.maximum(s, f32(d["gram_floor"])))).astype(f32)
    T = ((Q * si[None, :]).astype(np.float64) @ Q.T.astype(np.float64)) * dinv[:, None]
    return (Y @ T.astype(f32)).astype(f32), lost


def rayleigh_ritz(L, X, d):
    """H = X^T L X with the block's own departure from orthonormality E = X^T X - I (1e-6: the rounding of X's entries)
    taken out to first order in the projected problem: H <- H - (E H + H E) / 2, X <- X (I - E / 2) Q. Without it the
    Ritz values carry an error theta * E, which next to a spectral gap of 5e-4 lambda_max mixes neighbouring vectors."""
    m = X.shape[1]
    W = (L @ X).astype(f32)
    X64 = X.astype(np.float64)
    H = X64.T @ W.astype(np.float64)
    H = (H + H.T) * 0.5
    E = (X64.T @ X64 - np.eye(m)).astype(f32)
    E = ((E + E.T) * f32(0.5)).astype(f32)
    Hf = H.astype(f32)
    Hc = (H - 0.5 * (E @ Hf + Hf @ E).astype(np.float64)).astype(f32)
    Hc = ((Hc + Hc.T) * f32(0.5)).astype(f32)
    theta, Q = jacobi_eigh(Hc, d)
    T = (Q - f32(0.5) * (E @ Q)).astype(f32)
    return (X @ T).astype(f32), theta


def cheb_filter(L, X, degree, a0, a, b, range_max):
    """The scaled three-term recurrence: damps [a, b], grows below a, scaled to 1 at the anchor a0. The degree is cut where
    the filter's gain over the block, T_k((c - a0) / e), would pass ``range_max``: beyond it the columns nearest the cut
    drown in the rounding error of the lowest ones (the remaining steps of the fixed schedule copy)."""
    a0, a, b = f32(a0), f32(a), f32(b)
    e, c = (b - a) * f32(0.5), (b + a) * f32(0.5)
    x0 = (c - a0) / e
    deff = int(np.floor(np.log(f32(2) * f32(range_max)) / np.log(x0 + np.sqrt(x0 * x0 - f32(1)))))
    deff = max(1, min(degree, deff))
    sigma = e / (a0 - c)
    tau = f32(2) / sigma
    Y = (((L @ X) - c * X) * (sigma / e)).astype(f32)
    for _ in range(2, deff + 1):
        sn = f32(1) / (tau - sigma)
        Yn = (((L @ Y) - c * Y) * (f32(2) * sn / e) - (sigma * sn) * X).astype(f32)
        X, Y, sigma = Y, Yn, sn
    return Y


def cut_bounds(theta, ub, d):
    """(anchor, lower cut, upper bound) from the previous Ritz values and the Gershgorin bound, kept apart."""
    ub = f32(ub)
    a0 = f32(min(theta[0], ub * f32(0.5)))
    a = f32(min(max(theta[-1], a0 + f32(d["cut_min"]) * ub), ub * (f32(1) - f32(d["cut_min"]))))
    return a0, a, ub


def lowband_basis(L, lp, d, stats=None):
    """L dense fp32 [N,N] -> (U [N,lp], theta [lp], resid)."""
    L = np.asarray(L, f32)
    n = L.shape[0]
    m = block_size(n, lp, d)
    ub = f32(2) * f32(np.diag(L).max())
    X = hash_unit(np.arange(n)[:, None], np.arange(m)[None, :], 0)
    for _ in range(2):
        X, _lost = orthonormalise(X, d)
    X, theta = rayleigh_ritz(L, X, d)
    for it in range(int(d["iters"])):
        a0, a, b = cut_bounds(theta, ub, d)
        X = cheb_filter(L, X, int(d["degree"]), a0, a, b, min(float(d["range_max"]), float(d["range_first"]) * float(d["range_growth"]) ** it))
        for _ in range(2):
            X, lost = orthonormalise(X, d)
            if stats is not None:
                stats.append((it, lost))
        X, theta = rayleigh_ritz(L, X, d)
    U, th = X[:, :lp], theta[:lp]
    resid = np.abs((L @ U) - U * th[None, :]).max() if lp else 0.0
    return U, th, f32(resid)


# ---- the cloud families of the tests (tests/test_lowband_cpu.py, tests/test_lowband_gpu.py) -----------------------------
def face(n, seed):
    a = np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "face0424.txt"), delimiter=",")[:, :3]
    p = a[np.random.default_rng(seed).choice(len(a), n, replace=False)]
    p = p - p.mean(0)
    return (p / np.linalg.norm(p, axis=1).max()).astype(np.float32)


def ball(n, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return (g * rng.random((n, 1)) ** (1 / 3)).astype(np.float32)


def height_field(n, seed):
    xy = np.random.default_rng(seed).random((n, 2)) * 2 - 1
    return np.concatenate([xy, 0.3 * np.sin(3 * xy[:, :1]) * np.cos(2 * xy[:, 1:])], 1).astype(np.float32)


def sphere(n, seed):
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def two_blobs(n, seed):
    p = 0.3 * np.random.default_rng(seed).standard_normal((n, 3))
    p[n // 2:] += np.array([40.0, 0.0, 0.0])
    return p.astype(np.float32)
