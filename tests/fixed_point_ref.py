"""The reference of the fixed-point tests (tests/test_fixed_point_ref.py, test_fixed_point_host.py, test_gpu_fixed_point.py): a numpy
restatement, in the caller's dtype, of the contract of vjf_fixed_points (include/vjf_hip.h), on the state arrays tests/tangent_ref.py
uses (an OracleState's centroid, logwidth, w_mean).

    g(x, u) = Phi([x, u]) w_mean                           the velocity of the mean map f = x + g
    A(x, u) = dg/dx = -w_mean^T G,  G[k, j] = phi_k (x_j - c_kj) / width_k^2          (J = I + A: tangent_ref.jacobian)

and per trial the damped Newton (Levenberg-Marquardt) search on |g|^2: a candidate is accepted if it lowers r2 = |g|^2 (lam / 10,
floor 1e-7) and rejected otherwise (lam * 10, cap 1e7); the step solves (A^T A + lam mu I) delta = -A^T g, mu = trace(A^T A) / dout, by
numpy.linalg.cholesky, a failed or non-finite factor leaving the candidate at x."""
import numpy as np

from oracle import vjf_oracle as orc
from tests import tangent_ref as tr

LAM_MIN, LAM_MAX = 1e-7, 1e7


def features(s, x, u=None):
    """Phi([x, u]) (B, n) in the state's dtype."""
    x = np.atleast_2d(np.asarray(x, s.dtype))
    return orc.rbf(orc.nonecat(x, None if u is None else np.asarray(u, s.dtype)), s.centroid, np.exp(s.logwidth))


def g_and_A(s, x, u=None):
    """g (B, xdim) and A[b, i, j] = d g_i / d x_j (B, xdim, xdim) at x (B, xdim), u (B, udim) or None."""
    x = np.atleast_2d(np.asarray(x, s.dtype))
    xdim = x.shape[1]
    w = np.exp(s.logwidth)
    phi = features(s, x, u)
    G = (phi / (w * w)[None, :])[:, :, None] * (x[:, None, :] - s.centroid[None, :, :xdim])       # (B, n, xdim)
    return phi @ s.w_mean, -np.einsum("ki,bkj->bij", s.w_mean, G)


def g_scale(s, x, u=None):
    """(|Phi| |w_mean|)(x) per trial (B,): the largest sum of magnitudes behind a component of g."""
    return (np.abs(features(s, x, u)) @ np.abs(s.w_mean)).max(axis=1)


def jacobian(s, x, u=None):
    """J = I + A; the same map as tangent_ref.jacobian."""
    A = g_and_A(s, x, u)[1]
    return np.eye(A.shape[1], dtype=s.dtype)[None] + A


def _step(M, b, shift):
    """delta of (M + shift I) delta = -b through the Cholesky factor, or None where the factor fails."""
    dt = M.dtype
    K = M + shift * np.eye(M.shape[0], dtype=dt)
    if not np.isfinite(K).all():
        return None
    try:
        L = np.linalg.cholesky(K)
    except np.linalg.LinAlgError:
        return None
    if not (np.isfinite(L).all() and (np.diag(L) > 0).all()):
        return None
    y = np.linalg.solve(L, -b)
    return np.linalg.solve(L.T, y).astype(dt)


def solve(s, x0, u=None, max_iter=64, tol=1e-5, lam0=1e-3):
    """The contract, trial by trial: x (B, xdim), residual (B,), n_iter (B,) int32, converged (B,) bool and hist: per trial the list
    of r2 after every comparison (its monotonicity is a test of its own)."""
    dt = s.dtype.type
    x0 = np.atleast_2d(np.asarray(x0, s.dtype))
    B, dout = x0.shape
    U = None if u is None else np.atleast_2d(np.asarray(u, s.dtype))
    tol2 = dt(tol) * dt(tol)
    X, res = np.array(x0, copy=True), np.empty(B, s.dtype)
    nit, conv, hist = np.zeros(B, np.int32), np.zeros(B, bool), []
    with np.errstate(all="ignore"):
        for t in range(B):
            ub = None if U is None else U[t:t + 1]
            x, xc, r2, lam = x0[t].copy(), x0[t].copy(), dt(np.inf), dt(lam0)
            M, b, done, h = np.zeros((dout, dout), s.dtype), np.zeros(dout, s.dtype), False, []
            for k in range(max_iter + 1):
                g, A = g_and_A(s, xc[None], ub)
                g, A = g[0], A[0]
                r2c = dt(np.sum(g * g))
                if r2c < r2:
                    x, r2, M, b = xc.copy(), r2c, (A.T @ A).astype(s.dtype), (A.T @ g).astype(s.dtype)
                    if k > 0:
                        lam = max(lam / dt(10), dt(LAM_MIN))
                else:
                    lam = min(lam * dt(10), dt(LAM_MAX))
                h.append(float(r2))
                done = bool(r2 <= tol2)
                if k == max_iter or done:
                    break
                nit[t] += 1
                mu = dt(np.trace(M)) / dt(dout)
                delta = _step(M, b, dt(lam * mu))
                xc = x.copy() if delta is None else (x + delta).astype(s.dtype)
            X[t], res[t], conv[t] = x, np.sqrt(r2), done
            hist.append(h)
    return X, res, nit, conv, hist


def polish(s64, x, u=None, n_newton=50, target=1e-13):
    """Plain Newton in fp64 from x on g = 0: x** (B, xdim) and its residual (B,)."""
    x = np.array(np.atleast_2d(x), np.float64)
    for _ in range(n_newton):
        g, A = g_and_A(s64, x, u)
        if np.sqrt((g * g).sum(1)).max() < target:
            break
        x = x - np.linalg.solve(A, g[:, :, None])[:, :, 0]
    g = g_and_A(s64, x, u)[0]
    return x, np.sqrt((g * g).sum(1))


__all__ = ["features", "g_and_A", "g_scale", "jacobian", "solve", "polish", "tr"]
