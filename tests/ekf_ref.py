"""The reference of the extended-Kalman-filter tests (tests/test_ekf_ref.py, test_ekf_host.py, test_gpu_ekf.py): a numpy restatement,
in the caller's dtype, of the contract of vjf_ekf (include/vjf_hip.h), on the state arrays tests/fixed_point_ref.py uses (an
OracleState's centroid, logwidth, w_mean) plus the decoder y = C x + b.

    ekf        the contract: per row the prediction through the mean map f(x, u) = x + g(x, u) and J = I + A of fixed_point_ref.g_and_A
               (u[t] drives the step INTO row t), the update in the factored form of the contract, the row log-likelihood, the per-trial
               selects of an unobserved row and the poisoning
    textbook   the filter as the books state it (K = P^- C^T S^-1, slogdet S) on a linear-Gaussian model: nothing of the model
"""
import math

import numpy as np

from tests import fixed_point_ref as fr


def _T(a):
    return np.swapaxes(a, -1, -2)


def _mirror(S):
    """The symmetric matrix whose lower triangle is S's (the contract carries the lower triangle)."""
    return np.tril(S) + _T(np.tril(S, -1))


def _chol(S):
    """Per trial: the Cholesky factor of S (B, d, d) and whether every pivot was positive and finite (the identity where not)."""
    d = S.shape[-1]
    ok = np.isfinite(S).all(axis=(-1, -2))
    L = np.broadcast_to(np.eye(d, dtype=S.dtype), S.shape).copy()
    if ok.all():
        try:
            L = np.linalg.cholesky(S)
            return L, np.isfinite(L).all(axis=(-1, -2))
        except np.linalg.LinAlgError:
            pass
    for b in np.nonzero(ok)[0]:
        try:
            L[b] = np.linalg.cholesky(S[b])
        except np.linalg.LinAlgError:
            ok[b] = False
    ok &= np.isfinite(L).all(axis=(-1, -2))
    L[~ok] = np.eye(d, dtype=S.dtype)
    return L, ok


def ekf(s, C, b, y, u, q, r, prior_mean, prior_cov=None, prior_logvar=None, observed=None):
    """The contract of vjf_ekf in the state's dtype.
    C (ydim, xdim), b (ydim); y (T, B, ydim); u (T, B, udim) or None; q, r the scalar state and observation variances;
    prior_mean (B, xdim) with prior_cov (B, xdim, xdim) (its lower triangle counts) or prior_logvar (B, xdim);
    observed (T, B) of 0 / 1 or None.  Returns mean (T, B, xdim), var (T, B, xdim), cov (T, B, xdim, xdim), loglik (T, B)."""
    dt = s.dtype
    c = lambda a: np.asarray(a, dt)                                    # noqa: E731
    C, b, q, r = c(C), c(b), dt.type(q), dt.type(r)
    y = np.asarray(y, dt)
    T, B, dy = y.shape
    m = c(prior_mean).copy()
    d = m.shape[-1]
    I = np.eye(d, dtype=dt)
    assert (prior_cov is None) != (prior_logvar is None)
    P = _mirror(c(prior_cov)) if prior_cov is not None else np.exp(c(prior_logvar))[:, :, None] * I
    G = (_T(C) @ C) / r
    const = dt.type(dy) * (dt.type(math.log(2 * math.pi)) + np.log(r))
    mean, var = np.empty((T, B, d), dt), np.empty((T, B, d), dt)
    cov, loglik = np.empty((T, B, d, d), dt), np.empty((T, B), dt)
    bad = np.zeros(B, bool)
    half = dt.type(0.5)
    with np.errstate(all="ignore"):
        for t in range(T):
            obs = np.ones(B, bool) if observed is None else np.asarray(observed[t]).astype(bool)
            ut = None if u is None else c(u[t])
            bad = bad | ~np.isfinite(m).all(axis=1) | (False if ut is None else ~np.isfinite(ut).all(axis=1))
            g, A = fr.g_and_A(s, m, ut)
            mp = m + g
            Ls, okS = _chol(P)
            K = (I + A) @ Ls
            Lp, okP = _chol(K @ _T(K) + q * I)
            Gt = np.where(obs[:, None, None], G, dt.type(0))           # an unobserved row: the update with C^T C / r = 0, M = I
            Lm, okM = _chol(I + _T(Lp) @ Gt @ Lp)
            yt = np.where(obs[:, None], y[t], dt.type(0))              # its y never enters arithmetic
            v = np.where(obs[:, None], yt - b - mp @ _T(C), dt.type(0))
            sv = (v @ C) / r
            Y = np.linalg.solve(Lm, _T(Lp))
            Pn = _T(Y) @ Y
            mn = mp + (Pn @ sv[:, :, None])[:, :, 0]
            v2 = np.where(obs[:, None], yt - b - mn @ _T(C), dt.type(0))
            z = np.linalg.solve(Lp, (mn - mp)[:, :, None])[:, :, 0]
            logdet = const + 2 * np.log(np.diagonal(Lm, axis1=-2, axis2=-1)).sum(axis=1)
            ll = -half * (logdet + (v2 * v2).sum(axis=1) / r + (z * z).sum(axis=1))
            bad = bad | ~okS | ~okP | (obs & (~okM | ~np.isfinite(ll)))
            m = np.where(obs[:, None], mn, mp)
            P = _mirror(Pn)
            ll = np.where(obs, ll, dt.type(0))
            m[bad], P[bad], ll[bad] = np.nan, np.nan, np.nan
            mean[t], cov[t], loglik[t] = m, P, ll
            var[t] = np.diagonal(P, axis1=-2, axis2=-1)
            m, P = np.where(bad[:, None], dt.type(0), m), np.where(bad[:, None, None], I, P)      # (carried finite: `bad` holds the poison)
    return mean, var, cov, loglik


def textbook(F, Q, C, b, R, y, m0, P0, observed=None):
    """The Kalman filter of x_t = F x_{t-1} + N(0, Q), y_t = C x_t + b + N(0, R) for one trial, as the books state it: the gain
    K = P^- C^T S^-1, P = P^- - K S K^T and log N(y; C m^- + b, S) through slogdet.  y (T, ydim); row 0 is predicted from (m0, P0).
    Returns mean (T, d), cov (T, d, d), loglik (T,)."""
    m, P = np.asarray(m0, np.float64), np.asarray(P0, np.float64)
    T, dy = y.shape
    means, covs, lls = [], [], []
    for t in range(T):
        m, P = F @ m, F @ P @ F.T + Q
        ll = 0.0
        if observed is None or observed[t]:
            S = C @ P @ C.T + R
            v = y[t] - b - C @ m
            K = np.linalg.solve(S, C @ P).T
            m, P = m + K @ v, P - K @ S @ K.T
            ll = -0.5 * (dy * math.log(2 * math.pi) + np.linalg.slogdet(S)[1] + v @ np.linalg.solve(S, v))
        means.append(m), covs.append(P), lls.append(ll)
    return np.stack(means), np.stack(covs), np.asarray(lls)


__all__ = ["ekf", "textbook"]
