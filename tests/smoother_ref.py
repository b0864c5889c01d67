"""The reference of the smoother tests (tests/test_smoother_ref.py, test_smoother_host.py, test_gpu_smoother.py): a numpy restatement,
in the caller's dtype, of the contract of vjf_smooth (include/vjf_hip.h), on the state arrays tests/fixed_point_ref.py uses (an
OracleState's centroid, logwidth, w_mean).

    rts_backward   the Rauch-Tung-Striebel backward pass in its textbook form on given predictions and Jacobians: nothing of the model
    smooth         the extended pass with the mean map f(x, u) = x + g(x, u) and J = I + A of fixed_point_ref.g_and_A, the step from row t
                   to row t + 1 driven by u[t + 1], in the "information" form of the contract or through rts_backward ("textbook")
"""
import numpy as np

from tests import fixed_point_ref as fr


def _T(a):
    return np.swapaxes(a, -1, -2)


def rts_backward(mu, P, m_pred, J, Q, after=None):
    """Textbook RTS.  mu (T, ..., d) filtered means; P (T, ..., d) diagonal or (T, ..., d, d) full filtered covariances; m_pred[t]
    (..., d) and J[t] (..., d, d): the prediction of row t + 1 from row t and its Jacobian (T - 1 of them, T with `after`); Q a scalar
    or (d, d).  after = (mean, cov) of the row behind the last one.  Returns ms (T, ..., d), Ps (T, ..., d, d):
        P^- = J P_t J^T + Q,  G = P_t J^T (P^-)^-1,  ms_t = mu_t + G (ms_{t+1} - m^-),  Ps_t = P_t + G (Ps_{t+1} - P^-) G^T."""
    mu = np.asarray(mu)
    dt, T, d = mu.dtype, mu.shape[0], mu.shape[-1]
    P = np.asarray(P, dt)
    diag = P.ndim == mu.ndim
    full = (lambda p: p[..., :, None] * np.eye(d, dtype=dt)) if diag else (lambda p: p)
    Qm = np.asarray(Q, dt) * np.eye(d, dtype=dt) if np.ndim(Q) == 0 else np.asarray(Q, dt)
    ms, Ps = np.empty_like(mu), np.empty(mu.shape + (d,), dt)
    if after is None:
        m, S = mu[-1], full(P[-1])
        ms[-1], Ps[-1] = m, S
        start = T - 2
    else:
        m, S = np.asarray(after[0], dt), np.asarray(after[1], dt)
        start = T - 1
    for t in range(start, -1, -1):
        D, Jt = full(P[t]), np.asarray(J[t], dt)
        Pp = Jt @ D @ _T(Jt) + Qm
        G = _T(np.linalg.solve(Pp, Jt @ D))                  # D J^T (P^-)^-1  (D and P^- are symmetric)
        m = mu[t] + (G @ (m - np.asarray(m_pred[t], dt))[..., None])[..., 0]
        S = D + G @ (S - Pp) @ _T(G)
        ms[t], Ps[t] = m, S
    return ms, Ps


def predictions(s, mu, u, after=False):
    """m^-[t] = f(mu_t, u_{t+1}) (.., B, xdim) and J[t] (.., B, xdim, xdim) for t = 0 .. T - 2 (T - 1 with `after`: u has T + 1 rows)."""
    T = mu.shape[0]
    mp, Js = [], []
    for t in range(T - (0 if after else 1)):
        g, A = fr.g_and_A(s, mu[t], None if u is None else u[t + 1])
        mp.append(mu[t] + g)
        Js.append(np.eye(mu.shape[-1], dtype=s.dtype)[None] + A)
    return mp, Js


def _mirror(S):
    """The symmetric matrix whose lower triangle is S's (the contract carries the lower triangle)."""
    L = np.tril(S)
    return L + _T(np.tril(S, -1))


def smooth(s, mu, lv, u, q, form="information", after=None):
    """The contract of vjf_smooth in the state's dtype: mean (T, B, xdim), var (T, B, xdim), cov (T, B, xdim, xdim).
    mu, lv (T, B, xdim); u (T, B, udim) -- (T + 1, B, udim) with `after` -- or None; q the scalar state-noise variance;
    after = (mean (B, xdim), cov (B, xdim, xdim)): the smoothed moments of the row behind the last one (its lower triangle counts)."""
    dt = s.dtype
    mu, lv = np.asarray(mu, dt), np.asarray(lv, dt)
    u = None if u is None else np.asarray(u, dt)
    T, B, d = mu.shape
    if after is not None:
        after = (np.asarray(after[0], dt), _mirror(np.asarray(after[1], dt)))
    mp, Js = predictions(s, mu, u, after is not None)
    if form == "textbook":
        mean, cov = rts_backward(mu, np.exp(lv), mp, Js, dt.type(q), after)
    elif form == "information":
        I = np.eye(d, dtype=dt)
        rq = (1 / np.sqrt(np.asarray(q, dt))).astype(dt)
        mean, cov = np.empty_like(mu), np.empty((T, B, d, d), dt)
        if after is None:
            ms, Ps = mu[-1].copy(), np.exp(lv[-1])[:, :, None] * I
            mean[-1], cov[-1] = ms, Ps
            start = T - 2
        else:
            ms, Ps = after
            start = T - 1
        for t in range(start, -1, -1):
            sd = np.exp(dt.type(0.5) * lv[t])
            Jh = Js[t] * sd[:, None, :] * rq
            M = I + _T(Jh) @ Jh
            L = np.linalg.cholesky(M)
            Li = np.linalg.solve(L, np.broadcast_to(I, M.shape))               # L^-1
            Minv = _T(Li) @ Li
            C = sd[:, :, None] * Minv * sd[:, None, :]
            G = sd[:, :, None] * (Minv @ _T(Jh)) * rq
            ms = mu[t] + (G @ (ms - mp[t])[..., None])[..., 0]
            K = G @ np.linalg.cholesky(Ps)
            Ps = _mirror(C + K @ _T(K))
            mean[t], cov[t] = ms, Ps
    else:
        raise ValueError(form)
    return mean, np.diagonal(cov, axis1=-2, axis2=-1).copy(), cov


__all__ = ["rts_backward", "predictions", "smooth"]
