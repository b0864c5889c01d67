"""The reference of the posterior-draw tests (tests/test_sampler_ref.py, test_sampler_host.py, test_gpu_sampler.py): a numpy
restatement, in the caller's dtype, of the contract of vjf_smooth_sample (include/vjf_hip.h), on tests/smoother_ref.py.

    sample_backward   backward sampling in its textbook form on given predictions and Jacobians: nothing of the model
    sample            the contract: the mean map's predictions (smoother_ref.predictions), the factor of I + Jh^T Jh per row, one
                      back-substitution per member
"""
import numpy as np

from tests import smoother_ref as sr
from tests.smoother_ref import _T


def sample_backward(mu, P, m_pred, J, Q, z, after=None):
    """Textbook backward sampling, mirroring smoother_ref.rts_backward.  mu (T, ..., d) filtered means; P (T, ..., d) diagonal or
    (T, ..., d, d) full filtered covariances; m_pred[t] (..., d) and J[t] (..., d, d): the prediction of row t + 1 from row t and its
    Jacobian (T - 1 of them, T with `after`); Q a scalar or (d, d); z (S, T, ..., d) standard-normal values; after (S, ..., d) the draws
    of the row behind the last one.  Returns x (S, T, ..., d):
        x_{T-1} = mu_{T-1} + chol(P_{T-1}) z_{T-1},
        P^- = J P_t J^T + Q,  G = P_t J^T (P^-)^-1,  C = P_t - G J P_t,  x_t = mu_t + G (x_{t+1} - m^-) + chol(C) z_t
    (the lower Cholesky factor: another factor of C than the contract's, the same distribution)."""
    mu = np.asarray(mu)
    dt, T, d = mu.dtype, mu.shape[0], mu.shape[-1]
    P, z = np.asarray(P, dt), np.asarray(z, dt)
    diag = P.ndim == mu.ndim
    full = (lambda p: p[..., :, None] * np.eye(d, dtype=dt)) if diag else (lambda p: p)
    Qm = np.asarray(Q, dt) * np.eye(d, dtype=dt) if np.ndim(Q) == 0 else np.asarray(Q, dt)
    x = np.empty_like(z)
    mv = lambda A, v: (A @ v[..., None])[..., 0]                                          # noqa: E731
    if after is None:
        cur = mu[-1] + mv(np.linalg.cholesky(full(P[-1])), z[:, -1])
        x[:, -1] = cur
        start = T - 2
    else:
        cur = np.asarray(after, dt)
        start = T - 1
    for t in range(start, -1, -1):
        D, Jt = full(P[t]), np.asarray(J[t], dt)
        Pp = Jt @ D @ _T(Jt) + Qm
        G = _T(np.linalg.solve(Pp, Jt @ D))
        C = D - G @ Jt @ D
        C = (C + _T(C)) / 2
        cur = mu[t] + mv(G, cur - np.asarray(m_pred[t], dt)) + mv(np.linalg.cholesky(C), z[:, t])
        x[:, t] = cur
    return x


def sample(s, mu, lv, u, q, z, after=None):
    """The contract of vjf_smooth_sample in the state's dtype: x (S, T, B, xdim).
    mu, lv (T, B, xdim); u (T, B, udim) -- (T + 1, B, udim) with `after` -- or None; q the scalar state-noise variance; z (S, T, B, xdim)
    standard-normal values; after (S, B, xdim): the draws of the row behind the last one."""
    dt = s.dtype
    mu, lv, z = np.asarray(mu, dt), np.asarray(lv, dt), np.asarray(z, dt)
    u = None if u is None else np.asarray(u, dt)
    T, B, d = mu.shape
    assert z.shape[1:] == (T, B, d), z.shape
    mp, Js = sr.predictions(s, mu, u, after is not None)
    I = np.eye(d, dtype=dt)
    rq = (1 / np.sqrt(np.asarray(q, dt))).astype(dt)
    x = np.empty_like(z)
    if after is None:
        cur = mu[-1] + np.exp(dt.type(0.5) * lv[-1]) * z[:, -1]
        x[:, -1] = cur
        start = T - 2
    else:
        cur = np.asarray(after, dt)
        start = T - 1
    for t in range(start, -1, -1):
        sd = np.exp(dt.type(0.5) * lv[t])
        Jh = Js[t] * sd[:, None, :] * rq
        M = I + _T(Jh) @ Jh
        L = np.linalg.cholesky(M)
        Li = np.linalg.solve(L, np.broadcast_to(I, M.shape))                # L^-1
        G = sd[:, :, None] * (_T(Li) @ Li @ _T(Jh)) * rq
        w = (_T(Li) @ z[:, t][..., None])[..., 0]                            # L^T w = z, per member (broadcast over S)
        cur = (mu[t] + (G @ (cur - mp[t])[..., None])[..., 0]) + sd * w
        x[:, t] = cur
    return x


__all__ = ["sample_backward", "sample"]
