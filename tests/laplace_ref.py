"""The reference of the Poisson-filter tests (tests/test_laplace_ref.py, test_laplace_host.py, test_gpu_laplace.py): a numpy
restatement, in the caller's dtype, of the contract of vjf_laplace_filter (include/vjf_hip.h), on the state arrays
tests/fixed_point_ref.py uses (an OracleState's centroid, logwidth, w_mean) plus the decoder eta = C x + b.

    laplace_filter   the contract: per row the prediction of ekf_ref.ekf (u[t] drives the step INTO row t), the mode by n_iter Newton
                     steps in whitened coordinates with the per-trial step control, the Laplace posterior and evidence, the per-trial
                     selects of an unobserved row and the poisoning
    evaluate, direction   E(z) and D(z) of the contract for a batch, on their own: what the tests differentiate and inspect

The decision `phi_c <= phi` is taken here on the two values as they are, each rounded in the dtype.  The kernel takes it on their
difference formed term by term (include/vjf_hip.h says how): the same inequality, decided to more digits, so in fp32 the kernel ends
nearer the fp64 mode than this reference in fp32 does.
"""
import math

import numpy as np

from tests import fixed_point_ref as fr
from tests.ekf_ref import _T, _chol, _mirror


def _lg(v):
    """math.lgamma, infinite where it overflows (as lgammaf is on the device)."""
    try:
        return math.lgamma(v)
    except OverflowError:
        return math.inf


_lgamma = np.vectorize(_lg, otypes=[np.float64])


def log_pmf_sum(y, obs, eta, lam):
    """sum_j (y_j eta_j - lam_j - lgamma(y_j + 1)) over a row's counts, the terms formed per count (math.lgamma, rounded to the
    dtype); 0 where the row is not observed.  A y that is not finite or negative counts as 0 here: such a trial is poisoned anyway."""
    dt = eta.dtype
    ys = np.where(obs[:, None] & np.isfinite(y) & (y >= 0), y, 0).astype(np.float64)
    lg = _lgamma(ys + 1.0).astype(dt)
    return np.where(obs[:, None], y * eta - lam - lg, dt.type(0)).sum(axis=1)


def evaluate(C, b, mp, Lp, y, obs, z):
    """E(z): x, eta, lam and phi = sum_j (lam_j - y_j eta_j) + |z|^2 / 2; the terms of a row that is not observed are 0 by selects."""
    dt = z.dtype
    x = mp + (Lp @ z[:, :, None])[:, :, 0]
    eta = x @ _T(C) + b
    lam = np.exp(eta)
    terms = np.where(obs[:, None], lam - y * eta, dt.type(0))
    phi = terms.sum(axis=1) + (z * z).sum(axis=1) / dt.type(2)
    return x, eta, lam, phi


def direction(C, Lp, y, obs, z, lam):
    """D(z): H = sum_j lam_j c_j c_j^T, M = I + Lp^T H Lp = Lm Lm^T, grad = z - Lp^T C^T (y - lam), dz = -M^-1 grad.
    Returns Lm, whether its pivots were positive and finite, grad, dz and M."""
    dt = z.dtype
    d = z.shape[1]
    I = np.eye(d, dtype=dt)
    lam0 = np.where(obs[:, None], lam, dt.type(0))
    H = np.einsum("bj,ji,jp->bip", lam0, C, C)
    M = I + _T(Lp) @ H @ Lp
    Lm, ok = _chol(M)
    v = np.where(obs[:, None], y - lam, dt.type(0))
    grad = z - (_T(Lp) @ (v @ C)[:, :, None])[:, :, 0]
    a = np.linalg.solve(Lm, grad[:, :, None])
    dz = -np.linalg.solve(_T(Lm), a)[:, :, 0]
    return Lm, ok, grad, dz, M


def laplace_filter(s, C, b, y, u, q, prior_mean, prior_cov=None, prior_logvar=None, observed=None, n_iter=8):
    """The contract of vjf_laplace_filter in the state's dtype.
    C (ydim, xdim), b (ydim); y (T, B, ydim); u (T, B, udim) or None; q the scalar state variance;
    prior_mean (B, xdim) with prior_cov (B, xdim, xdim) (its lower triangle counts) or prior_logvar (B, xdim);
    observed (T, B) of 0 / 1 or None.
    Returns mean (T, B, xdim), var (T, B, xdim), cov (T, B, xdim, xdim), loglik (T, B), grad_norm (T, B)."""
    dt = s.dtype
    c = lambda a: np.asarray(a, dt)                                    # noqa: E731
    C, b, q = c(C), c(b), dt.type(q)
    y = np.asarray(y, dt)
    T, B, dy = y.shape
    m = c(prior_mean).copy()
    d = m.shape[-1]
    I = np.eye(d, dtype=dt)
    assert (prior_cov is None) != (prior_logvar is None)
    P = _mirror(c(prior_cov)) if prior_cov is not None else np.exp(c(prior_logvar))[:, :, None] * I
    mean, var = np.empty((T, B, d), dt), np.empty((T, B, d), dt)
    cov, loglik, gnorm = np.empty((T, B, d, d), dt), np.empty((T, B), dt), np.empty((T, B), dt)
    bad = np.zeros(B, bool)
    with np.errstate(all="ignore"):
        for t in range(T):
            obs = np.ones(B, bool) if observed is None else np.asarray(observed[t]).astype(bool)
            ut = None if u is None else c(u[t])
            yt = np.where(obs[:, None], y[t], dt.type(0))              # the y of a row that is not observed never enters arithmetic
            bad = bad | ~np.isfinite(m).all(axis=1) | (False if ut is None else ~np.isfinite(ut).all(axis=1))
            bad = bad | ~np.isfinite(yt).all(axis=1) | (yt < 0).any(axis=1)
            # 1. predict
            g, A = fr.g_and_A(s, m, ut)
            mp = m + g
            Ls, okS = _chol(P)
            K = (I + A) @ Ls
            Lp, okP = _chol(K @ _T(K) + q * I)
            # 2. mode
            z = np.zeros((B, d), dt)
            x, eta, lam, phi = evaluate(C, b, mp, Lp, yt, obs, z)
            bad = bad | ~np.isfinite(phi)
            Lm, okM, grad, dz, _ = direction(C, Lp, yt, obs, z, lam)
            alpha = np.ones(B, dt)
            for _ in range(int(n_iter)):
                zc = z + alpha[:, None] * dz
                xc, etac, lamc, phic = evaluate(C, b, mp, Lp, yt, obs, zc)
                acc = (phic <= phi) & np.isfinite(phic)
                a1 = acc[:, None]
                z, x, eta, lam, phi = np.where(a1, zc, z), np.where(a1, xc, x), np.where(a1, etac, eta), np.where(a1, lamc, lam), np.where(acc, phic, phi)
                Lm, ok, grad, dn, _ = direction(C, Lp, yt, obs, z, lam)
                okM = okM & ok
                dz = np.where(a1, dn, dz)
                alpha = np.where(acc, dt.type(1), alpha / dt.type(4))
            # 3. posterior
            mn = x                                                     # = m^- + Lp z
            Y = np.linalg.solve(Lm, _T(Lp))
            Pn = _T(Y) @ Y
            # 4., 5. evidence and |grad|
            ll = log_pmf_sum(yt, obs, eta, lam) - (z * z).sum(axis=1) / dt.type(2) - np.log(np.diagonal(Lm, axis1=-2, axis2=-1)).sum(axis=1)
            gn = np.sqrt((grad * grad).sum(axis=1))
            bad = bad | ~okS | ~okP | ~okM | ~np.isfinite(ll)
            # 6. a row that is not observed: z = 0 and M = I came out of the selects above
            m = mn.copy()
            P = _mirror(Pn)
            ll, gn = np.where(obs, ll, dt.type(0)), np.where(obs, gn, dt.type(0))
            m[bad], P[bad], ll[bad], gn[bad] = np.nan, np.nan, np.nan, np.nan
            mean[t], cov[t], loglik[t], gnorm[t] = m, P, ll, gn
            var[t] = np.diagonal(P, axis1=-2, axis2=-1)
            m, P = np.where(bad[:, None], dt.type(0), m), np.where(bad[:, None, None], I, P)      # (carried finite: `bad` holds the poison)
    return mean, var, cov, loglik, gnorm


__all__ = ["laplace_filter", "evaluate", "direction", "log_pmf_sum"]
