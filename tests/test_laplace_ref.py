"""The reference of the Poisson-filter tests itself (tests/laplace_ref.py) and the conditions on the yardstick (tests/laplace_cases.py),
on the CPU:

  1. grad and M of D(z) against autograd of phi in torch fp64;
  2. one dimension, ydim = 1: the evidence against Gauss-Hermite quadrature of the true integral, and how it falls with the prior variance;
  3. C = 0: loglik is the Poisson log-pmf at exp(b), summed; P = P^-; m = m^-;
  4. chunking with `before`, rows that are not observed, every poison rule;
  5. a start so far off that the first full step overflows: rejected, and the row still converges;
  6. the yardstick: E <= 1e-3 scale for every case, regime and gap setting, the fp64 grad_norm <= 1e-5 at n_iter = 8, and n_iter = 8
     against n_iter = 30 within 1e-7 scale."""
import math

import numpy as np
import pytest
import torch

from oracle import vjf_oracle as orc
from tests import laplace_cases as lc
from tests import laplace_ref as lr

NAMES = list(lc.CASES)
REGIMES = list(lc.REGIMES)


def small_state(xdim=3, udim=1, n=7, seed=0, w=0.3):
    g = np.random.default_rng(seed)
    s = orc.OracleState(1, xdim, udim, n, (1,), orc.GAUSSIAN)
    s.centroid, s.logwidth = g.standard_normal((n, xdim + udim)), 0.3 * g.standard_normal(n)
    s.w_mean = w * g.standard_normal((n, xdim))
    return s


def small_problem(seed=1, xdim=3, udim=1, ydim=6, B=5, T=7):
    g = np.random.default_rng(seed)
    s = small_state(xdim, udim, seed=seed)
    C, b = 0.5 * g.standard_normal((ydim, xdim)), 0.5 + 0.3 * g.standard_normal(ydim)
    u = g.standard_normal((T, B, udim)) if udim else None
    y = g.poisson(2.0, (T, B, ydim)).astype(np.float64)
    x0 = g.standard_normal((B, xdim))
    A = 0.3 * g.standard_normal((B, xdim, xdim))
    P0 = A @ np.swapaxes(A, -1, -2) + 0.05 * np.eye(xdim)
    return s, C, b, y, u, x0, P0


# ------------------------------------------------------------------ 1
def test_grad_and_M_against_autograd():
    g = np.random.default_rng(3)
    B, d, dy = 4, 3, 6
    C, b = 0.5 * g.standard_normal((dy, d)), 0.3 * g.standard_normal(dy)
    mp, z = g.standard_normal((B, d)), 0.5 * g.standard_normal((B, d))
    Lp = np.tril(0.3 * g.standard_normal((B, d, d))) + np.eye(d)
    y = g.poisson(2.0, (B, dy)).astype(np.float64)
    obs = np.array([True, True, False, True])
    _, _, lam, phi = lr.evaluate(C, b, mp, Lp, y, obs, z)
    Lm, ok, grad, dz, M = lr.direction(C, Lp, y, obs, z, lam)
    assert ok.all()
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)          # noqa: E731
    for k in range(B):
        def f(zz):
            eta = t(C) @ (t(mp[k]) + t(Lp[k]) @ zz) + t(b)
            like = (eta.exp() - t(y[k]) * eta).sum() if obs[k] else 0.0
            return like + 0.5 * (zz * zz).sum()
        zk = t(z[k]).requires_grad_(True)
        assert float(f(zk).detach()) == pytest.approx(float(phi[k]), rel=1e-13)
        np.testing.assert_allclose(grad[k], torch.autograd.grad(f(zk), zk)[0].numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(M[k], torch.autograd.functional.hessian(f, t(z[k])).numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(Lm[k] @ Lm[k].T, M[k], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(M[k] @ dz[k], -grad[k], rtol=1e-11, atol=1e-12)
    assert np.array_equal(M[2], np.eye(d)) and np.array_equal(grad[2], z[2])


# ------------------------------------------------------------------ 2
def _row_evidence(cc, bb, yy, pv):
    """(Laplace, quadrature) log p(y) of one count under x ~ N(0, pv), eta = cc x + bb: row 0 of the reference with a zero flow."""
    s = small_state(1, 0, n=3, w=0.0)
    q = 0.5 * pv
    out = lr.laplace_filter(s, np.array([[cc]]), np.array([bb]), np.array([[[yy]]], np.float64), None, q, np.zeros((1, 1)),
                            prior_logvar=np.full((1, 1), math.log(pv - q)), n_iter=30)
    x, w = np.polynomial.hermite_e.hermegauss(120)
    eta = cc * math.sqrt(pv) * x + bb
    logp = yy * eta - np.exp(eta) - math.lgamma(yy + 1.0)
    exact = math.log(float((w * np.exp(logp)).sum()) / math.sqrt(2 * math.pi))
    return float(out[3][0, 0]), exact


@pytest.mark.parametrize("cc, bb", [(1.0, math.log(5.0)), (2.0, 0.0)])
def test_the_evidence_against_quadrature_in_one_dimension(cc, bb):
    for yy in (0.0, 3.0, 12.0):
        e2, e3 = (abs(np.subtract(*_row_evidence(cc, bb, yy, pv))) for pv in (1e-2, 1e-3))
        print(f"c = {cc} b = {bb:.3f} y = {yy}: |laplace - quadrature| = {e2:.2e} at 1e-2, {e3:.2e} at 1e-3, ratio {e2 / e3:.0f}")
        assert e3 < 1e-5
        assert 50 <= e2 / e3 <= 200


# ------------------------------------------------------------------ 3
def test_a_zero_decoder():
    s, C, b, y, u, x0, P0 = small_problem()
    mean, var, cov, ll, gn = lr.laplace_filter(s, 0 * C, b, y, u, 0.02, x0, prior_cov=P0)
    none = np.zeros(y.shape[:2], np.uint8)
    pm, pv, pc, pl, pg = lr.laplace_filter(s, 0 * C, b, y, u, 0.02, x0, prior_cov=P0, observed=none)
    np.testing.assert_array_equal(mean, pm)
    np.testing.assert_array_equal(cov, pc)
    pmf = (y * b - np.exp(b) - np.vectorize(math.lgamma)(y + 1.0)).sum(axis=2)
    np.testing.assert_allclose(ll, pmf, rtol=1e-13)
    assert (gn == 0).all() and (pl == 0).all() and (pg == 0).all()


# ------------------------------------------------------------------ 4
def test_chunking_with_before():
    s, C, b, y, u, x0, P0 = small_problem()
    obs = np.ones(y.shape[:2], np.uint8)
    obs[2, 1] = obs[0, 3] = 0
    whole = lr.laplace_filter(s, C, b, y, u, 0.02, x0, prior_cov=P0, observed=obs)
    for k in (1, 3, 6):
        head = lr.laplace_filter(s, C, b, y[:k], u[:k], 0.02, x0, prior_cov=P0, observed=obs[:k])
        tail = lr.laplace_filter(s, C, b, y[k:], u[k:], 0.02, head[0][-1], prior_cov=head[2][-1], observed=obs[k:])
        for a, h, t in zip(whole, head, tail):
            np.testing.assert_array_equal(a, np.concatenate([h, t]))
    junk = P0 + np.triu(np.full_like(P0, np.nan), 1)
    for a, c in zip(whole, lr.laplace_filter(s, C, b, y, u, 0.02, x0, prior_cov=junk, observed=obs)):
        np.testing.assert_array_equal(a, c)


def test_rows_that_are_not_observed():
    s, C, b, y, u, x0, P0 = small_problem()
    obs = np.ones(y.shape[:2], np.uint8)
    obs[0, 0] = obs[2:4, 1] = obs[-1, 2] = 0
    obs[:, 3] = 0
    out = lr.laplace_filter(s, C, b, y, u, 0.02, x0, prior_cov=P0, observed=obs)
    o = obs.astype(bool)
    assert (out[3][~o] == 0).all() and (out[3][o] != 0).all() and (out[4][~o] == 0).all()
    yn = y.copy()
    yn[~o] = np.nan
    for a, c in zip(out, lr.laplace_filter(s, C, b, yn, u, 0.02, x0, prior_cov=P0, observed=obs)):
        np.testing.assert_array_equal(a, c)
    # the trial that is never observed follows the prediction: the mean map's roll-out, and P^- of P^- ...
    from tests import fixed_point_ref as fr
    m, P = x0[3:4], P0[3:4]
    for t in range(y.shape[0]):
        g, A = fr.g_and_A(s, m, u[t, 3:4])
        J = np.eye(3) + A
        m, P = m + g, J @ P @ np.swapaxes(J, -1, -2) + 0.02 * np.eye(3)
        np.testing.assert_allclose(out[0][t, 3], m[0], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(out[2][t, 3], P[0], rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("what", ["y nan", "y inf", "y negative", "u nan", "prior mean", "prior cov", "phi at z = 0", "loglik"])
def test_every_poison_rule(what):
    s, C, b, y, u, x0, P0 = small_problem()
    whole = lr.laplace_filter(s, C, b, y, u, 0.02, x0, prior_cov=P0)
    y, u, x0, P0 = y.copy(), u.copy(), x0.copy(), P0.copy()
    bad, t0 = 2, 3
    if what.startswith("y"):
        y[t0, bad, 1] = {"y nan": np.nan, "y inf": np.inf, "y negative": -1.0}[what]
    elif what == "u nan":
        u[t0, bad, 0] = np.nan
    elif what == "prior mean":
        x0[bad, 0], t0 = np.nan, 0
    elif what == "prior cov":
        P0[bad], t0 = -P0[bad], 0
    elif what == "phi at z = 0":
        x0[bad], t0 = 1e4, 0                       # exp(eta) overflows at the prediction
    else:
        y[t0, bad, 1] = 1e306                      # finite, and so is phi, but lgamma(y + 1) is not
    out = lr.laplace_filter(s, C, b, y, u, 0.02, x0, prior_cov=P0)
    others = [r for r in range(y.shape[1]) if r != bad]
    for a, w in zip(out, whole):
        np.testing.assert_array_equal(a[:, others], w[:, others])
        np.testing.assert_array_equal(a[:t0, bad], w[:t0, bad])
        assert np.isnan(a[t0:, bad]).all(), what


# ------------------------------------------------------------------ 5
def test_an_overflowing_first_step_is_rejected_and_the_row_converges():
    """One count y = 400 seen through c = 4 from a prediction at eta = -3 under a prior of variance 1: the full Newton step lands at
    eta of order a thousand, where exp overflows -- in fp32 and in fp64."""
    s = small_state(1, 0, n=3, w=0.0)
    for dt in (np.float64, np.float32):
        out = lr.laplace_filter(s.cast(dt) if dt == np.float32 else s, np.array([[4.0]], dt), np.array([-3.0], dt),
                                np.array([[[400.0]]], dt), None, 0.5, np.zeros((1, 1), dt), prior_logvar=np.full((1, 1), math.log(0.5), dt),
                                n_iter=30)
        mean, var, cov, ll, gn = (np.asarray(a, np.float64) for a in out)
        assert np.isfinite(ll).all() and np.isfinite(mean).all()
        # the first candidate: z_c = dz at z = 0
        lam0 = math.exp(-3.0)
        dz0 = 4.0 * (400.0 - lam0) / (1.0 + 16.0 * lam0)
        with np.errstate(over="ignore"):
            assert not np.isfinite(np.exp(dt(4.0 * dz0 - 3.0)))
        assert gn[0, 0] <= (1e-8 if dt == np.float64 else 1e-1)
        eta = 4.0 * mean[0, 0, 0] - 3.0
        assert abs(4.0 * (400.0 - math.exp(eta)) - mean[0, 0, 0]) <= (1e-6 if dt == np.float64 else 0.5)     # the stationarity of the mode


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", NAMES)
def test_the_conditions_on_the_yardstick(name, regime):
    worst = {}
    for gaps in (False, True):
        ref = lc.references(name, regime, gaps)
        for what in lc.TENSORS:
            r64, r32 = ref[what]
            lc.bound(what, r64, r32, name, regime)                     # asserts E <= 1e-3 scale, finite, |mean| < 100
            E = float(np.abs(np.asarray(r32, np.float64) - r64).max()) / lc.scale_of(what, r64, name, regime, r32)
            worst[what] = max(worst.get(what, 0.0), E)
        g64 = float(ref["grad_norm"][0].max())
        assert g64 <= 1e-5, f"fp64 grad_norm {g64:.2e}"
    long = lc.run_reference(name, regime, False, np.float64, n_iter=30)
    ref = lc.references(name, regime, False)
    for i, what in enumerate(lc.TENSORS[:4]):
        d = float(np.abs(long[i] - ref[what][0]).max())
        assert d <= 1e-7 * lc.scale_of(what, ref[what][0]), f"{what}: n_iter 8 against 30: {d:.2e}"
    y = lc.inputs(name, regime)["y"]
    print(f"{name} {regime}: E / scale {worst}, mean count {y.mean():.2f}, max {y.max():.0f}")
