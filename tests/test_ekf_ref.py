"""The reference of the extended-Kalman-filter tests against what it restates (tests/ekf_ref.py), all in fp64 on the CPU:
the textbook filter and the dense joint Gaussian of a linear-Gaussian model (w_mean = 0 makes the flow the identity), with and without
gaps; fixed_point_ref.g_and_A for the nonlinear part; chunking with `before`; nothing observed; poisoning; and that every case and regime
of tests/ekf_cases.py meets the conditions of the comparison rule."""
import math

import numpy as np
import pytest

from oracle import vjf_oracle as orc
from tests import ekf_cases as ec
from tests import ekf_ref as er
from tests import fixed_point_ref as fr

# (xdim, ydim) x (r, q): the shapes and settings the factored form was checked at
SHAPES = [(3, 7), (10, 50), (17, 33), (24, 7), (1, 3)]
SETTINGS = [(10.0, 1e-2), (0.1, 1e-4), (1e-3, 1e-2), (1e-3, 1e-4)]


def linear_state(xdim, n=6, seed=0):
    """A state whose flow is the identity: w_mean = 0."""
    r = np.random.default_rng(seed)
    s = orc.OracleState(1, xdim, 0, n, (1,), orc.GAUSSIAN)
    s.centroid, s.logwidth, s.w_mean = r.standard_normal((n, xdim)), np.zeros(n), np.zeros((n, xdim))
    return s


def linear_problem(xdim, ydim, T, B, seed):
    r = np.random.default_rng(seed)
    C, b = 0.5 * r.standard_normal((ydim, xdim)), 0.1 * r.standard_normal(ydim)
    A = r.standard_normal((B, xdim, xdim))
    P0 = 0.05 * np.eye(xdim) + 0.02 * A @ np.swapaxes(A, 1, 2) / xdim
    return C, b, r.standard_normal((T, B, ydim)), r.standard_normal((B, xdim)), P0


def gap_pattern(T, B):
    o = np.ones((T, B), np.uint8)
    o[0, 0::2] = 0
    o[2:4, 1::3] = 0
    o[T - 1, 0::3] = 0
    return o


def close(a, b, tol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err, scale = float(np.abs(a - b).max()), float(np.abs(b).max())
    assert err <= tol * max(scale, 1e-300), f"{what}: {err:.3e} against {scale:.3e}"


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("xdim,ydim", SHAPES)
def test_against_the_textbook_filter_on_a_linear_model(xdim, ydim, gaps):
    T, B = 6, 3
    s = linear_state(xdim)
    for k, (r, q) in enumerate(SETTINGS):
        C, b, y, m0, P0 = linear_problem(xdim, ydim, T, B, 10 * xdim + k)
        obs = gap_pattern(T, B) if gaps else None
        mean, var, cov, ll = er.ekf(s, C, b, y, None, q, r, m0, prior_cov=P0, observed=obs)
        for t in range(B):
            tm, tc, tl = er.textbook(np.eye(xdim), q * np.eye(xdim), C, b, r * np.eye(ydim), y[:, t], m0[t], P0[t],
                                     None if obs is None else obs[:, t])
            close(mean[:, t], tm, 1e-11, f"mean r={r} q={q}")
            close(cov[:, t], tc, 1e-8, f"cov r={r} q={q}")
            close(ll[:, t], tl, 1e-11, f"loglik r={r} q={q}")
        np.testing.assert_array_equal(var, np.diagonal(cov, axis1=-2, axis2=-1))
        np.testing.assert_array_equal(cov, np.swapaxes(cov, -1, -2))
        if gaps:
            assert (ll[obs == 0] == 0).all()


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("xdim,ydim,T", [(3, 7, 6), (5, 2, 5), (1, 3, 4)])
def test_the_evidence_is_the_dense_joint_gaussian(xdim, ydim, T, gaps):
    """sum_t loglik = log N(y_obs; mean, cov) of the joint Gaussian of the observed rows of x_t = x_{t-1} + N(0, q), y_t = C x_t + b + N(0, r)."""
    s = linear_state(xdim)
    r, q = 0.1, 0.01
    C, b, y, m0, P0 = linear_problem(xdim, ydim, T, 1, 77 + xdim)
    obs = gap_pattern(T, 2)[:, :1] if gaps else np.ones((T, 1), np.uint8)
    ll = er.ekf(s, C, b, y, None, q, r, m0, prior_cov=P0, observed=obs)[3][:, 0]
    # cov(x_s, x_t) = P0 + min(s, t) q I with rows counted from 1; the mean of every x_t is m0
    Sx = np.block([[P0[0] + (min(i, j) + 1) * q * np.eye(xdim) for j in range(T)] for i in range(T)])
    Cb = np.kron(np.eye(T), C)
    Sy = Cb @ Sx @ Cb.T + r * np.eye(T * ydim)
    my = np.tile(C @ m0[0] + b, T)
    keep = np.repeat(obs[:, 0].astype(bool), ydim)
    Sy, dv = Sy[np.ix_(keep, keep)], (y[:, 0].reshape(-1) - my)[keep]
    joint = -0.5 * (keep.sum() * math.log(2 * math.pi) + np.linalg.slogdet(Sy)[1] + dv @ np.linalg.solve(Sy, dv))
    assert abs(ll.sum() - joint) <= 1e-10 * abs(joint)


def test_the_nonlinear_part_is_g_and_A():
    """One row from a tiny prior covariance: the mean moves by g and the predicted covariance is J P J^T + q I of fixed_point_ref."""
    name = "control"
    s, (C, b), a = ec.state(name), ec.decoder(name), ec.inputs(name)
    x0, u = a["x0"].astype(np.float64), a["u"].astype(np.float64)
    B, d = x0.shape
    r = np.random.default_rng(5)
    Z = r.standard_normal((B, d, d))
    P0 = 0.01 * np.eye(d) + 0.01 * Z @ np.swapaxes(Z, 1, 2) / d
    obs = np.zeros((1, B), np.uint8)
    mean, var, cov, ll = er.ekf(s, C, b, a["y"][:1].astype(np.float64), u[:1], 0.01, 0.1, x0, prior_cov=P0, observed=obs)
    g, A = fr.g_and_A(s, x0, u[0])
    J = np.eye(d) + A
    close(mean[0], x0 + g, 1e-14, "m^-")
    close(cov[0], J @ P0 @ np.swapaxes(J, 1, 2) + 0.01 * np.eye(d), 1e-13, "P^-")
    assert (ll == 0).all()


@pytest.mark.parametrize("name", ["control", "x24"])
def test_nothing_observed_is_the_roll_out(name):
    s, (C, b), a = ec.state(name), ec.decoder(name), ec.inputs(name)
    xdim, udim, n, ydim, B, T = ec.CASES[name]
    u = None if a["u"] is None else a["u"].astype(np.float64)
    q = 0.01
    y = np.full((T, B, ydim), np.nan)
    mean, var, cov, ll = er.ekf(s, C, b, y, u, q, 0.1, a["x0"], prior_logvar=a["lv0"], observed=np.zeros((T, B), np.uint8))
    x, P = a["x0"].astype(np.float64), np.exp(a["lv0"].astype(np.float64))[:, :, None] * np.eye(xdim)
    for t in range(T):
        g, A = fr.g_and_A(s, x, None if u is None else u[t])
        J = np.eye(xdim) + A
        x, P = x + g, J @ P @ np.swapaxes(J, 1, 2) + q * np.eye(xdim)
        close(mean[t], x, 1e-13, f"row {t} mean")
        close(cov[t], P, 1e-12, f"row {t} cov")
    assert (ll == 0).all()


@pytest.mark.parametrize("gaps", [False, True])
def test_chunks_chained_with_before_equal_the_undivided_run(gaps):
    name = "control"
    s, (C, b), a = ec.state(name), ec.decoder(name), ec.inputs(name)
    T = ec.CASES[name][5]
    obs = ec.observed(name) if gaps else None
    whole = er.ekf(s, C, b, a["y"], a["u"], a["q"], a["r"], a["x0"], prior_logvar=a["lv0"], observed=obs)
    parts, head = [], None
    for lo, hi in ((0, 1), (1, 17), (17, T)):
        kw = dict(prior_logvar=a["lv0"]) if head is None else dict(prior_cov=head[1])
        out = er.ekf(s, C, b, a["y"][lo:hi], a["u"][lo:hi], a["q"], a["r"], a["x0"] if head is None else head[0],
                     observed=None if obs is None else obs[lo:hi], **kw)
        head = (out[0][-1], out[2][-1])
        parts.append(out)
    for i, what in enumerate(ec.TENSORS):
        close(np.concatenate([p[i] for p in parts]), whole[i], 1e-12, what)


def test_poisoning_is_per_trial_and_from_the_row_on():
    name = "ragged3"
    s, (C, b), a = ec.state(name), ec.decoder(name), ec.inputs(name)
    clean = er.ekf(s, C, b, a["y"], a["u"], a["q"], a["r"], a["x0"], prior_logvar=a["lv0"])
    y = a["y"].copy()
    y[5, 3, 2] = np.nan
    out = er.ekf(s, C, b, y, a["u"], a["q"], a["r"], a["x0"], prior_logvar=a["lv0"])
    for got, ref in zip(out, clean):
        assert np.isnan(got[5:, 3]).all()
        np.testing.assert_array_equal(got[:5, 3], ref[:5, 3])
        np.testing.assert_array_equal(np.delete(got, 3, axis=1), np.delete(ref, 3, axis=1))
    # an indefinite prior covariance poisons from row 0
    P0 = np.exp(a["lv0"].astype(np.float64))[:, :, None] * np.eye(3)
    P0[1] = -P0[1]
    out = er.ekf(s, C, b, a["y"], a["u"], a["q"], a["r"], a["x0"], prior_cov=P0)
    for got, ref in zip(out, clean):
        assert np.isnan(got[:, 1]).all() and np.isfinite(np.delete(got, 1, axis=1)).all()
    # a NaN in a row that is not observed poisons nothing
    obs = ec.observed(name)
    y = a["y"].copy()
    y[obs == 0] = np.nan
    gap = er.ekf(s, C, b, y, a["u"], a["q"], a["r"], a["x0"], prior_logvar=a["lv0"], observed=obs)
    ref = er.ekf(s, C, b, a["y"], a["u"], a["q"], a["r"], a["x0"], prior_logvar=a["lv0"], observed=obs)
    for got, want in zip(gap, ref):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("regime", list(ec.REGIMES))
@pytest.mark.parametrize("name", list(ec.CASES))
def test_every_case_meets_the_conditions_of_the_rule(name, regime):
    """E <= 1e-4 scale and max|mean| < 100 (asserted by ec.bound), with and without the gap pattern; and the pattern has the gaps it
    is meant to have."""
    for gaps in (False, True):
        ref = ec.references(name, regime, gaps)
        for what in ec.TENSORS:
            assert ec.bound(what, *ref[what]) > 0
    o = ec.observed(name)
    T, B = o.shape
    assert o[0].min() == 0 and o[T - 1].min() == 0 and (o[:, 1] == 0).all() and o[:, 0].max() == 1
    assert ((o[2] == 0) & (o[3] == 0)).any()
    ref = ec.references(name, regime, True)["loglik"][0]
    assert (ref[o == 0] == 0).all() and (ref[o == 1] != 0).all()
