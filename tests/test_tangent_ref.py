"""The reference of the tangent-dynamics tests itself (tests/tangent_ref.py), on the CPU: its Jacobian against autograd, its summed
log-stretches against the log-determinants along the trajectory, its Gram-Schmidt pass against numpy's QR, and the conditions that keep
the GPU tests' yardstick (tests/tangent_cases.py) honest for every case and mode the GPU file uses."""
import numpy as np
import pytest
import torch

from tests import tangent_cases as tc
from tests import tangent_ref as tr


def mean_map_torch(s, u):
    c, lw, W = (torch.tensor(a, dtype=torch.float64) for a in (s.centroid, s.logwidth, s.w_mean))

    def f(x):                                             # one trial: x (xdim,)
        xu = x if u is None else torch.cat([x, torch.tensor(u, dtype=torch.float64)])
        d2 = ((xu[None, :] - c) ** 2).sum(1)
        return x + torch.exp(-0.5 * d2 / torch.exp(lw) ** 2) @ W
    return f


@pytest.mark.parametrize("name", ["ragged3", "control", "wide"])
def test_jacobian_against_autograd(name):
    """fp64, with (control, wide) and without (ragged3) a control input: 1e-12 of the largest entry (achieved: 3e-16)."""
    s = tc.state(name)
    a = tc.inputs(name)
    x0 = a["x0"][:5].astype(np.float64)
    u0 = None if a["u"] is None else a["u"][0, :5].astype(np.float64)
    J = tr.jacobian(s, x0, u0)
    assert J.shape == (5, x0.shape[1], x0.shape[1])
    for b in range(5):
        want = torch.autograd.functional.jacobian(mean_map_torch(s, None if u0 is None else u0[b]), torch.tensor(x0[b])).numpy()
        assert np.abs(want).max() > 0.5
        assert np.abs(J[b] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", ["ragged3", "control"])
def test_summed_log_stretches_are_the_log_determinants(name):
    """m = xdim: sum_v lsum[b, v] = sum_t log|det J_t| (|det R| of every interval is |det| of the interval's product of Jacobians).
    T = 40, qr_every = 3: 14 intervals, the last one step long.  Under 1e-10 (achieved: 4e-15)."""
    xdim, udim, n, ydim, B, T = tc.CASES[name]
    assert T == 40
    s = tc.state(name)
    a = tc.inputs(name)
    x, Q, hist, lsum = tr.rollout(s, a["x0"].astype(np.float64), None if a["u"] is None else a["u"].astype(np.float64), None, T, xdim, 3)
    assert hist.shape == (14, B, xdim) and lsum.shape == (B, xdim)
    np.testing.assert_allclose(hist.sum(0), lsum, rtol=0, atol=1e-13)
    want = tc.logdet_sum(s, a["x0"].astype(np.float64), None if a["u"] is None else a["u"].astype(np.float64), T)
    assert np.abs(want).max() > 0.1
    assert np.abs(lsum.sum(1) - want).max() < 1e-10
    np.testing.assert_allclose(x, tr.trajectory(s, a["x0"].astype(np.float64), a["u"], T)[-1], rtol=0, atol=0)


@pytest.mark.parametrize("name,m", [("ragged3", 3), ("control", 2), ("wide", 17), ("configB", 4)])
def test_gram_schmidt_against_numpy_qr(name, m):
    """The frame and log R_vv of one pass on the raw product of five steps against numpy.linalg.qr of that product with the signs
    fixed (R_vv > 0); Q^T Q = I to 1e-12."""
    xdim = tc.CASES[name][0]
    s = tc.state(name)
    a = tc.inputs(name)
    u = None if a["u"] is None else a["u"].astype(np.float64)
    _, V, hist, _ = tr.rollout(s, a["x0"].astype(np.float64), u, None, 5, m, 0)
    assert hist.shape[0] == 0
    Q, logr = tr.mgs(V)
    for b in range(V.shape[0]):
        q, r = np.linalg.qr(V[b])
        sg = np.sign(np.diag(r))
        np.testing.assert_allclose(Q[b], q * sg[None, :], rtol=0, atol=1e-11)
        np.testing.assert_allclose(logr[b], np.log(np.abs(np.diag(r))), rtol=0, atol=1e-12)
        assert np.abs(Q[b].T @ Q[b] - np.eye(m)).max() <= 1e-12
    # the roll-out with one interval of five steps is that pass
    _, Q5, hist5, lsum5 = tr.rollout(s, a["x0"].astype(np.float64), u, None, 5, m, 5)
    np.testing.assert_array_equal(Q5, Q)
    np.testing.assert_array_equal(hist5[0], logr)
    np.testing.assert_array_equal(lsum5, logr)


def test_split_horizon_and_no_step():
    """The reference continues from (x, Q, lsum) at an interval boundary with the bits of the undivided run; T = 0 orthonormalises
    the start once."""
    name = "control"
    xdim, udim, n, ydim, B, T = tc.CASES[name]
    s = tc.state(name, np.float32)
    a = tc.inputs(name)
    whole = tr.rollout(s, a["x0"], a["u"], None, T, 2, 4)
    head = tr.rollout(s, a["x0"], a["u"][:24], None, 24, 2, 4)
    tail = tr.rollout(s, head[0], a["u"][24:], head[1], T - 24, 2, 4, lsum0=head[3])
    for i in (0, 1, 3):
        np.testing.assert_array_equal(tail[i], whole[i])
    np.testing.assert_array_equal(np.concatenate([head[2], tail[2]]), whole[2])
    q0 = np.random.default_rng(0).standard_normal((B, xdim, 2)).astype(np.float32)
    x, Q, hist, lsum = tr.rollout(s, a["x0"], None, q0, 0, 2, 1)
    np.testing.assert_array_equal(x, a["x0"])
    Qw, lw = tr.mgs(q0)
    np.testing.assert_array_equal(Q, Qw)
    np.testing.assert_array_equal(lsum, lw)
    assert hist.shape == (0, B, 2)


@pytest.mark.parametrize("m,qr", tc.PARITY)
@pytest.mark.parametrize("name", list(tc.CASES))
def test_the_yardstick_of_the_parity_cases(name, m, qr):
    """`tc.bound` asserts max|ref64| < 100 and E <= 1e-4 max(1, max|ref64|) for each tensor; the fp32 reference alone stays well inside
    (E <= 6e-6 max(1, max|ref64|) was found), the exponents are of the size the cases were made for, and the log-determinant sum of
    the fp32 reference is as close."""
    xdim, udim, n, ydim, B, T = tc.CASES[name]
    mm = xdim if m is None else m
    s = tc.state(name)
    a = tc.inputs(name)
    refs = tc.references(s, a["x0"], a["u"], T, mm, qr)
    for k, (r64, r32) in refs.items():
        b = tc.bound(r64, r32)
        assert b <= 2e-5 * max(1.0, float(np.abs(r64).max())), (k, b)
    lam = refs["lsum"][0] / T
    assert 0.005 < np.abs(lam).max() < 0.5, np.abs(lam).max()
    assert refs["log_stretch"][0].shape == (-(-T // qr), B, mm)
