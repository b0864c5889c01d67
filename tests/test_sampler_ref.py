"""The posterior-draw reference tested on its own (tests/sampler_ref.py, tests/sampler_cases.py): no GPU, no library.

  1. zero noise gives the smoother's mean;
  2. the unit-noise probe: one member without noise and T * xdim members with one unit entry each give a factor of the joint
     covariance, whose diagonal blocks are the smoother's covariances and whose lag-one blocks are G_t Ps_{t+1};
  3. sample_backward against the dense joint posterior of a linear-Gaussian state-space model: the whole covariance and the mean;
  4. chunked drawing with `after` equals the undivided run exactly;
  5. the yardstick's honesty conditions of tests/sampler_cases.py."""
import numpy as np
import pytest

from tests import sampler_cases as pc
from tests import sampler_ref as pr
from tests import smoother_cases as sc
from tests import smoother_ref as sr

NAMES = list(pc.CASES)
KINDS = list(pc.KINDS)
c64 = lambda v: None if v is None else np.asarray(v, np.float64)          # noqa: E731


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_zero_noise_gives_the_smoothed_mean(name, kind):
    a = pc.inputs(name, kind)
    ref = sc.references(name, kind)["mean"][0]
    x = pr.sample(pc.state(name), c64(a["mu"]), c64(a["lv"]), c64(a["u"]), pc.Q, np.zeros((2,) + a["mu"].shape))
    err = np.abs(x - ref[None]).max() / sc.scale_of("mean", ref)
    assert err <= 1e-12, f"{name} {kind}: zero-noise draw differs from the smoothed mean by {err:.2e} of scale"


def probe(T, B, d):
    """z (1 + T d, T, B, d): member 0 zero, member 1 + t d + j the unit vector e_j at row t."""
    z = np.zeros((1 + T * d, T, B, d))
    for t in range(T):
        for j in range(d):
            z[1 + t * d + j, t, :, j] = 1.0
    return z


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["scalar", "ragged3", "control"])
def test_unit_noise_probe_reproduces_the_smoothed_covariances(name, kind):
    """The draws are affine in the noise: x = m + Lam z, so Lam's columns are the differences from the zero-noise member and
    Lam Lam^T is the joint covariance.  Its diagonal blocks against smooth's cov and its lag-one blocks against G_t Ps_{t+1}, to 1e-9
    of scale -- the scale and the tolerance the smoother's reference tests use for its two forms."""
    T = 4
    a = pc.inputs(name, kind)
    s = pc.state(name)
    mu, lv, u = c64(a["mu"])[:T], c64(a["lv"])[:T], None if a["u"] is None else c64(a["u"])[:T]
    B, d = mu.shape[1:]
    x = pr.sample(s, mu, lv, u, pc.Q, probe(T, B, d))
    mean, var, cov = sr.smooth(s, mu, lv, u, pc.Q)
    assert np.abs(x[0] - mean).max() <= 1e-12 * sc.scale_of("mean", mean)
    Lam = np.moveaxis(x[1:] - x[:1], 0, -1)                      # (T, B, d, T d): row t's block of rows
    scale = sc.scale_of("cov", cov)
    for t in range(T):
        got = Lam[t] @ np.swapaxes(Lam[t], -1, -2)
        assert np.abs(got - cov[t]).max() <= 1e-9 * scale, f"{name} {kind}: row {t} block off by {np.abs(got - cov[t]).max() / scale:.2e}"
    # lag one: G_t from the contract's own definition, D J^T (J D J^T + q I)^-1
    mp, Js = sr.predictions(s, mu, u)
    for t in range(T - 1):
        D = np.exp(lv[t])[:, :, None] * np.eye(d)
        G = np.swapaxes(np.linalg.solve(Js[t] @ D @ np.swapaxes(Js[t], -1, -2) + pc.Q * np.eye(d), Js[t] @ D), -1, -2)
        want = G @ cov[t + 1]
        got = Lam[t] @ np.swapaxes(Lam[t + 1], -1, -2)
        assert np.abs(got - want).max() <= 1e-9 * scale, f"{name} {kind}: lag-one block {t} off by {np.abs(got - want).max() / scale:.2e}"


def test_sample_backward_against_the_dense_joint_posterior():
    """The linear-Gaussian model of tests/test_smoother_ref.py (T = 5, xdim = 3): a Kalman filter followed by sample_backward on the
    unit-noise probe gives a factor of the whole T d x T d posterior covariance, and the posterior mean at zero noise."""
    r = np.random.default_rng(11)
    T, d, dy = 5, 3, 2
    A = 0.8 * np.eye(d) + 0.2 * r.standard_normal((d, d))
    b = 0.3 * r.standard_normal(d)
    H = r.standard_normal((dy, d))
    sq = 0.4 * r.standard_normal((d, d))
    Q = sq @ sq.T + 0.05 * np.eye(d)
    R = np.diag(r.uniform(0.1, 0.3, dy))
    m0, P0 = r.standard_normal(d), np.diag(r.uniform(0.5, 1.5, d))
    y = r.standard_normal((T, dy))
    mus, Ps = [], []
    m, P = m0, P0
    for t in range(T):
        if t:
            m, P = A @ m + b, A @ P @ A.T + Q
        S = H @ P @ H.T + R
        K = P @ H.T @ np.linalg.inv(S)
        m, P = m + K @ (y[t] - H @ m), (np.eye(d) - K @ H) @ P
        mus.append(m)
        Ps.append(P)
    mus, Ps = np.stack(mus), np.stack(Ps)
    z = probe(T, 1, d)[:, :, 0]                                  # (1 + T d, T, d)
    x = pr.sample_backward(mus, Ps, [A @ mus[t] + b for t in range(T - 1)], [A] * (T - 1), Q, z)
    Lam, eta = np.zeros((T * d, T * d)), np.zeros(T * d)
    Qi, Ri, P0i = np.linalg.inv(Q), np.linalg.inv(R), np.linalg.inv(P0)
    blk = lambda t: slice(t * d, (t + 1) * d)      # noqa: E731
    Lam[blk(0), blk(0)] += P0i
    eta[blk(0)] += P0i @ m0
    for t in range(T):
        Lam[blk(t), blk(t)] += H.T @ Ri @ H
        eta[blk(t)] += H.T @ Ri @ y[t]
        if t:
            Lam[blk(t), blk(t)] += Qi
            Lam[blk(t - 1), blk(t - 1)] += A.T @ Qi @ A
            Lam[blk(t), blk(t - 1)] -= Qi @ A
            Lam[blk(t - 1), blk(t)] -= A.T @ Qi
            eta[blk(t)] += Qi @ b
            eta[blk(t - 1)] -= A.T @ Qi @ b
    Sig = np.linalg.inv(Lam)
    np.testing.assert_allclose(x[0].reshape(-1), Sig @ eta, rtol=0, atol=1e-10)
    F = (x[1:] - x[:1]).reshape(T * d, T * d).T                  # column k: the response to unit noise k
    np.testing.assert_allclose(F @ F.T, Sig, rtol=0, atol=1e-10)
    # chunks with `after`, and the marginals against rts_backward
    back = pr.sample_backward(mus[2:], Ps[2:], [A @ mus[t] + b for t in range(2, T - 1)], [A] * (T - 3), Q, z[:, 2:])
    front = pr.sample_backward(mus[:2], Ps[:2], [A @ mus[t] + b for t in range(2)], [A] * 2, Q, z[:, :2], after=back[:, 0])
    assert np.array_equal(np.concatenate([front, back], 1), x)
    ms, Pss = sr.rts_backward(mus, Ps, [A @ mus[t] + b for t in range(T - 1)], [A] * (T - 1), Q)
    np.testing.assert_allclose(x[0], ms, rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["control", "ragged3", "scalar", "x24"])
def test_chunked_equals_undivided(name, dtype):
    a, z = pc.inputs(name, "typical"), pc.noise(name).astype(dtype)
    s = pc.state(name).cast(dtype) if dtype is np.float32 else pc.state(name)
    c = lambda v: None if v is None else np.asarray(v, dtype)          # noqa: E731
    mu, lv, u = c(a["mu"]), c(a["lv"]), c(a["u"])
    T = mu.shape[0]
    whole = pr.sample(s, mu, lv, u, dtype(pc.Q), z)
    for k in (1, T // 2, T - 1):
        back = pr.sample(s, mu[k:], lv[k:], None if u is None else u[k:], dtype(pc.Q), z[:, k:])
        front = pr.sample(s, mu[:k], lv[:k], None if u is None else u[:k + 1], dtype(pc.Q), z[:, :k], after=back[:, 0])
        assert np.array_equal(np.concatenate([front, back], 1), whole), f"cut at {k}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_honesty_conditions_of_the_yardstick(name, kind):
    """E = max|ref32 - ref64| <= 1e-4 of scale and max|draw| < 1000 (both asserted inside `bound`); the shapes, and the draws are not
    the smoothed mean."""
    r64, r32 = pc.references(name, kind)
    xdim, udim, n, ydim, B, T = pc.CASES[name]
    assert r64.shape == (pc.MEMBERS[name], T, B, xdim) and r64.dtype == np.float64 and r32.dtype == np.float32
    b = pc.bound(r64, r32)
    scale = max(1.0, float(np.abs(r64).max()))
    print(f"{name} {kind}: S {pc.MEMBERS[name]} scale {scale:.3e} E/scale {np.abs(r32 - r64).max() / scale:.2e} bound {b:.3e}")
    if kind != "tiny":
        assert np.abs(r64 - sc.references(name, kind)["mean"][0][None]).max() > 1e-3
