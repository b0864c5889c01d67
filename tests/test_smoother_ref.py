"""The smoother's reference tested on its own (tests/smoother_ref.py, tests/smoother_cases.py): no GPU, no library.

  1. rts_backward against the marginals of the dense joint posterior of a linear-Gaussian state-space model;
  2. the two forms of `smooth` agree in fp64;
  3. the yardstick's honesty conditions: the fp32 run of the information form lies within 1e-4 of scale of the fp64 run;
  4. chunked smoothing with `after` equals the undivided run exactly;
  5. a huge state noise returns the filtered moments."""
import numpy as np
import pytest

from tests import smoother_cases as sc
from tests import smoother_ref as sr

NAMES = list(sc.CASES)
KINDS = list(sc.KINDS)


def test_rts_backward_against_the_dense_joint_posterior():
    """x_0 ~ N(m0, P0), x_{t+1} = A x_t + b + N(0, Q), y_t = H x_t + N(0, R), T = 5, xdim = 3.  The joint posterior of (x_0 .. x_4) is
    Gaussian with a block-tridiagonal precision; its marginals are what a Kalman filter followed by rts_backward has to give."""
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
    # Kalman filter
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
    ms, Pss = sr.rts_backward(mus, Ps, [A @ mus[t] + b for t in range(T - 1)], [A] * (T - 1), Q)
    # the dense joint: precision Lam and linear term eta
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
    mean = Sig @ eta
    for t in range(T):
        np.testing.assert_allclose(ms[t], mean[blk(t)], rtol=0, atol=1e-10)
        np.testing.assert_allclose(Pss[t], Sig[blk(t), blk(t)], rtol=0, atol=1e-10)
    # diagonal filtered covariances given as vectors are the same thing as their full form
    diag = np.stack([np.diag(P) for P in Ps])
    a = sr.rts_backward(mus, diag, [A @ mus[t] + b for t in range(T - 1)], [A] * (T - 1), 0.2)
    f = sr.rts_backward(mus, np.stack([np.diag(v) for v in diag]), [A @ mus[t] + b for t in range(T - 1)], [A] * (T - 1), 0.2 * np.eye(d))
    np.testing.assert_allclose(a[0], f[0], rtol=0, atol=1e-13)
    np.testing.assert_allclose(a[1], f[1], rtol=0, atol=1e-13)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_the_two_forms_agree_in_fp64(name, kind):
    a = sc.inputs(name, kind)
    s64 = sc.state(name)
    c = lambda v: None if v is None else np.asarray(v, np.float64)          # noqa: E731
    info = sc.references(name, kind)
    text = sr.smooth(s64, c(a["mu"]), c(a["lv"]), c(a["u"]), sc.Q, form="textbook")
    for i, what in enumerate(("mean", "var", "cov")):
        ref = info[what][0]
        err = np.abs(text[i] - ref).max() / sc.scale_of(what, ref)
        assert err <= 1e-9, f"{name} {kind} {what}: the forms differ by {err:.2e} of scale"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_honesty_conditions_of_the_yardstick(name, kind):
    """E = max|ref32 - ref64| <= 1e-4 of scale per tensor and max|mean| < 100 (both asserted inside `bound`); the fp32 covariances are
    positive definite and the filtered sequence is not already the smoothed one."""
    ref = sc.references(name, kind)
    for what in ("mean", "var", "cov"):
        r64, r32 = ref[what]
        assert r32.dtype == np.float32 and r64.dtype == np.float64
        b = sc.bound(what, r64, r32)
        print(f"{name} {kind} {what}: scale {sc.scale_of(what, r64):.3e} E/scale {np.abs(r32 - r64).max() / sc.scale_of(what, r64):.2e} bound {b:.3e}")
    assert np.linalg.eigvalsh(ref["cov"][1].astype(np.float64)).min() > 0
    assert (ref["var"][0] > 0).all()
    if kind != "tiny":
        assert np.abs(ref["mean"][0] - sc.inputs(name, kind)["mu"]).max() > 1e-3


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["control", "ragged3", "scalar"])
def test_chunked_equals_undivided(name, dtype):
    a = sc.inputs(name, "typical")
    s = sc.state(name).cast(dtype) if dtype is np.float32 else sc.state(name)
    c = lambda v: None if v is None else np.asarray(v, dtype)          # noqa: E731
    mu, lv, u = c(a["mu"]), c(a["lv"]), c(a["u"])
    T = mu.shape[0]
    whole = sr.smooth(s, mu, lv, u, dtype(sc.Q))
    for k in (1, T // 2, T - 1):
        back = sr.smooth(s, mu[k:], lv[k:], None if u is None else u[k:], dtype(sc.Q))
        front = sr.smooth(s, mu[:k], lv[:k], None if u is None else u[:k + 1], dtype(sc.Q), after=(back[0][0], back[2][0]))
        for i in range(3):
            assert np.array_equal(np.concatenate([front[i], back[i]]), whole[i]), f"cut at {k}: tensor {i}"
    # only the lower triangle of the after-covariance counts
    back = sr.smooth(s, mu[2:], lv[2:], None if u is None else u[2:], dtype(sc.Q))
    junk = back[2][0] + np.triu(np.ones_like(back[2][0]), 1)
    front = sr.smooth(s, mu[:2], lv[:2], None if u is None else u[:3], dtype(sc.Q), after=(back[0][0], junk))
    assert np.array_equal(front[0], whole[0][:2]) and np.array_equal(front[2], whole[2][:2])


@pytest.mark.parametrize("name", ["control", "wide", "scalar"])
def test_a_huge_state_noise_returns_the_filtered_moments(name):
    a = sc.inputs(name, "typical")
    c = lambda v: None if v is None else np.asarray(v, np.float64)          # noqa: E731
    for form in ("information", "textbook"):
        mean, var, cov = sr.smooth(sc.state(name), c(a["mu"]), c(a["lv"]), c(a["u"]), 1e12, form=form)
        np.testing.assert_allclose(mean, c(a["mu"]), rtol=0, atol=1e-9)
        np.testing.assert_allclose(var, np.exp(c(a["lv"])), rtol=0, atol=1e-9)
        off = cov - var[..., None] * np.eye(var.shape[-1])
        assert np.abs(off).max() <= 1e-9
    # and the last row is the filtered one whatever the noise
    mean, var, cov = sr.smooth(sc.state(name), c(a["mu"]), c(a["lv"]), c(a["u"]), sc.Q)
    assert np.array_equal(mean[-1], c(a["mu"])[-1]) and np.array_equal(var[-1], np.exp(c(a["lv"])[-1]))
