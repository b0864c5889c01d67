"""The reference of the `score_forecast` tests (tests/kstep_ref.py) checked on its own, without a GPU: against a plain double loop
over (t, b, h), against oracle.forecast with zero noise from each origin, on an affine map whose k-step error is known in closed
form, the stated summation order against numpy's own, and additivity over a split of the trials."""
import numpy as np
import pytest

from oracle import vjf_oracle as orc
from tests import kstep_cases as kc
from tests import kstep_ref as kr


def f64(st):
    return {k: np.asarray(v, np.float64) for k, v in st.items()}


def loop_score(st, mu, y, u, K, poisson):
    """The semantics, one (t, b, h) at a time."""
    T, B, dout = mu.shape
    dy = y.shape[-1]
    W, b_ = st["dec_W"], st["dec_b"]
    out = {k: np.zeros((K + 1, dout if k.endswith("x") else dy)) for k in ("sse_x", "base_x", "sse_y", "base_y")}
    pred = np.full((K, T, B, dout), np.nan)

    def term(eta, t):
        if poisson:
            ec = np.minimum(eta, 10.0)
            return np.exp(ec) - t * ec
        return (eta - t) ** 2
    for t in range(T):
        for b in range(B):
            xh = mu[t, b].copy()
            for h in range(0, K + 1):
                if t + h > T - 1:
                    break
                if h > 0:
                    xh = kr.mean_step(st, xh[None], None if u is None else u[t + h, b][None], np.float64)[0]
                    pred[h - 1, t, b] = xh
                out["sse_x"][h] += (xh - mu[t + h, b]) ** 2
                out["base_x"][h] += (mu[t, b] - mu[t + h, b]) ** 2
                out["sse_y"][h] += term(xh @ W.T + b_, y[t + h, b])
                out["base_y"][h] += term(mu[t, b] @ W.T + b_, y[t + h, b])
    out["pred"] = pred
    return out


@pytest.mark.parametrize("name", ["control", "short", "single", "poisson"])
def test_against_a_plain_loop(name):
    st, rec = f64(kc.state(name)), kc.record(name)
    mu, y = rec["mu"].astype(np.float64), rec["y"].astype(np.float64)
    u = None if rec["u"] is None else rec["u"].astype(np.float64)
    if name == "control":                                  # (the loop is slow: a corner of the case)
        mu, y, u = mu[:7, :5], y[:7, :5], u[:7, :5]
    want = loop_score(st, mu, y, u, kc.K, kc.is_poisson(name))
    T, B = mu.shape[:2]
    for ordered in (False, True):
        got = kr.score(st, mu, y, u, kc.K, poisson=kc.is_poisson(name), ordered=ordered)
        assert got["n"].tolist() == [max(T - h, 0) * B for h in range(kc.K + 1)]
        for k in ("sse_x", "base_x", "sse_y", "base_y"):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-11, atol=1e-12, err_msg=f"{name} {k} ordered={ordered}")
        np.testing.assert_array_equal(np.isnan(got["pred"]), np.isnan(want["pred"]))
        np.testing.assert_allclose(np.nan_to_num(got["pred"]), np.nan_to_num(want["pred"]), rtol=1e-12, atol=1e-13)
    assert (got["sse_x"][0] == 0).all()
    if name == "short":
        assert all((got[k][5:] == 0).all() for k in ("sse_x", "base_x", "sse_y", "base_y")) and np.isnan(got["pred"][4:]).all()


@pytest.mark.parametrize("name", ["control", "ragged3"])
def test_predictions_against_the_oracle_forecast_with_zero_noise(name):
    xdim, udim, n, ydim, B, T = kc.CASES[name]
    st, rec = f64(kc.state(name)), kc.record(name)
    s = orc.OracleState(ydim, xdim, udim, n, (1,), orc.GAUSSIAN)
    for k, v in st.items():
        setattr(s, k, v)
    mu = rec["mu"].astype(np.float64)
    u = None if rec["u"] is None else rec["u"].astype(np.float64)
    pred = kr.predictions(st, mu, u, kc.K)
    for t in range(T):
        steps = min(kc.K, T - 1 - t)
        assert np.isnan(pred[steps:, t]).all()
        if steps:
            x, _ = orc.forecast(s, mu[t], None if u is None else u[t + 1:t + 1 + steps], steps, np.zeros((steps, n, xdim)))
            np.testing.assert_allclose(pred[:steps, t], x[1:], rtol=1e-12, atol=1e-13)


def test_an_affine_map_has_the_closed_form():
    """One feature of enormous width is 1 everywhere: the map is x + w.  On the record mu[t] = a_b + t v the h-step error is h (w - v)
    for every pair, persistence's is -h v, and through the decoder W h (w - v) against y = decode(mu)."""
    T, B, K, xdim, ydim = 9, 5, 6, 2, 3
    r = np.random.default_rng(3)
    w, v = np.array([[0.3, -0.2]]), np.array([0.25, 0.1])
    st = {"centroid": np.zeros((1, xdim)), "logwidth": np.array([np.log(1e9)]), "w_mean": w, "dec_W": r.standard_normal((ydim, xdim)),
          "dec_b": r.standard_normal(ydim)}
    mu = r.standard_normal((1, B, xdim)) + np.arange(T)[:, None, None] * v
    y = mu @ st["dec_W"].T + st["dec_b"]
    for ordered in (False, True):
        got = kr.score(st, mu, y, None, K, ordered=ordered)
        h = np.arange(K + 1)[:, None]
        nn = got["n"][:, None]
        np.testing.assert_allclose(got["sse_x"], nn * h ** 2 * (w[0] - v) ** 2, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(got["base_x"], nn * h ** 2 * v ** 2, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(got["sse_y"], nn * h ** 2 * (st["dec_W"] @ (w[0] - v)) ** 2, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(got["base_y"], nn * h ** 2 * (st["dec_W"] @ v) ** 2, rtol=1e-9, atol=1e-11)


def test_the_stated_order_in_fp32_is_close_to_fp64_and_defined():
    name = "ragged3"
    r64, r32 = kc.references(name)
    for k in ("sse_x", "base_x", "sse_y", "base_y"):
        kc.bound(r64[k], r32[k])                           # (asserts the yardstick's conditions)
    rec, st = kc.record(name), kc.state(name)
    again = kr.score(st, rec["mu"], rec["y"], rec["u"], kc.K, dtype=np.float32, ordered=True)
    assert all(np.array_equal(again[k], r32[k]) for k in ("sse_x", "base_x", "sse_y", "base_y"))
    # sums_from_pred on the reference's own predictions is the reference's fold
    sse, base = kr.sums_from_pred(r32["pred"], rec["mu"], ordered=True)
    assert np.array_equal(sse, r32["sse_x"]) and np.array_equal(base, r32["base_x"])


def test_every_case_meets_the_conditions_of_the_rule():
    for name in kc.CASES:
        r64, r32 = kc.references(name)
        for k in ("sse_x", "base_x", "sse_y", "base_y"):
            u = kc.unit(name, k, r64["n"])
            assert kc.bound(r64[k] / u, r32[k] / u) > 0


def test_additivity_over_a_split_of_the_trials():
    name = "control"
    st, rec = f64(kc.state(name)), kc.record(name)
    mu, y, u = (rec[k].astype(np.float64) for k in ("mu", "y", "u"))
    whole = kr.score(st, mu, y, u, kc.K)
    a, b = kr.score(st, mu[:, :21], y[:, :21], u[:, :21], kc.K), kr.score(st, mu[:, 21:], y[:, 21:], u[:, 21:], kc.K)
    assert (a["n"] + b["n"]).tolist() == whole["n"].tolist()
    for k in ("sse_x", "base_x", "sse_y", "base_y"):
        np.testing.assert_allclose(a[k] + b[k], whole[k], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(np.concatenate([a["pred"], b["pred"]], 2), whole["pred"])
