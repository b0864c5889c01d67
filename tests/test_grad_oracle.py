"""The hand-derived backward passes of the test oracles (oracle.vjf_oracle.filter_step, tests/act_oracle.filter_step) against torch
autograd in fp64 (tests/autograd_ref.py), and both against gradients recorded from the reference before its clip
(tests/golden/g11_grads.npz, written by tests/golden/make_golden_grads.py).

Bound, per tensor:  max|hand - autograd| <= 1e-10 max|autograd|.  Both sides are fp64 and differ in the order of their sums only:
summation-order noise is some 1e-14 relative to the largest entry (2e-14 measured with gradients up to 67), any mistake in a
derivation is of order 1.
"""
import numpy as np
import pytest
from torch import nn

from oracle import vjf_oracle as orc
from tests import act_oracle as ao
from tests import autograd_ref as ag
from tests import goldenio as gio

RTOL = 1e-10
MEGA = dict(ydim=10, xdim=3, udim=2, n_rbf=40, hidden=(8,), likelihood="gaussian")            # tests/lifetime.FAMILIES["mega"]
MEGA_P = dict(ydim=12, xdim=5, udim=0, n_rbf=100, hidden=(20, 12), likelihood="poisson")      # ... ["mega_p"]
# nn.Module -> tests/act_oracle's (kind, p0, p1): the eight supported activations (vjf_amd.recognition.activation_code)
ACTS = {
    "Tanh": (nn.Tanh(), (ao.TANH, 0.0, 0.0)),
    "ReLU": (nn.ReLU(), (ao.RELU, 0.0, 0.0)),
    "LeakyReLU": (nn.LeakyReLU(0.2), (ao.LEAKY_RELU, 0.2, 0.0)),
    "ELU": (nn.ELU(0.5), (ao.ELU, 0.5, 0.0)),
    "Softplus": (nn.Softplus(beta=2.0, threshold=20.0), (ao.SOFTPLUS, 2.0, 20.0)),
    "Sigmoid": (nn.Sigmoid(), (ao.SIGMOID, 0.0, 0.0)),
    "Hardtanh": (nn.Hardtanh(-0.5, 0.5), (ao.HARDTANH, -0.5, 0.5)),
    "ReLU6": (nn.ReLU6(), (ao.HARDTANH, 0.0, 6.0)),
}


def assert_same(tag, hand, auto):
    assert sorted(hand) == sorted(auto), (tag, sorted(hand), sorted(auto))
    for k in sorted(auto):
        a = np.asarray(auto[k], np.float64)
        h = np.asarray(hand[k], np.float64).reshape(a.shape)
        err, scale = float(np.abs(h - a).max()), float(np.abs(a).max())
        assert err <= RTOL * scale, f"{tag} {k}: max|hand - autograd| = {err:.3e}, max|autograd| = {scale:.3e}"


def trained_state(shape, seed):
    """A state as a few steps leave it: non-zero RLS mean, a dense upper-triangular w_chol, non-trivial prior and variances."""
    r = np.random.default_rng(seed)
    s = orc.init_state(shape["ydim"], shape["xdim"], shape["udim"], shape["n_rbf"], shape["hidden"], shape["likelihood"], r)
    n = s.n_rbf
    s.w_mean = 0.1 * r.standard_normal((n, s.xdim))
    s.w_chol = np.triu(0.05 * r.standard_normal((n, n))) + 0.5 * np.eye(n)
    s.tr_logvar = np.asarray(-0.4)
    s.prior_mean, s.prior_logvar = 0.3 * r.standard_normal(s.xdim), 0.2 * r.standard_normal(s.xdim)
    return s


def data(s, B, seed, posterior=False):
    r = np.random.default_rng(seed)
    if s.likelihood == orc.POISSON:
        y = r.poisson(np.exp(0.5 * r.standard_normal((B, s.ydim)) - 0.5)).astype(np.float64)
    else:
        y = r.standard_normal((B, s.ydim))
    u = r.standard_normal((B, s.udim)) if s.udim else None
    mu_s, lv_s = (0.5 * r.standard_normal((B, s.xdim)), 0.3 * r.standard_normal((B, s.xdim))) if posterior else (None, None)
    return dict(y=y, u=u, mu_s=mu_s, lv_s=lv_s, eps_s=r.standard_normal((B, s.xdim)), eps_t=r.standard_normal((B, s.xdim)))


def hand(s, d, *, act=None, warm_up=False):
    """grads of the oracle's step (update=False: the gradient is taken before anything moves) on a copy of `s`"""
    c = s.clone()
    args = (d["y"], d["u"], d["mu_s"], d["lv_s"], d["eps_s"], d["eps_t"])
    if act is None:
        o = orc.filter_step(c, *args, sgd=True, update=False, warm_up=warm_up)
    else:
        o = ao.filter_step(c, act, *args, sgd=True, update=False, warm_up=warm_up)
    return ag.hand_gradients(o.grads, s), o


def auto(s, d, **kw):
    return ag.step(s, d["y"], d["u"], d["mu_s"], d["lv_s"], d["eps_s"], d["eps_t"], **kw)


@pytest.mark.parametrize("case", ["gaussian_control", "poisson_two_layers", "warm_up", "posterior", "poisson_warm_up_posterior"])
def test_oracle_backward_is_autograd(case):
    shape = MEGA_P if case.startswith("poisson") else MEGA
    s = trained_state(shape, 7)
    d = data(s, 37, 8, posterior="posterior" in case)
    wu = "warm_up" in case
    h, o = hand(s, d, warm_up=wu)
    a = auto(s, d, warm_up=wu)
    assert abs(o.loss - a.loss) <= 1e-12 * abs(a.loss)                      # (the same loss is differentiated)
    assert_same(case, h, a.grads)
    h2, _ = hand(s, d, act=ACTS["Tanh"][1], warm_up=wu)                     # act_oracle's copy of the step at Tanh
    assert_same(case + " act_oracle", h2, a.grads)


@pytest.mark.parametrize("name", sorted(ACTS))
@pytest.mark.parametrize("shape", [MEGA, MEGA_P], ids=["mega", "mega_p"])
def test_act_oracle_backward_is_autograd(shape, name):
    module, code = ACTS[name]
    s = trained_state(shape, 11)
    d = data(s, 37, 12, posterior=True)
    a = auto(s, d, activation=module)
    # every branch of the activation is taken, and no pre-activation sits on a kink (where the two derivatives may differ by convention)
    pre = np.concatenate([p.ravel() for p in a.pre])
    kinks = {"ReLU": [0.0], "LeakyReLU": [0.0], "ELU": [0.0], "Hardtanh": [-0.5, 0.5], "ReLU6": [0.0, 6.0]}.get(name, [])
    for kk in kinks:
        assert np.abs(pre - kk).min() > 1e-9
    if name in ("ReLU", "LeakyReLU", "ELU", "Hardtanh"):
        assert (pre < kinks[0]).any() and (pre > kinks[-1]).any()
    h, o = hand(s, d, act=code)
    assert abs(o.loss - a.loss) <= 1e-12 * abs(a.loss)
    assert_same(name, h, a.grads)


def test_relu6_upper_branch():
    """ReLU6's flat upper branch: hidden pre-activations pushed beyond 6 on purpose (the default initialisation never gets there)."""
    module, code = ACTS["ReLU6"]
    s = trained_state(MEGA, 13)
    s.rec_W[0] = s.rec_W[0] * 8.0
    d = data(s, 37, 14)
    a = auto(s, d, activation=module)
    pre = a.pre[0]
    assert (pre > 6.0).any() and (pre < 0.0).any() and ((pre > 0.0) & (pre < 6.0)).any() and np.abs(pre - 6.0).min() > 1e-9
    h, _ = hand(s, d, act=code)
    assert_same("ReLU6 upper", h, a.grads)


@pytest.mark.parametrize("which", ["oracle", "act_oracle"])
def test_dropped_dynamics_component(which):
    """A non-finite dynamics component is the constant 0 (vjf/model.py:141-142): w_chol scaled until the predictive variance
    overflows fp64, as test_nonfinite_component_is_dropped_like_the_reference does in fp32."""
    s = trained_state(MEGA, 15)
    s.w_chol = s.w_chol * 1e200
    d = data(s, 37, 16)
    h, o = hand(s, d, act=ACTS["Tanh"][1] if which == "act_oracle" else None)
    assert o.dyn == 0.0
    a = auto(s, d, drop={ag.DYNAMICS})
    assert_same("dropped dynamics", h, a.grads)
    full = auto(trained_state(MEGA, 15), d)                                  # (the dropped term does matter: the gradients differ)
    assert np.abs(full.grads["mean_W"] - a.grads["mean_W"]).max() > 1e-3


def test_poisson_clamp_gradient():
    """eta on both sides of the clamp at 10 (vjf/likelihood.py:60): beyond it the gradient is 0, not exp(10) - y."""
    s = trained_state(MEGA_P, 17)
    s.dec_W, s.dec_b = s.dec_W * 8.0, s.dec_b + 6.0
    d = data(s, 37, 18)
    a = auto(s, d)
    assert (a.eta > 10.0 + 1e-6).sum() >= 10 and (a.eta < 10.0 - 1e-6).sum() >= 10
    h, _ = hand(s, d)
    assert_same("poisson clamp", h, a.grads)


# ------------------------------------------------------------------ the reference's own gradients
def golden_cases():
    z = gio.load("g11_grads")
    out = []
    for i in range(int(z["count"])):
        meta = [int(v) for v in z[f"{i}.meta"]]
        B, dz, dy, du, n, wu = meta[:6]
        hidden = tuple(meta[6:])
        lik = str(z[f"{i}.lik"])
        g = lambda k: z[f"{i}.{k}"] if f"{i}.{k}" in z.files else None          # noqa: E731
        s = orc.OracleState(dy, dz, du, n, hidden, lik)
        for k in ("prior_mean", "prior_logvar", "lik_logvar", "tr_logvar", "centroid", "logwidth", "w_mean", "w_chol", "mean_W",
                  "lv_W", "lv_b", "dec_W", "dec_b"):
            setattr(s, k, g(k))
        s.rec_W = [g(f"rec_W{k}") for k in range(len(hidden))]
        s.rec_b = [g(f"rec_b{k}") for k in range(len(hidden))]
        d = dict(y=g("y"), u=g("u"), mu_s=g("mu_s"), lv_s=g("lv_s"), eps_s=g("eps")[0], eps_t=g("eps")[1])
        grads = {k: g("grad." + k) for k in ag.trainable_names(s)}
        out.append((i, s, d, bool(wu), grads))
    return out


def test_golden_file_is_what_the_issue_asks():
    cases = golden_cases()
    assert len(cases) == 4
    (_, s0, d0, w0, _), (_, s1, d1, w1, _), (_, s2, d2, w2, _), (_, s3, d3, w3, _) = cases
    assert all(a.dtype == np.float64 for _, s, d, _, gr in cases for a in list(gr.values()) + [s.centroid, d["y"], d["eps_s"]])
    assert all(d["y"].shape[0] <= 40 for _, _, d, _, _ in cases)
    assert d0["mu_s"] is None and d1["mu_s"] is not None and not w0 and not w1            # from the prior, then from a posterior
    assert np.abs(s1.w_mean).max() > 0 and np.abs(np.tril(s1.w_chol, -1)).max() == 0        # (an RLS update lies between them)
    assert w2 and not w3 and s3.likelihood == orc.POISSON
    eta = auto(s3, d3).eta
    assert (eta > 10.0 + 1e-6).sum() >= 10 and (eta < 10.0 - 1e-6).sum() >= 10             # eta on both sides of the clamp


@pytest.mark.parametrize("i", range(4))
def test_autograd_and_oracle_match_the_reference_gradients(i):
    _, s, d, wu, want = golden_cases()[i]
    a = auto(s, d, warm_up=wu)
    assert_same(f"g11 case {i} autograd", a.grads, want)
    h, _ = hand(s, d, warm_up=wu)
    assert_same(f"g11 case {i} oracle", h, want)
    h2, _ = hand(s, d, act=ACTS["Tanh"][1], warm_up=wu)
    assert_same(f"g11 case {i} act_oracle", h2, want)
