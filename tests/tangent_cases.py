"""Shared by the tangent-dynamics tests (test_tangent_ref.py, test_tangent_host.py, test_gpu_tangent.py): the cases, their state and
inputs, their references (computed once per process and never modified) and the comparison rule.

The cases are tests/forecast_cases.py's shapes, seeded state and inputs with w_mean multiplied by 10 (entries 0.5 N(0, 1)): the
forecast cases' own state is so close to the identity map that every stretch is log(1 + eps); the stiffer one gives exponents of
+-0.02 .. 0.2 per step.

The rule, per tensor:  max|got - ref64| <= F * max(E, 8 eps_fp32 max(1, max|ref64|)),  E = max|ref32 - ref64|, where ref32 is the
same numpy arithmetic in fp32 on the same fp32 values -- what fp32 rounding alone moves the result by.  The floor at 1: a log-stretch
near 0 carries the absolute rounding of a norm near 1.  Asserted with it: max|ref64| < 100 and E <= 1e-4 max(1, max|ref64|)."""
import numpy as np
import torch

from oracle import vjf_oracle as orc
from tests import forecast_cases as fc
from tests import tangent_ref as tr
from tests.helpers import load_oracle_state, model_arrays

CASES = fc.CASES                         # (xdim, udim, n_rbf, ydim, B, T); `beyond256`: the x step's streamed form is the only right one
EPS32 = fc.EPS32
W_SCALE = 10.0
# (m, qr_every) of the parity test; m = None: xdim.  (None, 3) ends with a ragged interval (T = 40: 13 x 3 + 1; T = 24: a whole one)
PARITY = [(None, 1), (2, 4), (None, 3)]
# The committed factor of the rule: start at 4, at most twice the worst ratio achieved on the MI355X, never above 16.  Achieved
# (profiles/tangent_margins.json): the worst ratio is 1.159 (beyond256, m = 2, qr_every = 4, the frame q -- 24 steps of a map that
# stretches a rounding difference, the fp32 reference's own E being one draw of the same amplification); four more comparisons of q
# are between 0.88 and 1.16, every other comparison is under 0.95.  F = 2.3 <= 2 * 1.159.
F = 2.3


case_index = fc.case_index


def state(name, dtype=np.float64):
    """OracleState of the case without a model: only what the mean map reads (centroid, logwidth, w_mean) is set."""
    xdim, udim, n, ydim, B, T = CASES[name]
    a = fc.synthetic_state(1000 + case_index(name), xdim, udim, n, ydim)
    s = orc.OracleState(ydim, xdim, udim, n, tuple(fc.HIDDEN), orc.GAUSSIAN)
    s.centroid, s.logwidth = a["centroid"].astype(dtype), a["logwidth"].astype(dtype)
    s.w_mean = (a["w_mean"] * np.float32(W_SCALE)).astype(dtype)         # (the fp32 product, as make_model forms it)
    return s


def make_model(vjf, name, **kw):
    """A model of the case's shape with forecast_cases' synthetic state written into it (as forecast_cases.make_model does), w_mean
    times W_SCALE."""
    xdim, udim, n, ydim, B, T = CASES[name]
    torch.manual_seed(5)
    m = vjf.VJF.make_model(ydim, xdim, udim, n, fc.HIDDEN, likelihood="gaussian", **kw)
    views = model_arrays(m)
    for k, a in fc.synthetic_state(1000 + case_index(name), xdim, udim, n, ydim).items():
        views[k].copy_(torch.as_tensor(a).reshape(views[k].shape).to(views[k].device))
    views["w_mean"].mul_(W_SCALE)
    return m


def inputs(name):
    """float32 arrays x0 (B, xdim), u (T, B, udim) or None, ~ N(0, 1): forecast_cases' own draws."""
    a = fc.inputs(name)
    return {"x0": a["x0"], "u": a["u"]}


def references(s64, x0, u, T, m, qr_every, q0=None, lsum0=None):
    """{tensor: (ref64, ref32)} for x, q, log_stretch, lsum of tangent_ref.rollout on an fp64 state and its fp32 twin, same fp32 inputs."""
    out = []
    for s, dt in ((s64, np.float64), (s64.cast(np.float32), np.float32)):
        c = lambda a: None if a is None else np.asarray(a, dt)          # noqa: E731
        out.append(tr.rollout(s, c(x0), c(u), c(q0), T, m, qr_every, c(lsum0)))
    return {k: (out[0][i], out[1][i]) for i, k in enumerate(("x", "q", "log_stretch", "lsum"))}


def model_state(model):
    return load_oracle_state(model, np.float64)


def bound(ref64, other):
    """The rule's right-hand side without F, with the yardstick's conditions asserted: max(E, 8 eps max(1, max|ref64|))."""
    ref64, other = np.asarray(ref64, np.float64), np.asarray(other, np.float64).reshape(np.shape(ref64))
    scale = max(1.0, float(np.abs(ref64).max()))
    E = float(np.abs(other - ref64).max())
    assert np.isfinite(ref64).all() and scale < 100, f"max|ref64| = {scale}"
    assert E <= 1e-4 * scale, f"E = {E:.3e} against max(1, max|ref64|) = {scale:.3e}"
    return max(E, 8 * EPS32 * scale)


def logdet_sum(s, x0, u, T):
    """sum_t log|det J(x_t, u_t)| per trial (B,) along the mean map's trajectory, in the state's dtype."""
    xs = tr.trajectory(s, x0, u, T)
    tot = np.zeros(xs.shape[1], s.dtype)
    for t in range(T):
        J = tr.jacobian(s, xs[t], None if u is None else np.asarray(u[t], s.dtype))
        tot = tot + np.linalg.slogdet(J)[1].astype(s.dtype)
    return tot
