"""Shared by tests/test_gpu_forecast.py and tests/test_forecast_host.py: the synthetic, seeded model state and inputs of the
`forecast_sequence` parity cases, their oracles (computed once per process and never modified), and the comparison rule.

The rule (both files):  max|got - oracle_fp64| <= F * max(E, 8 eps_fp32 max|oracle_fp64|)  with  E = max|oracle_fp32 - oracle_fp64|
measured per case and per tensor -- the fp32 oracle does the same arithmetic in numpy's order, so E is what fp32 rounding alone moves
the roll-out by.  The conditions that keep the yardstick honest are asserted with it: max|oracle_fp64| < 100 and
E <= 1e-4 max|oracle_fp64|."""
import math

import numpy as np
import torch

from oracle import vjf_oracle as orc
from tests.helpers import load_oracle_state, model_arrays

# (xdim, udim, n_rbf, ydim, B, T): the smallest shapes at which each part of the kernels can go wrong
CASES = {
    "ragged3": (3, 0, 20, 7, 37, 40),        # three tiles of trials, the last with 5
    "control": (5, 2, 37, 21, 37, 40),       # control input; n a multiple of neither 4 nor 16
    "wide": (17, 1, 70, 33, 18, 24),         # two output tiles in xdim
    "configB": (10, 0, 200, 50, 33, 24),     # configs[1]'s model dimensions
    # n beyond what the roll-out kernels' register form of the x step covers (a wavefront's share of K is more than 16 MFMA steps once
    # n > 256): the planners have to take the streamed form there, and every feature counts
    "beyond256": (5, 0, 300, 7, 18, 24),
}
# seed offsets, fixed per case: a case added later does not move the draws of those before it
_INDEX = {"configB": 0, "control": 1, "ragged3": 2, "wide": 3, "beyond256": 100}
HIDDEN = [8]
EPS32 = float(np.finfo(np.float32).eps)
# The committed factor of the rule.  The issue: start at 4, commit at most twice the worst ratio achieved on the MI355X, never above
# 16.  Achieved on an MI355X (profiles/forecast_margins.json): the worst ratio is 2.95 (ragged3 without state noise: x 2.91, y 2.95 --
# 40 steps of a map that stretches a rounding difference, the fp32 oracle's own E being one draw of the same amplification); every
# other comparison is between 0.12 and 1.08.  F = 4 is within [2.95, 2 * 2.95].
# `beyond256` without state noise reaches 6.56 in x (y 6.43; with state noise 1.86 and 2.73, inside F): 300 features summed in one fp32
# accumulator per weight sample and per K share, then 24 steps of the same amplification with no noise to cover it.  Every feature is
# counted: test_gpu_tangent.py::test_final_state_against_forecast_sequence finds the tangent kernel's final x at this shape equal to
# this kernel's bit for bit, and that x lies 0.23 of its bound from fp64 (profiles/tangent_margins.json).  By the same policy the
# comparison without state noise of that case alone is held to 8 <= 2 * 6.56; everything else stays at 4.
F = 4.0
F_CASE = {("beyond256", False): 8.0}


def factor(name, state_noise):
    """The committed factor of the rule for a case, with or without state noise."""
    return F_CASE.get((name, bool(state_noise)), F)


def case_index(name):
    """The case's seed offset (state 1000 +, inputs 2000 +, the ensemble's draws 3000 +)."""
    return _INDEX[name]


def synthetic_state(seed, xdim, udim, n, ydim):
    """{fixture key: float32 array} of the transition and the decoder; everything else keeps its constructor value."""
    r = np.random.default_rng(seed)
    A = 0.3 * r.standard_normal((n, n))
    P = np.eye(n) + A @ A.T
    Lc = np.linalg.cholesky(P)
    st = {"centroid": r.uniform(-2, 2, (n, xdim + udim)), "logwidth": math.log(1.5) + 0.1 * r.standard_normal(n),
          "w_mean": 0.05 * r.standard_normal((n, xdim)), "w_chol": np.linalg.inv(Lc.T), "w_pchol": Lc, "w_precision": P,
          "tr_logvar": np.asarray(math.log(0.01)), "dec_W": 0.5 * r.standard_normal((ydim, xdim)), "dec_b": 0.1 * r.standard_normal(ydim)}
    return {k: np.asarray(v, np.float32) for k, v in st.items()}


def make_model(vjf, name, **kw):
    """A model of the case's shape with the synthetic state written into it (through tests.helpers.model_arrays)."""
    xdim, udim, n, ydim, B, T = CASES[name]
    torch.manual_seed(5)
    m = vjf.VJF.make_model(ydim, xdim, udim, n, HIDDEN, likelihood="gaussian", **kw)
    views = model_arrays(m)
    for k, a in synthetic_state(1000 + case_index(name), xdim, udim, n, ydim).items():
        views[k].copy_(torch.as_tensor(a).reshape(views[k].shape).to(views[k].device))
    return m


def inputs(name):
    """float32 arrays x0 (B,xdim), u (T,B,udim) or None, w_noise (T,n,xdim), state_noise (T,B,xdim), all ~ N(0,1)."""
    xdim, udim, n, ydim, B, T = CASES[name]
    r = np.random.default_rng(2000 + case_index(name))
    f = lambda *s: r.standard_normal(s).astype(np.float32)          # noqa: E731
    return {"x0": f(B, xdim), "u": f(T, B, udim) if udim else None, "w_noise": f(T, n, xdim), "state_noise": f(T, B, xdim)}


def oracles(model, x0, u, w_noise, state_noise):
    """(x64, y64), (x32, y32): oracle.forecast on fp64 / fp32 twins of the model's present state, on the same fp32 input values."""
    s64 = load_oracle_state(model, np.float64)
    out = []
    for s, dt in ((s64, np.float64), (s64.cast(np.float32), np.float32)):
        c = lambda a: None if a is None else np.asarray(a, dt)          # noqa: E731
        out.append(orc.forecast(s, c(x0), c(u), np.asarray(w_noise).shape[0], c(w_noise), c(state_noise)))
    return out[0], out[1]


def bound(ref64, other):
    """The rule's right-hand side without F, with the yardstick's conditions asserted: max(E, 8 eps max|ref64|)."""
    ref64, other = np.asarray(ref64, np.float64), np.asarray(other, np.float64).reshape(np.shape(ref64))
    scale = float(np.abs(ref64).max())
    E = float(np.abs(other - ref64).max())
    assert np.isfinite(ref64).all() and scale < 100, f"max|oracle_fp64| = {scale}"
    assert E <= 1e-4 * scale, f"E = {E:.3e} against max|oracle_fp64| = {scale:.3e}"
    return max(E, 8 * EPS32 * scale)
