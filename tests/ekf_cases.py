"""Shared by the extended-Kalman-filter tests (test_ekf_ref.py, test_ekf_host.py, test_gpu_ekf.py): the cases, their state, decoder
and records, their references (computed once per process and never modified) and the comparison rule.

The shapes are tests/smoother_cases.py's -- a ragged last tile, a control input, two output tiles in xdim, configs[1]'s dimensions,
n > 256, `x24` and `scalar` -- with its state (forecast_cases.synthetic_state, w_mean times 10) and that state's decoder.  The record of
a case: the prior is N(x0, 0.05 I) with the case's x0; the latent path starts at x0 + sqrt(0.05) N(0, 1), follows the mean map
(row t is reached with u[t]) plus sqrt(q) N(0, 1) per row, and y = C x + b + sqrt(r) N(0, 1), rounded to fp32.  Seeds are fixed per
case and regime.  Three regimes (r, q): typical (0.1, 0.01), sharp (1e-3, 0.01), vague (10, 1e-4).  `observed(name)` is the fixed gap
pattern: row 0 of every third trial, rows 2 and 3 of every fourth trial from trial 1, the last row of every fifth trial from trial 2, and
trial 1 never.

The rule, per tensor:  max|got - ref64| <= F * max(E, 8 eps_fp32 scale),  E = max|ref32 - ref64|, where ref32 is the same numpy
arithmetic in fp32 on the same fp32 values.  scale = max(1, max|ref64|) for the mean and max|ref64| for var, cov and loglik.  Asserted
with it: E <= 1e-4 scale, and max|mean| < 100.  Every case, regime and gap setting meets both on the CPU (test_ekf_ref.py asserts it);
the closest is `x24`, sharp, var and cov at E = 0.96e-4 scale: 24 states seen through 7 outputs at r = 1e-3 give M a condition number
near 1400, which fp32 carries into the directions that are not observed."""
import math

import numpy as np

from tests import ekf_ref as er
from tests import fixed_point_ref as fr
from tests import forecast_cases as fc
from tests import smoother_cases as sc

CASES = sc.CASES                         # (xdim, udim, n_rbf, ydim, B, T)
EPS32 = sc.EPS32
REGIMES = {"typical": (0.1, 0.01), "sharp": (1e-3, 0.01), "vague": (10.0, 1e-4)}        # (r, q)
_REGIME_SEED = {"typical": 0, "sharp": 300, "vague": 600}
PRIOR_VAR = 0.05
# The committed factor of the rule: start at 4, at most twice the worst ratio achieved on the MI355X, never above 16.  Achieved on an
# MI355X (profiles/ekf_margins.json): the worst ratio is 1.696 (x24, sharp: mean, with and without gaps -- xdim = 24 observed through
# ydim = 7 at r = 1e-3, where M has a condition number near 1400 and the fp32 reference's own E is 1.4e-5 of the scale), then 1.666 and
# 1.547 (x24, sharp: loglik), 1.477 (beyond256, vague, gaps: var and cov) and 1.462 (wide, vague: var and cov); every other
# comparison is under 1.46.  F = 3.3 <= 2 * 1.696.
F = 3.3

case_index = sc.case_index
state = sc.state
make_model = sc.make_model


def decoder(name, dtype=np.float64):
    """(C (ydim, xdim), b (ydim)) of the case: the synthetic state's decoder, what make_model writes into the model."""
    a = sc._synthetic(name)
    xdim, udim, n, ydim, B, T = sc.shape(name)
    return a["dec_W"].reshape(ydim, xdim).astype(dtype), a["dec_b"].reshape(ydim).astype(dtype)


def observed(name):
    """uint8 (T, B): the fixed gap pattern -- row 0, two consecutive rows, the last row, and one trial never observed."""
    xdim, udim, n, ydim, B, T = sc.shape(name)
    o = np.ones((T, B), np.uint8)
    o[0, 0::3] = 0
    o[2:4, 1::4] = 0
    o[T - 1, 2::5] = 0
    if B > 1:
        o[:, 1] = 0
    return o


_IN = {}


def inputs(name, regime="typical"):
    """float32 arrays y (T, B, ydim), u (T, B, udim) or None, x0 (B, xdim), lv0 (B, xdim) and the floats r, q: once per case and regime."""
    if (name, regime) not in _IN:
        xdim, udim, n, ydim, B, T = sc.shape(name)
        r, q = REGIMES[regime]
        if name in fc.CASES:
            a = fc.inputs(name)
            x0, u = a["x0"], a["u"]
        else:
            r0 = np.random.default_rng(2000 + case_index(name))
            x0 = r0.standard_normal((B, xdim)).astype(np.float32)
            u = r0.standard_normal((T, B, udim)).astype(np.float32) if udim else None
        s64 = state(name)
        C, b = decoder(name)
        g = np.random.default_rng(8000 + case_index(name) + _REGIME_SEED[regime])
        x = x0.astype(np.float64) + math.sqrt(PRIOR_VAR) * g.standard_normal((B, xdim))
        ys = []
        for t in range(T):
            x = x + fr.g_and_A(s64, x, None if u is None else u[t].astype(np.float64))[0] + math.sqrt(q) * g.standard_normal((B, xdim))
            ys.append(x @ C.T + b + math.sqrt(r) * g.standard_normal((B, ydim)))
        _IN[(name, regime)] = {"y": np.stack(ys).astype(np.float32), "u": u, "x0": x0,
                               "lv0": np.full((B, xdim), math.log(PRIOR_VAR), np.float32), "r": r, "q": q}
    return _IN[(name, regime)]


_REF = {}
TENSORS = ("mean", "var", "cov", "loglik")


def references(name, regime="typical", gaps=False):
    """{"mean" | "var" | "cov" | "loglik": (ref64, ref32)} of ekf_ref.ekf on the case's state: once per process."""
    key = (name, regime, bool(gaps))
    if key not in _REF:
        a = inputs(name, regime)
        s64 = state(name)
        obs = observed(name) if gaps else None
        out = []
        for s, dt in ((s64, np.float64), (s64.cast(np.float32), np.float32)):
            c = lambda v: None if v is None else np.asarray(v, dt)          # noqa: E731
            C, b = decoder(name, dt)
            out.append(er.ekf(s, C, b, c(a["y"]), c(a["u"]), a["q"], a["r"], c(a["x0"]), prior_logvar=c(a["lv0"]), observed=obs))
        _REF[key] = {k: (out[0][i], out[1][i]) for i, k in enumerate(TENSORS)}
    return _REF[key]


def scale_of(what, ref64):
    m = float(np.abs(np.asarray(ref64, np.float64)).max())
    return max(1.0, m) if what == "mean" else m


def bound(what, ref64, other):
    """The rule's right-hand side without F, with the yardstick's conditions asserted: max(E, 8 eps scale)."""
    ref64, other = np.asarray(ref64, np.float64), np.asarray(other, np.float64).reshape(np.shape(ref64))
    scale = scale_of(what, ref64)
    E = float(np.abs(other - ref64).max())
    assert np.isfinite(ref64).all() and (what != "mean" or float(np.abs(ref64).max()) < 100), f"max|ref64| = {np.abs(ref64).max()}"
    assert E <= 1e-4 * scale, f"{what}: E = {E:.3e} against scale {scale:.3e}"
    return max(E, 8 * EPS32 * scale)
