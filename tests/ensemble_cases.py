"""Shared by tests/test_gpu_ensemble.py and tests/test_ensemble_host.py: the `forecast_ensemble` parity cases.  The shapes, the
synthetic model state, the start and the control input are tests/forecast_cases.py's; this adds the seeded draws of S_MAX members and
the ensemble's references, built on `oracle.forecast` member by member (computed once per process and never modified):

    fp64   np.mean / np.var over the members of the fp64 roll-outs and of their decoded y
    fp32   the fp32 oracle's roll-outs folded in member order by Welford's recurrence in np.float32, as the kernel folds them:
           mean_k = mean_{k-1} + (v - mean_{k-1}) / k,  M2 += (v - mean_{k-1}) (v - mean_k),  var = M2 / S

The rule is the forecast suite's, per case and per tensor (x_mean, x_var, y_mean, y_var):
    max|got - ref64| <= F * max(E, 8 eps_fp32 max|ref64|),  E = max|ref32 - ref64|
with `fc.bound`'s conditions asserted (max|ref64| < 100, E <= 1e-4 max|ref64|)."""
import math

import numpy as np

from tests import forecast_cases as fc

CASES = fc.CASES
S_MAX = 8
LOGVAR0 = math.log(0.04)                 # the Gaussian start's log variance (sd 0.2), every element
MODES = ("quiet", "noisy", "gaussian")   # no state noise / state noise / a Gaussian start (mean fc.inputs' x0), no state noise
TENSORS = ("x_mean", "x_var", "y_mean", "y_var")
# The committed factor of the rule.  The issue: start at 4, commit at most twice the worst ratio achieved on the MI355X, never above
# 16.  Achieved on an MI355X (profiles/ensemble_margins.json, 60 comparisons): the worst ratio is 3.43 (ragged3, S = 8, state noise:
# y_var 3.43, x_var 3.03, x_mean 2.16 -- the case whose single roll-out is the forecast suite's worst too); every other case is below
# 1.8.  F = 4 is within [3.43, 2 * 3.43].
F = 4.0


def noises(name):
    """float32 w_noise (S_MAX, T, n, xdim), state_noise (S_MAX, T, B, xdim), x0_noise (S_MAX, B, xdim), all ~ N(0, 1); an ensemble of
    S < S_MAX members takes the first S of each."""
    xdim, udim, n, ydim, B, T = CASES[name]
    r = np.random.default_rng(3000 + fc.case_index(name))
    f = lambda *s: r.standard_normal(s).astype(np.float32)          # noqa: E731
    return {"w_noise": f(S_MAX, T, n, xdim), "state_noise": f(S_MAX, T, B, xdim), "x0_noise": f(S_MAX, B, xdim)}


def welford32(members):
    """(mean, var) over axis 0 by the kernel's recurrence in np.float32."""
    members = np.asarray(members, np.float32)
    mean, m2 = np.zeros(members.shape[1:], np.float32), np.zeros(members.shape[1:], np.float32)
    for k, v in enumerate(members, 1):
        delta = v - mean
        mean = mean + delta / np.float32(k)
        m2 = m2 + delta * (v - mean)
    return mean, m2 / np.float32(len(members))


_REFS = {}


def references(model, name, S, mode):
    """{tensor: (ref64, ref32)} for the case, the first S members and the mode, plus "x": (members64, members32) (S, T + 1, B, xdim)."""
    key = (name, S, mode)
    if key not in _REFS:
        a, z = fc.inputs(name), noises(name)
        T = CASES[name][5]
        xs, ys = {}, {}
        for dt in (np.float64, np.float32):
            mx, my = [], []
            for s in range(S):
                x0 = a["x0"].astype(dt)
                if mode == "gaussian":
                    x0 = x0 + z["x0_noise"][s].astype(dt) * np.exp(dt(0.5) * dt(LOGVAR0))
                pair = fc.oracles(model, x0, a["u"], z["w_noise"][s], z["state_noise"][s] if mode == "noisy" else None)
                x, y = pair[0] if dt is np.float64 else pair[1]
                mx.append(x)
                my.append(y)
            xs[dt], ys[dt] = np.stack(mx), np.stack(my)
            assert xs[dt].shape == (S, T + 1) + a["x0"].shape and xs[dt].dtype == dt
        xm32, xv32 = welford32(xs[np.float32])
        ym32, yv32 = welford32(ys[np.float32])
        _REFS[key] = {"x_mean": (xs[np.float64].mean(0), xm32), "x_var": (xs[np.float64].var(0), xv32),
                      "y_mean": (ys[np.float64].mean(0), ym32), "y_var": (ys[np.float64].var(0), yv32),
                      "x": (xs[np.float64], xs[np.float32])}
        for v in _REFS[key].values():
            for r in v:
                r.setflags(write=False)
    return _REFS[key]
