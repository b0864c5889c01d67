"""Shared by tests/test_gpu_kstep.py and tests/test_kstep_ref.py: the cases of `score_forecast` (vjf_kstep_score), their synthetic
model state (tests.forecast_cases.synthetic_state), their records, the references (computed once per process and never modified)
and the comparison rule (tests.forecast_cases.bound).

The record of a case: mu[0] ~ N(0, 1), mu[t + 1] = f(mu[t], u[t + 1]) + 0.1 N(0, 1) with f the fp64 mean map, u ~ N(0, 1),
y = mu dec_W^T + dec_b + 0.1 N(0, 1); all stored as float32.  `poisson`: y are integer counts and dec_b is shifted so that the linear
predictor lies on both sides of the likelihood's clamp at 10 (asserted on the fp64 reference: terms on each side).

The rule:  max|got - ref64| <= F max(E, 8 eps32 max|ref64|),  E = max|ref32 - ref64|, ref32 the fp32 restatement with the stated
summation order (tests/kstep_ref.py, ordered=True); the yardstick's conditions max|ref64| < 100 and E <= 1e-4 max|ref64| are asserted
by `bound`.  The rule is homogeneous in the unit of the compared quantity; the Poisson sums (hundreds of terms of up to
exp(10) = 22026 each) are compared in ONE unit for all horizons, exp(10) n[0] -- the largest rate the clamp admits times the pairs of
horizon 0, `unit(name, key, n)` -- so that the range condition, written for states of order one, can be asserted on them at all: a
single scalar, so the achieved ratio is the raw sums'.  Every other case is compared as the raw sums."""
import math

import numpy as np
import torch

from tests import kstep_ref as kr
from tests.forecast_cases import EPS32, HIDDEN, bound, synthetic_state   # noqa: F401  (bound, EPS32: used by the tests)
from tests.helpers import model_arrays

K = 8
# (xdim, udim, n_rbf, ydim, B, T)
CASES = {
    "ragged3": (3, 0, 20, 7, 37, 12),          # tiles straddle origins, the last tile partial
    "control": (5, 2, 37, 21, 37, 12),         # u; n a multiple of neither 4 nor 16
    "wide": (17, 1, 70, 33, 18, 10),           # two output tiles, three y tiles
    "configB": (10, 0, 200, 50, 33, 10),       # configs[1]'s model dimensions
    "beyond256": (5, 0, 300, 7, 18, 10),       # the streamed form of the x step
    "single": (3, 0, 20, 7, 1, 40),            # one trial: tiles of 16 origins
    "short": (3, 0, 20, 7, 37, 5),             # ragged3's model with T = 5 < K: horizons 5 .. 8 are empty
    "poisson": (3, 0, 20, 7, 37, 12),          # ragged3's shape, integer counts, the clamp on both sides
}
_INDEX = {name: i for i, name in enumerate(CASES)}
_MODEL_OF = {"short": "ragged3"}               # (the model's seed)
# The state's seed per case, fixed: drawn until the fp64 reference ALONE met the yardstick's range condition max|ref64| < 100 (the
# persistence sums of a map that drifts fast exceed it with most seeds at these B and T); no output of the code under test was looked at.
_STATE_SEED = {name: 5400 + i for name, i in _INDEX.items()}
_STATE_SEED["configB"] = 5503
POISSON_SHIFT = 8.8                            # added to dec_b: the linear predictor straddles 10

# The committed factor of the rule: start at 4, commit at most twice the worst ratio achieved on the MI355X, never above 16
# (the policy of tests/forecast_cases.py).  Achieved on an MI355X (profiles/kstep_margins.json): the worst ratio is 0.447 (beyond256
# sse_x and sse_y, the streamed x step's 300 features per accumulator share), every other comparison is below 0.26.  F = 0.89 <= 2 * 0.447.
F = 0.89


def is_poisson(name):
    return name == "poisson"


def state(name):
    """{key: float32 array} of the transition and the decoder."""
    xdim, udim, n, ydim, B, T = CASES[name]
    st = synthetic_state(_STATE_SEED[_MODEL_OF.get(name, name)], xdim, udim, n, ydim)
    if is_poisson(name):
        st["dec_b"] = (st["dec_b"] + np.float32(POISSON_SHIFT)).astype(np.float32)
    return st


def make_model(vjf, name, **kw):
    xdim, udim, n, ydim, B, T = CASES[name]
    torch.manual_seed(5)
    m = vjf.VJF.make_model(ydim, xdim, udim, n, HIDDEN, likelihood="poisson" if is_poisson(name) else "gaussian", **kw)
    views = model_arrays(m)
    for k, a in state(name).items():
        views[k].copy_(torch.as_tensor(a).reshape(views[k].shape).to(views[k].device))
    return m


_REC, _REF = {}, {}


def record(name):
    """{mu (T,B,xdim), y (T,B,ydim), u (T,B,udim) or None} float32; do not modify."""
    if name not in _REC:
        xdim, udim, n, ydim, B, T = CASES[name]
        st = {k: np.asarray(v, np.float64) for k, v in state(name).items()}
        r = np.random.default_rng(6000 + _INDEX[name])
        u = r.standard_normal((T, B, udim)).astype(np.float32) if udim else None
        mu = np.empty((T, B, xdim))
        mu[0] = r.standard_normal((B, xdim))
        for t in range(T - 1):
            mu[t + 1] = kr.mean_step(st, mu[t], None if u is None else u[t + 1].astype(np.float64), np.float64) + 0.1 * r.standard_normal((B, xdim))
        eta = mu @ st["dec_W"].T + st["dec_b"]
        if is_poisson(name):
            y = r.poisson(3.0, size=eta.shape).astype(np.float32)
        else:
            y = (eta + 0.1 * r.standard_normal(eta.shape)).astype(np.float32)
        _REC[name] = {"mu": mu.astype(np.float32), "y": y, "u": u}
    return _REC[name]


def references(name):
    """(ref64, ref32): tests.kstep_ref.score in fp64 with numpy's sums, and in fp32 with the stated summation order."""
    if name not in _REF:
        rec, st = record(name), state(name)
        kw = dict(K=K, poisson=is_poisson(name))
        _REF[name] = (kr.score(st, rec["mu"], rec["y"], rec["u"], dtype=np.float64, **kw),
                      kr.score(st, rec["mu"], rec["y"], rec["u"], dtype=np.float32, ordered=True, **kw))
        if is_poisson(name):
            eta = rec["mu"].astype(np.float64) @ st["dec_W"].astype(np.float64).T + st["dec_b"].astype(np.float64)
            assert (eta > kr.ETA_MAX).any() and (eta < kr.ETA_MAX).any(), "the linear predictor has to lie on both sides of the clamp"
            p = _REF[name][0]["pred"][0, :-1].astype(np.float64) @ st["dec_W"].astype(np.float64).T + st["dec_b"].astype(np.float64)
            assert (p > kr.ETA_MAX).any() and (p < kr.ETA_MAX).any(), "so have the predictions'"
    return _REF[name]


def unit(name, key, n):
    """What a compared output is divided by before the rule is applied, one scalar: 1, or for the Poisson sums exp(10) n[0]."""
    if is_poisson(name) and key in ("sse_y", "base_y"):
        return math.exp(kr.ETA_MAX) * float(np.asarray(n)[0])
    return 1.0
