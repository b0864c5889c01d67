"""Shared by the Poisson-filter tests (test_laplace_ref.py, test_laplace_host.py, test_gpu_laplace.py): the cases, their state,
decoder and records, their references (computed once per process and never modified) and the comparison rule.

The shapes are tests/ekf_cases.py's (tests/smoother_cases.py's: a ragged last tile, a control input, two output tiles in xdim,
configs[1]'s dimensions, n > 256, `x24` and `scalar`), with its state, its prior N(x0, 0.05 I) and its `observed` pattern.  A regime
(gain, offset) scales and shifts the case's decoder, C' = gain C and b' = gain b + offset, written into a Poisson model:
sparse (0.5, -1.5), typical (0.5, +0.5), busy (0.3, +3.0).  The latent path is ekf_cases' with q = 0.01: it starts at
x0 + sqrt(0.05) N(0, 1) and follows the mean map (row t is reached with u[t]) plus sqrt(q) N(0, 1) per row; the counts are drawn
Poisson(exp(min(eta, 8))) from seeds fixed per case and regime.

The rule, per tensor:  max|got - ref64| <= F * max(E, 8 eps_fp32 scale),  E = max|ref32 - ref64|, where ref32 is the same numpy
arithmetic in fp32 on the same fp32 values.  scale = max(1, max|ref64|) for the mean and max|ref64| for var, cov and loglik; grad_norm
is compared on the scale of the gradient's own terms, max(1, max|C'^T y|) -- the fp64 value is near 1e-6 and the
fp32 one is the cancellation in C^T (y - lam).  Asserted with it on the CPU: E <= 1e-3 scale, max|mean| < 100, the fp64 grad_norm
<= 1e-5 at n_iter = 8, and n_iter = 8 against n_iter = 30 within 1e-7 scale in fp64 (test_laplace_ref.py)."""
import math

import numpy as np
import torch

from tests import ekf_cases as ec
from tests import fixed_point_ref as fr
from tests import forecast_cases as fc
from tests import laplace_ref as lr
from tests import smoother_cases as sc
from tests.helpers import model_arrays

CASES = ec.CASES                         # (xdim, udim, n_rbf, ydim, B, T)
EPS32 = ec.EPS32
REGIMES = {"sparse": (0.5, -1.5), "typical": (0.5, 0.5), "busy": (0.3, 3.0)}        # (gain, offset)
_REGIME_SEED = {"sparse": 0, "typical": 300, "busy": 600}
PRIOR_VAR = ec.PRIOR_VAR
Q = 0.01
N_ITER = 8
ETA_CAP = 8.0                            # of the draw of the counts only
# The committed factor of the rule: start at 4, at most twice the worst ratio achieved on the MI355X, never above 16.  Achieved on an
# MI355X (profiles/laplace_margins.json): over the 210 parity comparisons the worst ratio is 0.71 (wide, typical, gaps: var and cov),
# then 0.57 (configB, typical, gaps: var and cov); mean, loglik and grad_norm stay under 0.27.  Over the module's other comparisons by
# the rule the worst is 1.907 (control, busy, n_iter = 1: loglik -- one step from the prediction), then 0.65 (ydim = 1: var and cov).  F = 3.8 <= 2 * 1.907.
F = 3.8
TENSORS = ("mean", "var", "cov", "loglik", "grad_norm")

case_index = ec.case_index
state = ec.state
observed = ec.observed


def decoder(name, regime="typical", dtype=np.float64):
    """(C' (ydim, xdim), b' (ydim)) of the case under the regime: fp32 values (what make_model writes into the model) in `dtype`."""
    gain, offset = REGIMES[regime]
    C, b = ec.decoder(name, np.float64)
    return (gain * C).astype(np.float32).astype(dtype), (gain * b + offset).astype(np.float32).astype(dtype)


def make_model(vjf, name, regime="typical", **kw):
    """A Poisson model of the case's shape with the case's state and the regime's decoder written into it."""
    xdim, udim, n, ydim, B, T = sc.shape(name)
    torch.manual_seed(5)
    m = vjf.VJF.make_model(ydim, xdim, udim, n, fc.HIDDEN, likelihood="poisson", **kw)
    views = model_arrays(m)
    s = state(name, np.float32)
    C, b = decoder(name, regime, np.float32)
    for k, a in (("centroid", s.centroid), ("logwidth", s.logwidth), ("w_mean", s.w_mean), ("dec_W", C), ("dec_b", b)):
        views[k].copy_(torch.as_tensor(np.ascontiguousarray(a, np.float32)).reshape(views[k].shape).to(views[k].device))
    return m


def state_of(m):
    """(OracleState with the model's centroid, logwidth and w_mean, C (ydim, xdim), b (ydim)) in fp64: what the reference takes."""
    from oracle import vjf_oracle as orc
    vel = m.transition.velocity
    n, d = vel.feature.centroid.shape
    s = orc.OracleState(1, vel.n_output, d - vel.n_output, n, (1,), orc.GAUSSIAN)
    g = lambda t: t.detach().cpu().numpy().astype(np.float64)      # noqa: E731
    s.centroid, s.logwidth, s.w_mean = g(vel.feature.centroid), g(vel.feature.logwidth), g(vel.w_mean).reshape(n, vel.n_output)
    return s, g(m.decoder.decode.weight), g(m.decoder.decode.bias)


_IN = {}


def inputs(name, regime="typical"):
    """float32 arrays y (T, B, ydim) of counts, u (T, B, udim) or None, x0 (B, xdim), lv0 (B, xdim) and the float q: once per case
    and regime."""
    if (name, regime) not in _IN:
        xdim, udim, n, ydim, B, T = sc.shape(name)
        a = ec.inputs(name, "typical")                 # x0, u and lv0 are the case's, whatever the regime
        x0, u = a["x0"], a["u"]
        s64 = state(name)
        C, b = decoder(name, regime)
        g = np.random.default_rng(9000 + case_index(name) + _REGIME_SEED[regime])
        x = x0.astype(np.float64) + math.sqrt(PRIOR_VAR) * g.standard_normal((B, xdim))
        ys = []
        for t in range(T):
            x = x + fr.g_and_A(s64, x, None if u is None else u[t].astype(np.float64))[0] + math.sqrt(Q) * g.standard_normal((B, xdim))
            ys.append(g.poisson(np.exp(np.minimum(x @ C.T + b, ETA_CAP))))
        _IN[(name, regime)] = {"y": np.stack(ys).astype(np.float32), "u": u, "x0": x0, "lv0": a["lv0"], "q": Q}
    return _IN[(name, regime)]


def run_reference(name, regime, gaps, dt, n_iter=N_ITER):
    """laplace_ref.laplace_filter on the case in the dtype `dt`: (mean, var, cov, loglik, grad_norm)."""
    a = inputs(name, regime)
    s = state(name) if dt == np.float64 else state(name).cast(np.float32)
    c = lambda v: None if v is None else np.asarray(v, dt)          # noqa: E731
    C, b = decoder(name, regime, dt)
    return lr.laplace_filter(s, C, b, c(a["y"]), c(a["u"]), a["q"], c(a["x0"]), prior_logvar=c(a["lv0"]),
                             observed=observed(name) if gaps else None, n_iter=n_iter)


_REF = {}


def references(name, regime="typical", gaps=False):
    """{tensor: (ref64, ref32)} of laplace_ref.laplace_filter at n_iter = 8 on the case's state: once per process."""
    key = (name, regime, bool(gaps))
    if key not in _REF:
        out = [run_reference(name, regime, gaps, dt) for dt in (np.float64, np.float32)]
        _REF[key] = {k: (out[0][i], out[1][i]) for i, k in enumerate(TENSORS)}
    return _REF[key]


def grad_scale(name, regime, ref32):
    """The scale grad_norm is compared on: the size of the terms that cancel in grad = z - Lp^T C^T (y - lam)."""
    C, _ = decoder(name, regime)
    y = inputs(name, regime)["y"].astype(np.float64)
    return max(1.0, float(np.abs(y @ C).max()))


def scale_of(what, ref64, name=None, regime=None, other=None):
    if what == "grad_norm":
        return grad_scale(name, regime, other)
    m = float(np.abs(np.asarray(ref64, np.float64)).max())
    return max(1.0, m) if what == "mean" else m


def bound(what, ref64, other, name=None, regime=None):
    """The rule's right-hand side without F, with the yardstick's conditions asserted: max(E, 8 eps scale)."""
    ref64, other = np.asarray(ref64, np.float64), np.asarray(other, np.float64).reshape(np.shape(ref64))
    scale = scale_of(what, ref64, name, regime, other)
    E = float(np.abs(other - ref64).max())
    assert np.isfinite(ref64).all() and (what != "mean" or float(np.abs(ref64).max()) < 100), f"max|ref64| = {np.abs(ref64).max()}"
    assert E <= 1e-3 * scale, f"{what}: E = {E:.3e} against scale {scale:.3e}"
    return max(E, 8 * EPS32 * scale)


def lds_floats(n, d, dout, dy, vg, cl, dl):
    """The floats of dynamic LDS of vjf_laplace_kernel as DESIGN.md section 3 "Laplace filter" adds them up."""
    LD, NW = 17, 4
    doutp, dyp, ntri = (dout + 15) // 16 * 16, (dy + 15) // 16 * 16, dout * (dout + 1) // 2
    x_step = n * LD + d * LD + NW * doutp * LD + n + (n * d if cl else 0)
    own = n + 7 * dout * LD + dout * dout * LD + 3 * ntri * LD + NW * vg * doutp * LD + (n * dout if cl else 0) + 16 * LD + LD
    dec = dout * ((dy + 31) // 32 * 32 + 16) + dyp * (16 if dout <= 16 else 48) if dl else 0
    return x_step + own + dec
