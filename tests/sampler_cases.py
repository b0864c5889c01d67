"""Shared by the posterior-draw tests (test_sampler_ref.py, test_sampler_host.py, test_gpu_sampler.py): tests/smoother_cases.py's
cases, states, filtered sequences, kinds and state-noise variance, plus the noise, the references (computed once per process and never
modified) and the comparison rule.

Noise: default_rng(8000 + case_index) standard normal, fp32, (S, T, B, xdim); S per case from {1, 5, 17, 33}, so the sixteen-lane member
split of the kernel meets one member, a remainder, and two and three rounds.

The rule is smoother_cases' rule on the draws:  max|got - ref64| <= F * max(E, 8 eps_fp32 scale),  E = max|ref32 - ref64|, where ref32 is
the same numpy arithmetic in fp32 on the same fp32 values and scale = max(1, max|ref64|).  Asserted with it: E <= 1e-4 scale, and a
bound of the draws' own, max|ref64| < 1000 (the `mixed` kind has sd up to e^3: `scalar` reaches 154)."""
import numpy as np

from tests import sampler_ref as pr
from tests import smoother_cases as sc

CASES, KINDS, Q, EPS32 = sc.CASES, sc.KINDS, sc.Q, sc.EPS32
state, make_model, inputs, case_index = sc.state, sc.make_model, sc.inputs, sc.case_index
MEMBERS = {"ragged3": 17, "control": 5, "wide": 5, "configB": 17, "beyond256": 5, "x24": 33, "scalar": 1}
assert set(MEMBERS) == set(CASES)
EXTRA_MEMBERS = {}                       # S of the shapes registered in smoother_cases.EXTRA
# The committed factor of the rule: start at 4, at most twice the worst ratio achieved on the MI355X, never above 16.  Achieved on an
# MI355X (profiles/sampler_margins.json has every comparison): the worst ratio is 0.390 (configB, mixed), then 0.309 (control, mixed),
# 0.270 (x24, mixed) and 0.201 (ragged3, typical); the edge sizes (T = 1, T = 2, S = 1) are under 0.20.  F = 0.78 = 2 * 0.390.
F = 0.78


def noise(name):
    """(S, T, B, xdim) fp32 standard-normal values of the case: the same for every kind."""
    xdim, udim, n, ydim, B, T = sc.shape(name)
    S = MEMBERS[name] if name in MEMBERS else EXTRA_MEMBERS[name]
    return np.random.default_rng(8000 + case_index(name)).standard_normal((S, T, B, xdim)).astype(np.float32)


_REF = {}


def references(name, kind="typical"):
    """(ref64, ref32) of sampler_ref.sample on the case's state, inputs and noise: once per process."""
    if (name, kind) not in _REF:
        a, z = inputs(name, kind), noise(name)
        s64 = state(name)
        out = []
        for s, dt in ((s64, np.float64), (s64.cast(np.float32), np.float32)):
            c = lambda v: None if v is None else np.asarray(v, dt)          # noqa: E731
            out.append(pr.sample(s, c(a["mu"]), c(a["lv"]), c(a["u"]), dt(Q), c(z)))
        _REF[(name, kind)] = tuple(out)
    return _REF[(name, kind)]


def bound(ref64, other):
    """The rule's right-hand side without F, with the yardstick's conditions asserted: max(E, 8 eps scale)."""
    ref64, other = np.asarray(ref64, np.float64), np.asarray(other, np.float64).reshape(np.shape(ref64))
    scale = max(1.0, float(np.abs(ref64).max()))
    E = float(np.abs(other - ref64).max())
    assert np.isfinite(ref64).all() and float(np.abs(ref64).max()) < 1000, f"max|ref64| = {np.abs(ref64).max()}"
    assert E <= 1e-4 * scale, f"E = {E:.3e} against scale {scale:.3e}"
    return max(E, 8 * EPS32 * scale)
