"""TEST INFRASTRUCTURE: the forgetting factor of the RLS update (`transition.shrink`, VJF_SC_SHRINK), shared by the host tests
(tests/test_forget_host.py) and the GPU tests (tests/test_gpu_forget.py).  A plain module: nothing here is collected by pytest.

The oracle's step calls `rls(..., 1.0)` (oracle/vjf_oracle.py, as the reference's step does, vjf/model.py:371); `pin` replaces the
module's `rls` for the length of a test by a wrapper that runs it with a pinned factor -- the oracle itself is not edited.
`tests/lifetime.reference` is never used here: its cache is shared with the lifetime tests, which expect the unpatched oracle.
"""
import warnings

import numpy as np

from oracle import vjf_oracle as orc
from tests import goldenio as gio
from tests import lifetime as life
from tests.helpers import load_oracle_state

LAM = 0.9
FIXTURES = {"f64": "g10_forget0.9_f64", "f32": "g10_forget0.9_f32"}      # tests/golden/make_golden_forget.py
# test_rls_failure_is_flagged_and_leaves_rls_state's: one block; three blocks failing in the second column; the multi-launch path
FAIL_SHAPES = ((16, 0), (72, 40), (260, 100))


class Pin:
    """The factor the patched oracle runs with (`lam` may be changed between calls) and how many of its factorisations failed."""
    def __init__(self, lam):
        self.lam, self.failed = lam, 0


def pin(monkeypatch, lam=LAM):
    """monkeypatch.setattr(orc, "rls", ...): every RLS update of the oracle's step runs with `pin.lam` until the test ends."""
    real = orc.rls
    p = Pin(lam)

    def rls(s, feat, target, v, shrink=1.0):
        st = real(s, feat, target, v, p.lam)
        p.failed += int(st != 0)
        return st
    monkeypatch.setattr(orc, "rls", rls)
    return p


def run_traj(name):
    """A trajectory fixture on the oracle, step by step (as tests/test_oracle_golden.py runs the g5 ones)."""
    z, info, s = gio.traj_case(name)
    u = z["u"] if info["du"] else None
    outs = []
    for t in range(info["T"]):
        mu = outs[-1].mu_t if outs else None
        lv = outs[-1].lv_t if outs else None
        o = orc.filter_step(s, z["y"][t], None if u is None else u[t], mu, lv, z["eps"][t, 0], z["eps"][t, 1],
                            sgd=True, update=True, warm_up=info["warm_up"])
        outs.append(o)
        o.rho = float(s.lik_logvar) if s.lik_logvar is not None else 0.0
        o.sigma = float(s.tr_logvar)
        o.n_lik, o.n_tr = s.n_lik, s.n_tr
        if f"s{t + 1}.w_mean" in z.files:
            o.state = s.clone()
    return z, info, s, outs


_TRACES = {}


def reference(fam, model, monkeypatch, lam=LAM):
    """The lifetime script on the oracle with the factor pinned, in fp64 and in fp32, from `model`'s CURRENT state -- which must be
    the seeded initial one.  Computed once per (family, factor) and shared (the overlap settings of one family); read-only."""
    key = (fam, lam)
    if key not in _TRACES:
        p = pin(monkeypatch, lam)
        s64, s32 = load_oracle_state(model, np.float64), load_oracle_state(model, np.float32)
        s0 = s64.clone()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            steps = list(life.drive(fam, None, (s64, s32)))
        assert p.failed == 0, f"{fam}: {p.failed} factorisations of the oracle failed: the yardstick would be meaningless"
        _TRACES[key] = life.Trace(s0, [st.refs[0] for st in steps], [st.refs[1] for st in steps], s64, s32)
    return _TRACES[key]
