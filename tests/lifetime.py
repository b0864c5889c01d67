"""TEST INFRASTRUCTURE: one native context across its life.

A context is created for `max_batch` trials and then serves whatever comes: any B <= max_batch, every flag set of `VJF.filter`,
`filter` and `filter_sequence` interleaved, a posterior or the prior, `set_state` from the host, learning-rate and decoder-freeze
changes between calls, growth (the host mirror re-creates the context for a larger batch).  This module holds

  FAMILIES   the smallest shape of every plan family (taken from CASES of tests/test_gpu_parity.py),
  SCRIPT     nine calls on ONE model, 19 steps in all,
  drive      the driver: the script on a model and / or on oracle states, in step,

and the comparisons the GPU tests (tests/test_gpu_lifetime.py) and the host tests (tests/test_lifetime_host.py) share.  It is a plain
module: nothing here is collected by pytest.  An activation axis can be added to FAMILIES / make_model without touching the script.
"""
import collections
import math

import numpy as np
import torch

from oracle import vjf_oracle as orc
from tests import goldenio as gio
from tests.helpers import LOOSE, load_oracle_state, model_arrays
from tests.margins import check_close

# id -> shape; `small`: the batch of call 7 (one trial where the plan serves it; 24 trials where the RLS update of ONE trial against
# hundreds of features is so ill-conditioned that the fp32 reference itself is off by more than the fixed tolerance)
FAMILIES = {
    "mega": dict(dy=10, dz=3, du=2, n=40, hidden=[8], lik="gaussian", small=1),           # one-launch, 2 blocks (last partial), control input
    "mega_p": dict(dy=12, dz=5, du=0, n=100, hidden=[20, 12], lik="poisson", small=1),    # one-launch, 4 blocks, two layers
    "rlsb": dict(dy=10, dz=3, du=0, n=260, hidden=[8], lik="gaussian", small=24),         # multi-launch RLS (n > 224), two-stream
    "serial": dict(dy=9, dz=4, du=1, n=222, hidden=[12], lik="gaussian", small=24),       # n % 4 != 0: single-workgroup serial kernel
    "ldschol": dict(dy=30, dz=20, du=0, n=96, hidden=[32], lik="gaussian", small=24, wide_init=True),   # 16 < dz <= 32: LDS Cholesky, own solve / inverse
    "wide": dict(dy=300, dz=6, du=0, n=1200, hidden=[400], lik="gaussian", small=24),     # GEMM-per-layer trial path + multi-launch RLS
}
MODEL_SEED, DATA_SEED = 41, 42
LR = 1e-3

TR = dict(sgd=True, update=True, warm_up=False)
WARM = dict(sgd=True, update=True, warm_up=True)
INFER = dict(sgd=False, update=False, warm_up=False)
SGD_ONLY = dict(sgd=True, update=False, warm_up=False)
RLS_ONLY = dict(sgd=False, update=True, warm_up=False)

Call = collections.namedtuple("Call", "k entry B T flags start before")
# before: "halve_lr_freeze" -- every group's lr x 0.5 and freeze_decoder(True); "state_round_trip" -- m.set_state(m.get_state())
SCRIPT = (
    Call(1, "filter_sequence", 64, 3, WARM, "prior", None),
    Call(2, "filter_sequence", 64, 2, TR, "posterior", None),              # from the last posterior of call 1
    Call(3, "filter", 37, 1, TR, "prior", None),
    Call(4, "filter_sequence", 37, 3, INFER, "posterior", None),           # from the posterior of call 3
    Call(5, "filter_sequence", 150, 2, TR, "prior", None),                 # (the host mirror grows the context)
    Call(6, "filter_sequence", 64, 2, SGD_ONLY, "prior", "halve_lr_freeze"),
    Call(7, "filter_sequence", "small", 2, TR, "prior", "state_round_trip"),
    Call(8, "filter_sequence", 64, 2, RLS_ONLY, "prior", None),
    Call(9, "filter_sequence", 150, 2, TR, "prior", None),
)

# tolerances against the fp64 oracle: test_filter_vs_oracle's for the outputs, test_filter_sequence_vs_oracle's for the state
POST = dict(rtol=2e-6, atol=2e-6)
LOSS = dict(rtol=2e-5, atol=2e-5)
STATE = dict(rtol=1e-5, atol=1e-6)
RLS = dict(rtol=5e-3, atol=5e-5)


def batch(fam, call):
    return FAMILIES[fam]["small"] if call.B == "small" else call.B


def make_model(vjf, fam):
    """The family's model, seeded: the same initial state on every build, with or without a GPU."""
    f = FAMILIES[fam]
    torch.manual_seed(MODEL_SEED)
    m = vjf.VJF.make_model(f["dy"], f["dz"], f["du"], f["n"], f["hidden"], likelihood=f["lik"], lr=LR)
    if f.get("wide_init"):
        # initialise-style RBF init (as test_filter_vs_oracle does for wide latents): the default one makes every feature underflow
        # at dz = 20 and the RLS comparison vacuous.  Drawn on the CPU generator: identical whichever device holds the blob.
        r = math.sqrt(f["dz"])
        feat = m.transition.velocity.feature
        g = torch.Generator().manual_seed(MODEL_SEED)
        with torch.no_grad():
            feat.centroid.copy_((torch.rand(f["n"], f["dz"] + f["du"], generator=g) * 2 - 1) * r)
            feat.logwidth.fill_(math.log(r))
    return m


_INPUTS = {}


def inputs(fam):
    """[(y, u, eps)] per call of the script: CPU fp32 tensors from one seeded generator.  Cached; read-only."""
    if fam not in _INPUTS:
        f = FAMILIES[fam]
        g = torch.Generator().manual_seed(DATA_SEED)
        out = []
        for call in SCRIPT:
            T, B = call.T, batch(fam, call)
            if f["lik"] == "poisson":
                y = torch.poisson(torch.exp(0.5 * torch.randn(T, B, f["dy"], generator=g) - 0.5), generator=g)
            else:
                y = torch.randn(T, B, f["dy"], generator=g)
            u = torch.randn(T, B, f["du"], generator=g) if f["du"] else None
            out.append((y, u, torch.randn(T, 2, B, f["dz"], generator=g)))
        _INPUTS[fam] = out
    return _INPUTS[fam]


def _call_model(model, call, y, u, eps, qs):
    """One call of the script on the model -> (mu (T,B,dz), logvar (T,B,dz), loss (T,4))"""
    if call.entry == "filter":
        q, loss, *comp = model.filter(y[0], None if u is None else u[0], qs, verbose=True, eps=(eps[0, 0], eps[0, 1]), **call.flags)
        return q.mean[None], q.logvar[None], torch.stack([loss, *comp])[None]
    return model.filter_sequence(y, u, qs, eps=eps, **call.flags)


Step = collections.namedtuple("Step", "k call B out refs")


def drive(fam, model=None, oracles=(), *, pre=None, around=None):
    """Generator over the script: runs call k on `model` (if given) and on every OracleState of `oracles`, then yields
    Step(k, call, B, out, refs) -- `out` the model's three output tensors (None without a model), `refs` one
    (mu, logvar, losses) numpy triple per oracle.  `pre(k, call, B)` runs before anything of call k; `around(k, thunk)` wraps the
    model's call (default: thunk())."""
    import vjf_amd
    post_m, post_o = None, [None] * len(oracles)
    for call, (y, u, eps) in zip(SCRIPT, inputs(fam)):
        B = y.shape[1]
        if pre is not None:
            pre(call.k, call, B)
        if call.before == "halve_lr_freeze":
            if model is not None:
                for g in model.optimizer.param_groups:
                    g["lr"] = g["lr"] * 0.5
                model.freeze_decoder(True)
            for s in oracles:
                s.lr = [v * 0.5 for v in s.lr]
                s.freeze_decoder = True
        elif call.before == "state_round_trip" and model is not None:     # (changes nothing in the oracle)
            model.set_state(model.get_state())
        out = None
        if model is not None:
            qs = None if call.start == "prior" else post_m
            thunk = lambda: _call_model(model, call, y, u, eps, qs)          # noqa: E731
            out = around(call.k, thunk) if around is not None else thunk()
            post_m = vjf_amd.Gaussian(out[0][-1], out[1][-1])
        refs = []
        for i, s in enumerate(oracles):
            mu0, lv0 = (None, None) if call.start == "prior" else post_o[i]
            r = orc.filter_sequence(s, y.numpy(), None if u is None else u.numpy(), eps.numpy(), mu0=mu0, lv0=lv0, **call.flags)
            post_o[i] = (r[0][-1], r[1][-1])
            refs.append(r)
        yield Step(call.k, call, B, out, refs)


Trace = collections.namedtuple("Trace", "s0 refs64 refs32 s64 s32")
_TRACES = {}


def reference(fam, model):
    """The script on the oracle in fp64 and in fp32 (the reference's own arithmetic) from `model`'s CURRENT state -- which must be the
    seeded initial one: computed once per family and shared by the tests that need it.  Read-only."""
    if fam not in _TRACES:
        s64, s32 = load_oracle_state(model, np.float64), load_oracle_state(model, np.float32)
        s0 = s64.clone()
        steps = list(drive(fam, None, (s64, s32)))
        _TRACES[fam] = Trace(s0, [st.refs[0] for st in steps], [st.refs[1] for st in steps], s64, s32)
    return _TRACES[fam]


def expected_counters(fam):
    """(n_lik, n_tr) after the script, from the running-variance recurrence n <- min(n, cap) + B of every step with update=True
    (vjf/util.py:20-35; caps 1000 and 500); a Poisson likelihood keeps no count."""
    n_lik = n_tr = 0
    for call in SCRIPT:
        if call.flags["update"]:
            for _ in range(call.T):
                n_lik = min(n_lik, 1000) + batch(fam, call)
                n_tr = min(n_tr, 500) + batch(fam, call)
    return (n_lik if FAMILIES[fam]["lik"] == "gaussian" else 0), n_tr


def _np(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float64)


def compare_outputs(tag, step, ref, post=POST, loss=LOSS):
    """mu, logvar and the loss rows of one call against an oracle's (asserts, and records the achieved margins)"""
    mu, lv, ls = step.out
    check_close(_np(mu), ref[0], err_msg=f"{tag} call {step.k}: mean", what=f"{tag} call {step.k} mean", **post)
    check_close(_np(lv), ref[1], err_msg=f"{tag} call {step.k}: logvar", what=f"{tag} call {step.k} logvar", **post)
    check_close(_np(ls), ref[2], err_msg=f"{tag} call {step.k}: losses", what=f"{tag} call {step.k} losses", **loss)


def compare_state(tag, model, s64, s32):
    """The whole state after the script.  Non-RLS tensors at STATE.  The four RLS tensors as tools/fuzz_parity.py judges them: the
    suite's fixed tolerance (RLS) first; beyond it, at most 3 x as far from fp64 as the oracle run in fp32 on the same script (its
    Judge raises beyond that) -- such a tensor is returned as a note and recorded with that bound.  Counters: exactly."""
    from tools.fuzz_parity import Judge
    judge = Judge()
    got = {k: _np(v) for k, v in model_arrays(model).items()}
    w64, w32 = gio.state_arrays(s64), gio.state_arrays(s32)
    w64["prior_mean"], w64["prior_logvar"] = s64.prior_mean, s64.prior_logvar
    for k in sorted(got):
        if w64.get(k) is None:
            continue
        r64 = np.asarray(w64[k], np.float64).reshape(got[k].shape)
        if k not in LOOSE:
            check_close(got[k], r64, err_msg=f"{tag}: state tensor {k}", what=f"{tag} state {k}", **STATE)
        elif np.allclose(got[k], r64, **RLS):
            check_close(got[k], r64, err_msg=f"{tag}: state tensor {k}", what=f"{tag} state {k} [rls]", **RLS)
        else:
            r32 = np.asarray(w32[k], np.float64).reshape(got[k].shape)
            n = len(judge.notes)
            judge(f"{tag} state {k}", got[k], r64, r32, RLS["rtol"], RLS["atol"])
            assert len(judge.notes) == n + 1
            bound = judge.slack * np.abs(r32 - r64).max() + RLS["atol"] + 1e-5 * np.abs(r64).max()      # (the Judge's own bound)
            check_close(got[k], r64, rtol=0.0, atol=float(bound), err_msg=f"{tag}: state tensor {k}",
                        what=f"{tag} state {k} [rls, NOTE fp32 yardstick: {judge.notes[-1]}]")
    assert model._get_counter("lik") == s64.n_lik, (tag, model._get_counter("lik"), s64.n_lik)
    assert model._get_counter("tr") == s64.n_tr, (tag, model._get_counter("tr"), s64.n_tr)
    return list(judge.notes)


def blob_diff(a, b):
    """Which tensors of two models' state blobs differ, and by how much (the message of a failed bitwise assertion)."""
    out = []
    ta, tb = model_arrays(a), model_arrays(b)
    for k in sorted(ta):
        if not torch.equal(ta[k], tb[k]):
            out.append(f"{k}: max |d| {float((ta[k].double() - tb[k].double()).abs().max()):.3e}")
    sa, sb = a._scalars.cpu().tolist(), b._scalars.cpu().tolist()
    out += [f"scalar[{i}]: {x} vs {y}" for i, (x, y) in enumerate(zip(sa, sb)) if x != y]
    return "; ".join(out) or ("blobs differ outside every named tensor" if not torch.equal(a._blob, b._blob) else "equal")


ROUTE_NAME = {0: "per-step", 1: "one-launch", 2: "two-stream", 3: "streams", 4: "packed"}


def flag_bits(flags):
    from vjf_amd import _native as N
    return (N.FLAG_SGD if flags["sgd"] else 0) | (N.FLAG_UPDATE if flags["update"] else 0) | (N.FLAG_WARM_UP if flags["warm_up"] else 0)


def expected_route(fam, setting, flags):
    """The route of a sequence on one rank for the families "mega" and "rlsb", by the overlap setting `vjf_set_overlap` returned
    (the table at pick_route, vjf_host_routes.h): 1 -- one-launch unless the call asks for an RLS update without SGD, the
    multi-launch RLS plans their update on a second stream; 0 -- the one-stream order; 3 -- three streams for an RLS update on the
    plans that have the fast kernels, nothing else."""
    rls = flags["update"] and not flags["warm_up"]
    if setting == 0:
        return "per-step"
    if fam == "mega":
        if setting == 3:
            return "streams" if rls else "per-step"
        return "per-step" if (rls and not flags["sgd"]) else "one-launch"
    assert fam == "rlsb" and setting == 1
    return "two-stream" if rls else "per-step"
