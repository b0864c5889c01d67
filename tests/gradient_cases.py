"""TEST INFRASTRUCTURE shared by tests/test_gpu_gradients.py: shapes, seeded states and inputs, the fp64 reference of a gradient
(tests/autograd_ref.py), its fp32 yardstick, the conditions a case must meet on the reference alone, and the comparison rule.
A plain module: nothing here is collected by pytest, and nothing here touches the device beyond reading a model's state.

The rule (tests/forecast_cases.py's), per case and per tensor:

    max|got - ref64| <= F * max(E, 8 eps32 max|ref64|) + R,      E = max|oracle_fp32 - ref64|

ref64 is autograd in fp64; oracle_fp32 the gradient of oracle.filter_step (tests/act_oracle.filter_step for another activation) run
in fp32 on the same values -- what fp32 rounding alone moves the gradient by, in numpy's order of summation.  R is the rounding of
the recovery: 0 for the raw sums; for a gradient recovered from a step, w1 = fl(w0 - lr clip(g)) with lr a power of two, one ulp of
the stored weight over lr, 2^-23 max(|w0|, |w1|) / lr (T ulps for T steps).  For a recovered step ref64 and oracle_fp32 are
clip(g, +-1): that is the quantity the step holds.
"""
import functools
import math
import zlib

import numpy as np
import torch
from torch import nn

from oracle import vjf_oracle as orc
from tests import act_oracle as ao
from tests import autograd_ref as ag
from tests.helpers import load_oracle_state, model_arrays
from tests.lifetime import FAMILIES
from tests.margins import check_close

EPS32 = float(np.finfo(np.float32).eps)
ULP = 2.0 ** -23
# The committed factor of the rule: it started at 4; at most twice the worst ratio achieved on the MI355X, never above 16.  Achieved
# (profiles/gradient_margins.json holds E, the ratios and this F): the worst ratio is 1.72 (the one-launch route's mean_W at one
# trial, RBF(200), hidden [128]); the recovered steps are between 0 and 1.3 otherwise, the raw sums at most 0.54, the three-step
# sums within their rounding term R.  F = 3.4 is within [1.72, 2 * 1.72].
F = 3.4
MODEL_SEED = 41

SHAPES = dict(FAMILIES)
SHAPES.update({
    "h32": dict(dy=10, dz=3, du=2, n=40, hidden=[32], lik="gaussian"),              # a gradient tile whose bias column is the 33rd
    "ragged": dict(dy=29, dz=3, du=0, n=40, hidden=[33, 31, 5], lik="gaussian"),    # din = 35: tiles that end at 1, 3 and 5 columns
    "long": dict(dy=50, dz=10, du=0, n=200, hidden=[128], lik="gaussian"),          # a long parameter vector: later SGD rounds read memory
})
# quiet inputs: the prior of the RBF weights is narrowed (w_chol = c I, w_precision = I / c^2) where the predictive variance
# sum Phi^2 of many features keeps lv_b loud, and the decoder of the widest observation is scaled down: lv_b's reconstruction
# term, exp(-rho) / 2 sigma^2 sum_i C_ij^2 over 300 outputs, is 4 at the default initialisation
W_CHOL_QUIET = {"rlsb": 0.25, "wide": 0.125}
DEC_W_QUIET = {"wide": 0.3}
# loud inputs: y ~ LOUD_Y N(0,1) -- 1 unless the batch mean over more outputs leaves fewer than a quarter of the entries clipped
LOUD_Y = {"long": 2.0, "ldschol": 2.0}

ACTS = {                                                  # name -> (module class / partial for Recognition, act_oracle code)
    "Tanh": (nn.Tanh, (ao.TANH, 0.0, 0.0)),
    "ReLU": (nn.ReLU, (ao.RELU, 0.0, 0.0)),
    "ELU": (functools.partial(nn.ELU, 0.5), (ao.ELU, 0.5, 0.0)),
    "Softplus": (functools.partial(nn.Softplus, beta=2.0, threshold=20.0), (ao.SOFTPLUS, 2.0, 20.0)),
    "Hardtanh": (functools.partial(nn.Hardtanh, -0.5, 0.5), (ao.HARDTANH, -0.5, 0.5)),
}
KINKS = {"Tanh": (), "ReLU": (0.0,), "ELU": (0.0,), "Softplus": (10.0,), "Hardtanh": (-0.5, 0.5)}     # (Softplus: beta x = threshold)

TRAIN = dict(sgd=True, update=True, warm_up=False)
WARM = dict(sgd=True, update=True, warm_up=True)
NO_UPDATE = dict(sgd=True, update=False, warm_up=False)


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def build(vjf, name, act="Tanh", lr=1.0):
    """The shape's model, seeded (the same state on every build, whichever device holds the blob), every group's lr = `lr`."""
    from vjf_amd.likelihood import GaussianLikelihood, PoissonLikelihood
    from vjf_amd.model import RBFDS
    from vjf_amd.recognition import Recognition
    f = SHAPES[name]
    torch.manual_seed(MODEL_SEED)
    lik = PoissonLikelihood() if f["lik"] == "poisson" else GaussianLikelihood()
    m = vjf.VJF(f["dy"], f["dz"], lik, RBFDS(f["n"], f["dz"], f["du"]),
                Recognition(f["dy"], f["dz"], f["du"], f["hidden"], activation=ACTS[act][0]), lr=lr)
    if f.get("wide_init"):                                   # (tests/lifetime.make_model: the default RBF init underflows at dz = 20)
        r = math.sqrt(f["dz"])
        feat = m.transition.velocity.feature
        g = torch.Generator().manual_seed(MODEL_SEED)
        with torch.no_grad():
            feat.centroid.copy_((torch.rand(f["n"], f["dz"] + f["du"], generator=g) * 2 - 1) * r)
            feat.logwidth.fill_(math.log(r))
    return m


def _put(t, a):
    with torch.no_grad():
        t.copy_(torch.as_tensor(np.asarray(a, np.float32)).reshape(t.shape).to(t.device))


def make_quiet(model, name):
    """The quiet starting point: lik_logvar = tr_logvar = log 2, w_mean ~ 0.05 N(0,1); Poisson: dec_b - 1; W_CHOL_QUIET, DEC_W_QUIET."""
    a = model_arrays(model)
    r = np.random.default_rng(seed_of("quiet", name))
    if "lik_logvar" in a:
        _put(a["lik_logvar"], math.log(2.0))
    _put(a["tr_logvar"], math.log(2.0))
    _put(a["w_mean"], 0.05 * r.standard_normal(tuple(a["w_mean"].shape)))
    if SHAPES[name]["lik"] == "poisson":
        _put(a["dec_b"], a["dec_b"].detach().cpu().numpy() - 1.0)
    if name in W_CHOL_QUIET:
        c = W_CHOL_QUIET[name]
        for k, f in (("w_chol", c), ("w_pchol", 1.0 / c), ("w_precision", 1.0 / (c * c))):
            _put(a[k], a[k].detach().cpu().numpy() * f)
    if name in DEC_W_QUIET:
        _put(a["dec_W"], a["dec_W"].detach().cpu().numpy() * DEC_W_QUIET[name])


def inputs(name, B, kind, T=1, shift=0):
    """CPU fp32 tensors y (T,B,dy), u (T,B,du) or None, eps (T,2,B,dz).
    loud: y ~ LOUD_Y N(0,1) (Poisson: counts of rate exp(0.5 N(0,1) + 2): those of tests/lifetime, of rate exp(0.5 N(0,1) - 0.5),
          clip 0.2 % of the entries);
    quiet: y ~ 0.5 N(0,1) (Poisson: counts of rate 0.4);
    quiet_rho: y ~ N(0,1), for the steps whose lik_logvar is set from the residual (set_rho_for_visible_gradient): the seed
          exp(-rho) r of the reconstruction term is then r / mean r^2, and grows as y shrinks."""
    f = SHAPES[name]
    g = torch.Generator().manual_seed(seed_of(name, B, kind, T) + shift)
    if f["lik"] == "poisson":
        rate = torch.full((T, B, f["dy"]), 0.4) if kind != "loud" else torch.exp(0.5 * torch.randn(T, B, f["dy"], generator=g) + 2.0)
        y = torch.poisson(rate, generator=g)
    else:
        y = torch.randn(T, B, f["dy"], generator=g) * {"quiet": 0.5, "quiet_rho": 1.0, "loud": LOUD_Y.get(name, 1.0)}[kind]
    u = torch.randn(T, B, f["du"], generator=g) if f["du"] else None
    return y, u, torch.randn(T, 2, B, f["dz"], generator=g)


def trainables(s, with_lik):
    return [k for k in ag.trainable_names(s) if with_lik or k != "lik_logvar"]


def oracle_step(s, act, y, u, mu_s, lv_s, eps_s, eps_t, **flags):
    """One step of the hand-derived oracle in the dtype of `s` (mutates `s`)"""
    dt = s.dtype
    c = lambda a: None if a is None else np.asarray(a, dt)          # noqa: E731
    code = ACTS[act][1]
    if code[0] == ao.TANH:
        return orc.filter_step(s, c(y), c(u), c(mu_s), c(lv_s), c(eps_s), c(eps_t), **flags)
    return ao.filter_step(s, code, c(y), c(u), c(mu_s), c(lv_s), c(eps_s), c(eps_t), **flags)


def set_rho_for_visible_gradient(model, act, y, u, eps):
    """lik_logvar = log(mean r^2) + off from the oracle's forward pass, so that its gradient 0.5 dy (1 - exp(-off)) is not clipped:
    off = 0.05 (a gradient of about 0.025 dy), and 0.5 / dy where that would still be beyond 0.9 (dy > 36: about 0.25)."""
    s = load_oracle_state(model, np.float64)
    o = oracle_step(s.clone(), act, y[0].numpy(), None if u is None else u[0].numpy(), None, None, eps[0, 0].numpy(), eps[0, 1].numpy(),
                    sgd=False, update=False)
    r = o.py - y[0].numpy().astype(np.float64)
    off = 0.05 if 0.025 * model.ydim < 0.9 else 0.5 / model.ydim
    _put(model_arrays(model)["lik_logvar"], math.log(float(np.mean(r * r))) + off)


class Reference:
    """ref64 (autograd), g32 (the fp32 oracle's hand-derived gradient) and the forward values the conditions need, of one step."""
    def __init__(self, s64, act, y, u, eps, *, warm_up=False, drop=(), mu_s=None, lv_s=None):
        import warnings
        n = lambda a: None if a is None else a.numpy()              # noqa: E731
        self.s64 = s64
        r = ag.step(s64, n(y), n(u), mu_s, lv_s, n(eps[0]), n(eps[1]), warm_up=warm_up, activation=ACTS[act][0](), drop=drop)
        self.ref, self.pre, self.eta, self.mu_t = r.grads, r.pre, r.eta, r.mu_t
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                         # (numpy's overflow warnings where a component is dropped)
            o = oracle_step(s64.cast(np.float32), act, n(y), n(u), mu_s, lv_s, n(eps[0]), n(eps[1]), sgd=True, update=False, warm_up=warm_up)
        assert (o.dyn == 0.0) == (ag.DYNAMICS in drop) and (o.recon == 0.0) == (ag.RECON in drop), "the fp32 oracle drops other components"
        self.g32 = ag.hand_gradients(o.grads, s64)
        assert all(np.isfinite(v).all() for v in self.ref.values()) and all(np.isfinite(v).all() for v in self.g32.values())


def yardstick(ref, g32, clip):
    """(E, max(E, 8 eps32 max|ref|)) of one tensor; clip: of clip(., +-1), the quantity a step holds"""
    ref, g32 = np.asarray(ref, np.float64), np.asarray(g32, np.float64).reshape(np.shape(ref))
    if clip:
        ref, g32 = np.clip(ref, -1, 1), np.clip(g32, -1, 1)
    E = float(np.abs(g32 - ref).max())
    return E, max(E, 8 * EPS32 * float(np.abs(ref).max()))


# ------------------------------------------------------------------ conditions on the reference alone
def share(ref, names, pred):
    tot = sum(ref[k].size for k in names)
    return sum(int(pred(np.abs(ref[k])).sum()) for k in names) / tot


def assert_kind(tag, kind, ref, names):
    if kind != "loud":                                     # at least 90 % of every tensor's entries have |g| < 0.9
        for k in names:
            q = float((np.abs(ref[k]) < 0.9).mean())
            assert q >= 0.9, f"{tag}: not quiet: {k} has {100 * q:.1f} % of its entries below 0.9"
    else:                                                   # over all tensors: at least 25 % clipped and at least 25 % not
        c = share(ref, names, lambda a: a > 1.0)
        assert 0.25 <= c <= 0.75, f"{tag}: not loud: {100 * c:.1f} % of the entries are clipped"


def assert_left_out(tag, R, w0, lr, names, T=1):
    """At most 1 % of a tensor's entries lie within its bound m of +-1, with m taken at its largest: |w1| <= |w0| + T lr."""
    for k in names:
        _, yard = yardstick(R.ref[k], R.g32[k], True)
        m = F * yard + T * ULP * (float(np.abs(w0[k]).max()) + T * lr) / lr
        near = np.abs(np.abs(R.ref[k]) - 1.0) < m
        assert near.mean() <= 0.01, f"{tag}: {k}: {int(near.sum())} of {near.size} entries within {m:.2e} of +-1"


def assert_off_kinks(tag, act, R, dist=1e-4):
    pre = np.concatenate([p.ravel() for p in R.pre])
    for kk in KINKS[act]:
        d = float(np.abs(pre - kk).min())
        assert d >= dist, f"{tag}: a pre-activation lies {d:.2e} from the kink at {kk}"
    if act in ("ReLU", "ELU", "Hardtanh"):                  # (both sides of a kink are taken)
        assert (pre < KINKS[act][0]).mean() > 0.05 and (pre > KINKS[act][-1]).mean() > 0.05, f"{tag}: one branch only"


def assert_straddles_clamp(tag, R, dist=1e-3, least=10):
    hi, lo = int((R.eta > 10.0 + dist).sum()), int((R.eta < 10.0 - dist).sum())
    assert hi >= least and lo >= least and hi + lo == R.eta.size, f"{tag}: eta: {hi} above, {lo} below, {R.eta.size - hi - lo} at the clamp"


# ------------------------------------------------------------------ comparisons
def state64(model, names):
    a = model_arrays(model)
    return {k: a[k].detach().cpu().numpy().astype(np.float64).copy() for k in names}


def compare_sums(tag, got, R, names):
    """Raw gradient sums over B (`got`: already divided by B) against autograd: every entry, R = 0."""
    for k in names:
        E, yard = yardstick(R.ref[k], R.g32[k], False)
        err = float(np.abs(got[k] - R.ref[k]).max())
        print(f"{tag} {k}: err {err:.3e} E {E:.3e} yard {yard:.3e} ratio {err / yard:.2f} max|ref| {np.abs(R.ref[k]).max():.3e}")
    for k in names:
        E, yard = yardstick(R.ref[k], R.g32[k], False)
        check_close(got[k], R.ref[k], rtol=0, atol=F * yard, err_msg=f"{tag}: gradient of {k}",
                    what=f"{tag} {k} [E={E:.3e} yard={yard:.3e} R=0 F={F}]")


def compare_step(tag, w0, w1, R, names, lr):
    """The gradient recovered from one step, (w0 - w1) / lr = clip(g): values where |g_ref| <= 1 - m, w1 == float32(w0 -+ lr) bit
    for bit where |g_ref| >= 1 + m; entries within m (the tensor's bound) of +-1 are left out (assert_left_out caps their number)."""
    rows = []
    for k in names:
        ref = R.ref[k]
        E, yard = yardstick(ref, R.g32[k], True)
        rnd = ULP * max(float(np.abs(w0[k]).max()), float(np.abs(w1[k]).max())) / lr
        m = F * yard + rnd
        got = (w0[k] - w1[k]) / lr
        U, C = np.abs(ref) <= 1.0 - m, np.abs(ref) >= 1.0 + m
        err = float(np.abs(got - ref)[U].max()) if U.any() else 0.0
        print(f"{tag} {k}: unclipped {int(U.sum())} clipped {int(C.sum())} of {ref.size}: err {err:.3e} E {E:.3e} yard {yard:.3e} "
              f"R {rnd:.3e} ratio {max(err - rnd, 0.0) / yard:.2f}")
        rows.append((k, ref, E, yard, rnd, m, got, U, C))
    for k, ref, E, yard, rnd, m, got, U, C in rows:
        if U.any():
            check_close(got[U], ref[U], rtol=0, atol=m, err_msg=f"{tag}: recovered gradient of {k}",
                        what=f"{tag} {k} [E={E:.3e} yard={yard:.3e} R={rnd:.3e} F={F}]")
        if C.any():
            want = (w0[k].astype(np.float32) - np.float32(lr) * np.sign(ref).astype(np.float32))
            bad = (w1[k].astype(np.float32) != want) & C
            assert not bad.any(), f"{tag}: {k}: {int(bad.sum())} of {int(C.sum())} clipped entries are not float32(w0 -+ lr)"


def compare_total(tag, w0, wT, ref_sum, sum32, names, lr, T):
    """(w0 - wT) / lr of T steps against the same sum of clip(g_t) from the fp64 oracle: every entry (clip is continuous)."""
    for k in names:
        E, yard = yardstick(ref_sum[k], sum32[k], False)
        rnd = T * ULP * max(float(np.abs(w0[k]).max()), float(np.abs(wT[k]).max())) / lr
        got = (w0[k] - wT[k]) / lr
        err = float(np.abs(got - ref_sum[k]).max())
        print(f"{tag} {k}: err {err:.3e} E {E:.3e} yard {yard:.3e} R {rnd:.3e} ratio {max(err - rnd, 0.0) / yard:.2f}")
        check_close(got, ref_sum[k], rtol=0, atol=F * yard + rnd, err_msg=f"{tag}: summed gradient of {k}",
                    what=f"{tag} {k} [E={E:.3e} yard={yard:.3e} R={rnd:.3e} F={F}]")
