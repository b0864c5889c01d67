"""The gradients themselves, which `w -= lr clip(g, +-1)` at the suite's learning rates hides: the raw gradient sums of the per-step
routes (the reduce buffer behind vjf_filter_local), and on every route the gradient recovered from one step at lr = 1,
(w0 - w1) = clip(g) -- values where the reference is inside +-1, w1 == float32(w0 -+ 1) bit for bit where it is outside.  The
reference is torch autograd in fp64 (tests/autograd_ref.py); the rule, its yardstick E and the conditions every case asserts on the
reference alone, before the device is touched, are in tests/gradient_cases.py.  Every comparison goes through tests.margins.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from tests import autograd_ref as ag
from tests import goldenio as gio
from tests import gradient_cases as gc
from tests.helpers import load_oracle_state, model_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


# ------------------------------------------------------------------ 1. the raw gradient sums of the per-step routes
# (shape, B, activation, special): the smallest shapes that reach each kernel and edge -- the matrix-core trial kernel with 16 trials
# per workgroup (B around 16), the GEMM-per-layer path (wide: 4 trials per loss workgroup), bias columns that are a tile's 33rd,
# ragged tiles, three row splits of the Gram kernel with a short last one (B = 777), the Poisson clamp
SUMS = [(f, B, "Tanh", None) for f in ("mega", "mega_p", "ldschol") for B in (1, 15, 16, 17, 37)]
SUMS += [("wide", 37, "Tanh", None), ("h32", 37, "Tanh", None), ("ragged", 37, "Tanh", None), ("mega", 777, "Tanh", None),
         ("mega", 37, "ELU", None), ("wide", 37, "ReLU", None), ("mega_p", 37, "Tanh", "clamp")]


# data-seed shifts, chosen on the reference alone: the first for which every pre-activation keeps 1e-4 from the activation's kinks
SEED_SHIFT = {("sums", "wide", "ReLU"): 1, ("step", "ReLU"): 1, ("step", "ELU"): 1}


def case_sums(vjf, shape, B, act, special):
    tag = f"sums {shape} B={B} {act}" + (f" {special}" if special else "")
    m = gc.build(vjf, shape, act)
    if special == "clamp":                                    # eta on both sides of the clamp at 10 (vjf/likelihood.py:60)
        a = model_arrays(m)
        gc._put(a["dec_W"], a["dec_W"].detach().cpu().numpy() * 8.0)
        gc._put(a["dec_b"], a["dec_b"].detach().cpu().numpy() + 6.0)
    y, u, eps = gc.inputs(shape, B, "loud", shift=SEED_SHIFT.get(("sums", shape, act), 0))
    R = gc.Reference(load_oracle_state(m, np.float64), act, y[0], None if u is None else u[0], eps[0])
    if special == "clamp":
        gc.assert_straddles_clamp(tag, R)
    if act != "Tanh":
        gc.assert_off_kinks(tag, act, R)
    return tag, m, (y, u, eps), R


@pytest.mark.parametrize("shape,B,act,special", SUMS, ids=[f"{s}-{B}-{a}" + (f"-{x}" if x else "") for s, B, a, x in SUMS])
def test_raw_gradient_sums(vjf, shape, B, act, special):
    from vjf_amd import _native as N
    tag, m, (y, u, eps), R = case_sums(vjf, shape, B, act, special)
    yd, ud, ed = y[0].cuda(), None if u is None else u[0].cuda(), eps[0].cuda()
    m._ensure_ctx(B)
    m._push_lr()
    L, ctx = m._backend(), m._ctx
    flags = N.FLAG_SGD | N.FLAG_UPDATE
    dz = m.xdim
    mu, lv = torch.empty(B, dz, device="cuda"), torch.empty(B, dz, device="cuda")
    N.check(L.vjf_set_stream(ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    N.check(L.vjf_filter_local(ctx, B, N.ptr(yd), N.ptr(ud), None, None, N.ptr(ed[0]), N.ptr(ed[1]), N.ptr(mu), N.ptr(lv), flags))
    torch.cuda.synchronize()
    red = m._reduce.detach().cpu().numpy().astype(np.float64)
    a = model_arrays(m)
    base = a["rec_W0"].data_ptr()
    names = gc.trainables(R.s64, with_lik=False)
    got = {}
    for k in names:
        o = (a[k].data_ptr() - base) // 4                     # the sums mirror the state blob from REC_W0 to DEC_B
        got[k] = red[o:o + a[k].numel()].reshape(tuple(a[k].shape)) / B
    if "lik_logvar" in a:                                     # RS_SSEY sits behind the sums (and the three loss sums)
        train_len = (a["dec_b"].data_ptr() - base) // 4 + (a["dec_b"].numel() + 3) // 4 * 4
        rho = float(R.s64.lik_logvar)
        got["lik_logvar"] = np.asarray(0.5 * (m.ydim - np.exp(-rho) * red[train_len + 3] / B))
        names = names + ["lik_logvar"]
    gc.compare_sums(tag, got, R, names)
    np.testing.assert_allclose(mu.cpu().numpy(), R.mu_t, rtol=2e-5, atol=2e-5)      # (the step that was measured is the case's)


# ------------------------------------------------------------------ 2. the gradient recovered from one step
_REFERENCES = {}


def case_step(vjf, shape, B, kind, flags, *, act="Tanh", rho=False, drop=(), freeze=False):
    """model (lr = 1 in all four groups), inputs and reference of one step, with the case's conditions asserted on the reference"""
    tag = f"step {shape} B={B} {kind} {'/'.join(k for k, v in flags.items() if v)} {act}" + (" dropped-dynamics" if drop else "") \
          + (" frozen-decoder" if freeze else "")
    m = gc.build(vjf, shape, act, lr=1.0)
    if kind != "loud":
        gc.make_quiet(m, shape)
    y, u, eps = gc.inputs(shape, B, "quiet_rho" if (rho and kind == "quiet") else kind, shift=SEED_SHIFT.get(("step", act), 0))
    if rho:
        gc.set_rho_for_visible_gradient(m, act, y, u, eps)
    if drop:
        with torch.no_grad():
            m.transition.velocity.w_chol.mul_(1e25)           # the predictive variance overflows fp32: the dynamics component is dropped
    if freeze:
        m.freeze_decoder(True)
    key = (shape, B, kind, flags["update"], flags["warm_up"], act, rho, bool(drop))
    if key not in _REFERENCES:                                        # (computed once, shared by the routes, never modified)
        _REFERENCES[key] = gc.Reference(load_oracle_state(m, np.float64), act, y[0], None if u is None else u[0], eps[0],
                                        warm_up=flags["warm_up"], drop=drop)
    R = _REFERENCES[key]
    names = gc.trainables(R.s64, with_lik=not flags["update"])        # (an update moves lik_logvar by the running variance as well)
    gc.assert_kind(tag, kind, R.ref, names)
    gc.assert_left_out(tag, R, gc.state64(m, names), 1.0, names)
    if act != "Tanh":
        gc.assert_off_kinks(tag, act, R)
    return tag, m, (y, u, eps), R, names


def run_step(m, R, route, y, u, eps, flags, overlap=None):
    if overlap is not None:
        m.set_overlap(overlap)
    names = ag.trainable_names(R.s64)
    w0 = gc.state64(m, names)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.filter_sequence(y.cuda(), None if u is None else u.cuda(), None, eps=eps.cuda(), **flags)
        torch.cuda.synchronize()
        if route is not None:
            assert m.route(**flags) == route, (m.route(**flags), route)
        st = m.status()
    assert st & m._WAIT_BITS == 0, hex(st)
    return w0, gc.state64(m, names), st


# shapes whose one-launch grid gives a trial workgroup several 32-trial tiles on 256 compute units: the trial role gets at most
# (256 - n_rls - n_prep) * 128 / 227 workgroups (mega_shape) -- 128 for RBF(200), so 4097 trials are 129 tiles
ONE_LAUNCH = [(f, B, "loud") for f in ("mega", "mega_p", "long") for B in (1, 32, 33, 37)]
ONE_LAUNCH += [(f, 37, "quiet") for f in ("mega", "mega_p", "long")] + [("long", 4097, "quiet")]


@pytest.mark.parametrize("shape,B,kind", ONE_LAUNCH, ids=[f"{s}-{B}-{k}" for s, B, k in ONE_LAUNCH])
def test_one_launch_step(vjf, shape, B, kind):
    tag, m, (y, u, eps), R, names = case_step(vjf, shape, B, kind, gc.TRAIN)
    w0, w1, st = run_step(m, R, "one-launch", y, u, eps, gc.TRAIN)
    assert st == 0
    gc.compare_step(tag + " one-launch", w0, w1, R, names, 1.0)


NO_RLS = [(s, k, f) for s in ("mega", "mega_p") for k, f in (("warm_up", gc.WARM), ("no_update", gc.NO_UPDATE))]


@pytest.mark.parametrize("shape,which,flags", NO_RLS, ids=[f"{s}-{k}" for s, k, _ in NO_RLS])
def test_one_launch_step_without_rls_update(vjf, shape, which, flags):
    """warm_up: the gradient has no dynamics term; update=False: lik_logvar moves by its gradient alone, made visible by its value."""
    rho = which == "no_update" and gc.SHAPES[shape]["lik"] == "gaussian"
    tag, m, (y, u, eps), R, names = case_step(vjf, shape, 37, "quiet", flags, rho=rho)
    assert ("lik_logvar" in names) == rho
    w0, w1, st = run_step(m, R, "one-launch", y, u, eps, flags)
    assert st == 0
    gc.compare_step(tag + " one-launch", w0, w1, R, names, 1.0)


# prep-kernel SGD | the serial kernel's SGD (n % 4 != 0) | multi-launch RLS | LDS Cholesky, dz > 16 | the GEMM-per-layer trial path
ONE_STREAM = [(s, k, f) for s in ("mega", "serial", "rlsb", "ldschol", "wide")
              for k, f in (("loud", gc.TRAIN), ("quiet", gc.TRAIN), ("quiet", gc.NO_UPDATE))]


@pytest.mark.parametrize("shape,kind,flags", ONE_STREAM, ids=[f"{s}-{k}-{'train' if f['update'] else 'no_update'}" for s, k, f in ONE_STREAM])
def test_one_stream_step(vjf, shape, kind, flags):
    tag, m, (y, u, eps), R, names = case_step(vjf, shape, 37, kind, flags, rho=not flags["update"])
    w0, w1, st = run_step(m, R, "per-step", y, u, eps, flags, overlap=False)
    assert st == 0
    gc.compare_step(tag + " one-stream", w0, w1, R, names, 1.0)


@pytest.mark.parametrize("overlap", [1, False], ids=["one-launch", "one-stream"])
@pytest.mark.parametrize("act", ["ReLU", "ELU", "Softplus", "Hardtanh"])
def test_activation_step(vjf, act, overlap):
    tag, m, (y, u, eps), R, names = case_step(vjf, "mega", 37, "quiet", gc.TRAIN, act=act)
    w0, w1, st = run_step(m, R, "one-launch" if overlap else "per-step", y, u, eps, gc.TRAIN, overlap=overlap)
    assert st == 0
    gc.compare_step(tag + (" one-launch" if overlap else " one-stream"), w0, w1, R, names, 1.0)


@pytest.mark.parametrize("overlap", [1, False], ids=["one-launch", "one-stream"])
def test_replayed_step_has_the_gradient_without_the_dropped_component(vjf, overlap):
    """A non-finite dynamics component is the constant 0 (vjf/model.py:141-142): the step is replayed without its seeds, and the
    recovered gradient is autograd's of the loss without that component."""
    from vjf_amd import _native as N
    tag, m, (y, u, eps), R, names = case_step(vjf, "mega", 37, "quiet", gc.TRAIN, drop={ag.DYNAMICS})
    m2 = gc.build(vjf, "mega")
    gc.make_quiet(m2, "mega")
    full = ag.step(load_oracle_state(m2, np.float64), y[0].numpy(), u[0].numpy(), None, None, eps[0, 0].numpy(), eps[0, 1].numpy()).grads
    assert np.abs(full["mean_W"] - R.ref["mean_W"]).max() > 1e-2         # (the dropped component does carry gradient)
    w0, w1, st = run_step(m, R, "one-launch" if overlap else "per-step", y, u, eps, gc.TRAIN, overlap=overlap)
    assert st & N.STATUS_NONFINITE_DYN
    gc.compare_step(tag + (" one-launch" if overlap else " one-stream"), w0, w1, R, names, 1.0)


# ------------------------------------------------------------------ 3. three steps: the routes that exist only for T > 1
SEQ = [("mega", 1, "one-launch"), ("mega", 3, "streams"), ("rlsb", 1, "two-stream")]


def case_three_steps(vjf, shape, lr, T):
    tag = f"three-steps {shape}"
    m = gc.build(vjf, shape, lr=lr)
    gc.make_quiet(m, shape)
    y, u, eps = gc.inputs(shape, 37, "quiet", T=T)
    s64 = load_oracle_state(m, np.float64)
    names = gc.trainables(s64, with_lik=False)
    sums = []
    for s in (s64.clone(), s64.cast(np.float32)):
        before = {k: np.asarray(v, np.float64).copy() for k, v in gio.state_arrays(s).items()}
        mu = lv = None
        for t in range(T):
            o = gc.oracle_step(s, "Tanh", y[t].numpy(), None if u is None else u[t].numpy(), mu, lv, eps[t, 0].numpy(), eps[t, 1].numpy(),
                               **gc.TRAIN)
            mu, lv = o.mu_t, o.lv_t
            if s.dtype == np.float64:
                gc.assert_kind(f"{tag} step {t}", "quiet", ag.hand_gradients(o.grads, s), names)
        after = gio.state_arrays(s)
        sums.append({k: (before[k] - np.asarray(after[k], np.float64)) / lr for k in names})
    return tag, m, (y, u, eps), sums[0], sums[1], names


@pytest.mark.parametrize("shape,overlap,route", SEQ, ids=[r for _, _, r in SEQ])
def test_three_steps_sum_of_gradients(vjf, shape, overlap, route):
    lr, T = 2.0 ** -3, 3
    tag, m, (y, u, eps), ref_sum, sum32, names = case_three_steps(vjf, shape, lr, T)
    m.set_overlap(overlap)
    w0 = gc.state64(m, names)
    m.filter_sequence(y.cuda(), None if u is None else u.cuda(), None, eps=eps.cuda(), **gc.TRAIN)
    torch.cuda.synchronize()
    assert m.route() == route and m.status() == 0
    gc.compare_total(f"{tag} {route}", w0, gc.state64(m, names), ref_sum, sum32, names, lr, T)


# ------------------------------------------------------------------ 4. invariants, bit for bit
@pytest.mark.parametrize("shape,overlap", [("mega", 1), ("mega", False), ("wide", False)], ids=["mega", "mega-one-stream", "wide-one-stream"])
def test_update_without_sgd_leaves_the_trainable_tensors(vjf, shape, overlap):
    m = gc.build(vjf, shape, lr=1.0)
    m.set_overlap(overlap)
    y, u, eps = gc.inputs(shape, 37, "loud")
    names = gc.trainables(load_oracle_state(m, np.float32), with_lik=False)     # (lik_logvar: the running variance moves it)
    a = model_arrays(m)
    before = {k: a[k].clone() for k in names}
    w_mean = a["w_mean"].clone()
    m.filter_sequence(y.cuda(), None if u is None else u.cuda(), None, eps=eps.cuda(), sgd=False, update=True)
    torch.cuda.synchronize()
    assert m.status() == 0
    for k in names:
        assert torch.equal(a[k], before[k]), k
    assert not torch.equal(a["w_mean"], w_mean)                                 # (the update did run)


@pytest.mark.parametrize("overlap", [1, False], ids=["one-launch", "one-stream"])
def test_frozen_decoder_keeps_its_bits_and_the_rest_its_gradient(vjf, overlap):
    tag, m, (y, u, eps), R, names = case_step(vjf, "mega", 37, "loud", gc.TRAIN, freeze=True)
    w0, w1, st = run_step(m, R, "one-launch" if overlap else "per-step", y, u, eps, gc.TRAIN, overlap=overlap)
    assert st == 0
    for k in ("dec_W", "dec_b"):
        assert np.array_equal(w0[k], w1[k]), k
    gc.compare_step(tag + (" one-launch" if overlap else " one-stream"), w0, w1, R, [k for k in names if not k.startswith("dec_")], 1.0)
