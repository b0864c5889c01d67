"""Recognition activations other than Tanh on every filter route (vjf_set_activation; the act kernels: vjf_mega_act_kernel,
vjf_mega_lite_act_kernel, vjf_trial_mfma_act_kernel, the wide route's element-wise pass, vjf_recognition_act_kernel), against the
reference's g9_act_* fixtures and the fp64 restatement tests/act_oracle.py.  Tolerances are those of the Tanh tests
(tests/test_gpu_parity.py, tests/test_gpu_configs.py); the achieved margins are recorded (tests/margins.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
from torch import nn

from tests import act_oracle as ao
from tests import goldenio as gio
from tests.helpers import load_fixture_state, load_oracle_state, model_arrays, state_close
from tests.margins import check_close

pytestmark = pytest.mark.gpu

POST = dict(rtol=1e-6, atol=1e-6)
G9 = sorted(p[:-4] for p in os.listdir(gio.GOLDEN) if p.startswith("g9_act_") and p.endswith("_f32.npz"))


def close(a, b, **kw):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    check_close(np.asarray(a, np.float64), np.asarray(b, np.float64), **kw)


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


def act_class(name, p):
    """The `activation` argument for a fixture's recorded activation."""
    return {"ReLU": nn.ReLU, "ReLU6": nn.ReLU6, "Sigmoid": nn.Sigmoid, "Tanh": nn.Tanh,
            "LeakyReLU": functools.partial(nn.LeakyReLU, float(p[0])), "ELU": functools.partial(nn.ELU, float(p[0])),
            "Softplus": functools.partial(nn.Softplus, beta=float(p[0]), threshold=float(p[1])),
            "Hardtanh": functools.partial(nn.Hardtanh, float(p[0]), float(p[1]))}[name]


def make(vjf, dy, dz, du, n, hidden, lik, lr, act):
    from vjf_amd.likelihood import GaussianLikelihood, PoissonLikelihood
    from vjf_amd.model import RBFDS
    from vjf_amd.recognition import Recognition
    likelihood = PoissonLikelihood() if lik == "poisson" else GaussianLikelihood()
    return vjf.VJF(dy, dz, likelihood, RBFDS(n, dz, du), Recognition(dy, dz, du, hidden, activation=act), lr=lr)


def model_for(vjf, z, info):
    m = make(vjf, info["dy"], info["dz"], info["du"], info["n"], info["hidden"], info["lik"], 1e-4,
             act_class(str(z["act"]), z["act_params"]))
    load_fixture_state(m, z, "s0")
    return m


# ------------------------------------------------------------------ a. the fixtures through filter, on each route
@pytest.mark.parametrize("overlap", [1, 0, 3], ids=["one-launch", "one-stream", "three-stream"])
@pytest.mark.parametrize("name", G9)
def test_act_trajectory_golden(vjf, name, overlap):
    z, info, _ = gio.traj_case(name)
    model = model_for(vjf, z, info)
    if overlap != 1:
        model.set_overlap(overlap)
    u = z["u"] if info["du"] else None
    q = None
    for t in range(info["T"]):
        ut = None if u is None else torch.tensor(u[t])
        q, loss, *comp = model.filter(torch.tensor(z["y"][t]), ut, q, sgd=True, update=True, verbose=True,
                                      warm_up=info["warm_up"], eps=(torch.tensor(z["eps"][t, 0]), torch.tensor(z["eps"][t, 1])))
        close(q.mean, z["out.mu"][t], **POST)
        close(q.logvar, z["out.lv"][t], **POST)
        close(torch.stack([loss, *comp]), z["out.loss"][t], rtol=1e-6, atol=1e-6)
        close(model.transition.logvar, z["out.sigma"][t], rtol=0, atol=1e-6)
        if info["lik"] == "gaussian":
            close(model.likelihood.logvar, z["out.rho"][t], rtol=0, atol=1e-6)
    state_close(model, z, prefix="sT", rtol=5e-6, atol=1e-6, rls_rtol=5e-4, rls_atol=5e-6)
    want = {1: "one-launch", 0: "per-step", 3: "per-step" if info["warm_up"] else "streams"}[overlap]
    assert model.route(warm_up=info["warm_up"]) == want
    assert model.status() == 0


# ------------------------------------------------------------------ b. filter_sequence == stepwise filter
@pytest.mark.parametrize("name", ["g9_act_relu_gaussian_f32", "g9_act_softplus2_gaussian_f32", "g9_act_hardtanh_gaussian_f32"])
def test_act_sequence_equals_steps(vjf, name):
    z, info, _ = gio.traj_case(name)
    m1, m2 = model_for(vjf, z, info), model_for(vjf, z, info)
    mu, lv, loss = m1.filter_sequence(torch.tensor(z["y"]), None, None, eps=torch.tensor(z["eps"]))
    q = None
    for t in range(info["T"]):
        q, l, *c = m2.filter(torch.tensor(z["y"][t]), None, q, verbose=True, eps=(torch.tensor(z["eps"][t, 0]), torch.tensor(z["eps"][t, 1])))
        assert torch.equal(q.mean, mu[t]) and torch.equal(q.logvar, lv[t])      # same kernels, same order: bitwise
        assert torch.equal(torch.stack([l, *c]), loss[t])
    assert torch.equal(m1._blob, m2._blob)
    close(mu, z["out.mu"], **POST)


# ------------------------------------------------------------------ c. stand-alone Recognition.forward
def test_act_recognition_golden(vjf):
    z = gio.load("g9_act_recognition")
    for i in range(int(z["count"])):
        dy, dz, du, B, *hid = [int(v) for v in z[f"{i}.meta"]]
        r = vjf.recognition.Recognition(dy, dz, du, hid, activation=act_class(str(z[f"{i}.act"]), z[f"{i}.act_params"]))
        for k, lin in enumerate(r.linears()):
            lin.weight.copy_(torch.tensor(z[f"{i}.rec_W{k}"]))
            lin.bias.copy_(torch.tensor(z[f"{i}.rec_b{k}"]))
        r.mean.weight.copy_(torch.tensor(z[f"{i}.mean_W"]))
        r.logvar.weight.copy_(torch.tensor(z[f"{i}.lv_W"]))
        r.logvar.bias.copy_(torch.tensor(z[f"{i}.lv_b"]))
        q = r(torch.tensor(z[f"{i}.y"]), vjf.Gaussian(torch.tensor(z[f"{i}.mu"]), torch.tensor(z[f"{i}.lv"])), torch.tensor(z[f"{i}.u"]))
        close(q.mean, z[f"{i}.out_mu"], rtol=2e-6, atol=1e-6)
        close(q.logvar, z[f"{i}.out_lv"], rtol=2e-6, atol=1e-6)


# ------------------------------------------------------------------ d. configs[1] size: one launch vs per-step kernels, and the oracle
def _data(B, dy, dz, T, seed, du=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(T, B, dy, generator=g)
    u = torch.randn(T, B, du, generator=g) if du else None
    eps = torch.randn(T, 2, B, dz, generator=g)
    return y, u, eps


def _oracle_steps(s, act, y, u, eps, T, mu0=None, lv0=None, **flags):
    outs, om, ol = [], mu0, lv0
    for t in range(T):
        o = ao.filter_step(s, act, y[t].numpy(), None if u is None else u[t].numpy(), om, ol, eps[t, 0].numpy(), eps[t, 1].numpy(),
                           **flags)
        om, ol = o.mu_t, o.lv_t
        outs.append(o)
    return outs


@pytest.mark.parametrize("act", [nn.ReLU, nn.Softplus], ids=["ReLU", "Softplus"])
def test_act_config_b_one_launch_vs_per_step_and_oracle(vjf, act):
    B, dz, dy, n, hid = 4096, 10, 50, 200, [128]
    torch.manual_seed(11)
    m1 = make(vjf, dy, dz, 0, n, hid, "gaussian", 1e-3, act)
    torch.manual_seed(11)
    m2 = make(vjf, dy, dz, 0, n, hid, "gaussian", 1e-3, act)
    torch.manual_seed(11)
    m3 = make(vjf, dy, dz, 0, n, hid, "gaussian", 1e-3, act)
    s = load_oracle_state(m3, np.float64)
    m2.set_overlap(False)
    y, _, eps = _data(B, dy, dz, 20, 21)
    yd, ed = y.cuda(), eps.cuda()
    o1 = m1.filter_sequence(yd, eps=ed)
    o2 = m2.filter_sequence(yd, eps=ed)
    assert m1.route() == "one-launch" and m2.route() == "per-step"
    for a, b in zip(o1, o2):
        close(a, b, rtol=1e-6, atol=1e-6)
    # the state: test_filter_sequence_one_launch_vs_per_step_kernels compares the whole blob at rtol 1e-4 over 6 steps of 256 trials;
    # over 20 steps of 4096 the RLS factors' conditioning carries the two summation orders further apart (a few elements of
    # w_chol / w_pchol at 1e-3 relative, 2e-5 absolute, for a smooth activation as for ReLU): those four tensors at the RLS
    # tolerance of the oracle comparisons at this size (test_sequence_at_bench_size_bitwise_and_oracle), everything else as there
    a1, a2 = model_arrays(m1), model_arrays(m2)
    for k in a1:
        rls = k in ("w_mean", "w_chol", "w_precision", "w_pchol")
        close(a1[k], a2[k], rtol=5e-3 if rls else 1e-4, atol=5e-5 if rls else 1e-6)
    assert m1.status() == 0 and m2.status() == 0
    mu, lv, ls = m3.filter_sequence(yd[:3], eps=ed[:3])
    kind = m3.recognition.act_code
    for t, o in enumerate(_oracle_steps(s, kind, y, None, eps, 3)):
        close(mu[t], o.mu_t, rtol=1e-6, atol=1e-6)
        close(lv[t], o.lv_t, rtol=1e-6, atol=1e-6)
        close(ls[t], [o.loss, o.recon, o.dyn, o.entropy], rtol=1e-6, atol=1e-6)
    state_close(m3, s, rtol=5e-6, atol=1e-6, rls_rtol=5e-3, rls_atol=5e-5)


# ------------------------------------------------------------------ e. the flag sets without an RLS update (lite act kernel)
@pytest.mark.parametrize("flags", [dict(warm_up=True), dict(sgd=False, update=False), dict(update=False)],
                         ids=["warm_up", "deployed", "no_update"])
@pytest.mark.parametrize("act", [functools.partial(nn.ELU, 0.5), nn.Sigmoid], ids=["ELU", "Sigmoid"])
def test_act_lite_flag_sets_vs_oracle(vjf, act, flags):
    B, dz, dy, du, n, hid = 48, 4, 12, 1, 40, [16, 16]
    torch.manual_seed(5)
    m = make(vjf, dy, dz, du, n, hid, "gaussian", 1e-2, act)
    s = load_oracle_state(m, np.float64)
    y, u, eps = _data(B, dy, dz, 4, 7, du)
    mu, lv, ls = m.filter_sequence(y, u, None, eps=eps, **flags)
    assert m.route(**flags) == "one-launch"
    full = dict(sgd=True, update=True, warm_up=False)
    full.update(flags)
    for t, o in enumerate(_oracle_steps(s, m.recognition.act_code, y, u, eps, 4, **full)):
        close(mu[t], o.mu_t, rtol=5e-6, atol=5e-6)
        close(lv[t], o.lv_t, rtol=5e-6, atol=5e-6)
        close(ls[t], [o.loss, o.recon, o.dyn, o.entropy], rtol=5e-6, atol=5e-6)
    state_close(m, s, rtol=5e-5, atol=5e-6, rls_rtol=5e-3, rls_atol=5e-5)
    assert m.status() == 0


# ------------------------------------------------------------------ f. the wide route (trial working set beyond LDS)
def test_act_wide_route_vs_oracle(vjf):
    B, dz, dy, n, hid = 64, 64, 512, 64, [512, 512]
    torch.manual_seed(12)
    m = make(vjf, dy, dz, 0, n, hid, "gaussian", 1e-3, functools.partial(nn.LeakyReLU, 0.2))
    r = float(np.sqrt(dz))                       # (as test_gpu_configs: the default RBF init underflows every feature at d_z = 64)
    m.transition.velocity.feature.centroid.uniform_(-r, r)
    m.transition.velocity.feature.logwidth.fill_(float(np.log(r)))
    s = load_oracle_state(m, np.float64)
    y, _, eps = _data(B, dy, dz, 3, 22)
    q = None
    outs = _oracle_steps(s, m.recognition.act_code, y, None, eps, 3)
    for t in range(2):
        q, loss, *comp = m.filter(y[t], None, q, verbose=True, eps=(eps[t, 0], eps[t, 1]))
        close(q.mean, outs[t].mu_t, rtol=1e-6, atol=1e-6)
        close(q.logvar, outs[t].lv_t, rtol=1e-6, atol=1e-6)
        close(torch.stack([loss, *comp]), [outs[t].loss, outs[t].recon, outs[t].dyn, outs[t].entropy], rtol=1e-6, atol=1e-6)
    mu, lv, ls = m.filter_sequence(y[2:], qs=q, eps=eps[2:])
    close(mu[0], outs[2].mu_t, rtol=1e-6, atol=1e-6)
    close(ls[0], [outs[2].loss, outs[2].recon, outs[2].dyn, outs[2].entropy], rtol=1e-6, atol=1e-6)
    state_close(m, s, rtol=5e-6, atol=1e-6, rls_rtol=5e-5, rls_atol=5e-5)
    assert m.status() == 0


# ------------------------------------------------------------------ g. a Tanh and a ReLU context interleaved on two streams
def test_tanh_and_relu_contexts_interleaved(vjf):
    B, dz, dy, n, hid = 256, 10, 50, 200, [128]
    y, _, eps = _data(B, dy, dz, 6, 31)
    yd, ed = y.cuda(), eps.cuda()

    def pair():
        torch.manual_seed(3)
        a = make(vjf, dy, dz, 0, n, hid, "gaussian", 1e-3, nn.Tanh)
        torch.manual_seed(3)
        b = make(vjf, dy, dz, 0, n, hid, "gaussian", 1e-3, nn.ReLU)
        return a, b
    def run(m, k, prev):
        return m.filter_sequence(yd[k:k + 2], qs=None if prev is None else vjf.Gaussian(prev[0][-1], prev[1][-1]), eps=ed[k:k + 2])
    alone = []
    for m in pair():
        o = []
        for k in (0, 2, 4):
            o.append(run(m, k, o[-1] if o else None))
        torch.cuda.synchronize()
        alone.append(([t.clone() for r in o for t in r], m._blob.clone(), m.route()))
    a, b = pair()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    oa, ob = [], []
    for k in (0, 2, 4):
        with torch.cuda.stream(s1):
            oa.append(run(a, k, oa[-1] if oa else None))
        with torch.cuda.stream(s2):
            ob.append(run(b, k, ob[-1] if ob else None))
    torch.cuda.synchronize()
    for (want, blob, route), got, m in zip(alone, (oa, ob), (a, b)):
        assert route == "one-launch" and m.route() == "one-launch"
        got = [t for r in got for t in r]
        assert all(torch.equal(x, w) for x, w in zip(got, want))
        assert torch.equal(m._blob, blob)
        assert m.status() == 0
    assert not torch.equal(alone[0][1], alone[1][1])          # (the two activations do give different models)


# ------------------------------------------------------------------ h. vjf_filter_local + vjf_filter_global == vjf_filter_step
def test_act_local_global_equals_step(vjf):
    from vjf_amd import _native as N
    B, dz, dy, n, hid = 512, 6, 20, 64, [32, 32]
    act = functools.partial(nn.Hardtanh, -0.5, 0.5)
    torch.manual_seed(9)
    m1 = make(vjf, dy, dz, 0, n, hid, "gaussian", 1e-2, act)
    torch.manual_seed(9)
    m2 = make(vjf, dy, dz, 0, n, hid, "gaussian", 1e-2, act)
    m1.set_overlap(False)
    y, _, eps = _data(B, dy, dz, 2, 41)
    yd, ed = y.cuda(), eps.cuda()
    q, loss, *comp = m1.filter(yd[0], None, None, verbose=True, eps=(ed[0, 0], ed[0, 1]))
    m2._ensure_ctx(B)
    m2._push_lr()
    L, ctx = m2._backend(), m2._ctx
    flags = N.FLAG_SGD | N.FLAG_UPDATE
    mu = torch.empty(B, dz, device="cuda"); lv = torch.empty(B, dz, device="cuda"); loss4 = torch.empty(4, device="cuda")
    N.check(L.vjf_set_stream(ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    N.check(L.vjf_filter_local(ctx, B, N.ptr(yd[0]), None, None, None, N.ptr(ed[0, 0]), N.ptr(ed[0, 1]), N.ptr(mu), N.ptr(lv), flags))
    N.check(L.vjf_filter_global(ctx, B, N.ptr(loss4), flags))
    torch.cuda.synchronize()
    close(mu, q.mean, rtol=1e-6, atol=1e-6)
    close(lv, q.logvar, rtol=1e-6, atol=1e-6)
    close(loss4, torch.stack([loss, *comp]), rtol=1e-6, atol=1e-6)
    close(m2._blob, m1._blob, rtol=1e-5, atol=1e-6)
    # the activation is structure: once a context has run, it is not changed under it
    a = N.VjfActivation(N.ACT_RELU, 0.0, 0.0)
    assert L.vjf_set_activation(ctx, C.byref(a)) < 0 and b"already run" in L.vjf_last_error()


# ------------------------------------------------------------------ i. Tanh passed explicitly == the default model
def test_explicit_tanh_is_the_default(vjf):
    B, dz, dy, n, hid = 64, 4, 12, 40, [16]
    y, _, eps = _data(B, dy, dz, 4, 51)
    outs = []
    for explicit in (False, True):
        torch.manual_seed(2)
        if explicit:
            m = make(vjf, dy, dz, 0, n, hid, "gaussian", 1e-3, nn.Tanh)
        else:
            m = vjf.VJF.make_model(dy, dz, 0, n, hid, likelihood="gaussian", lr=1e-3)
        outs.append((m.filter_sequence(y, None, None, eps=eps), m._blob.clone()))
    (a, ba), (b, bb) = outs
    assert all(torch.equal(x, w) for x, w in zip(a, b)) and torch.equal(ba, bb)
