"""Recognition activations other than Tanh (vjf/recognition.py:17-24), without a GPU: the module -> vjf_activation mapping and the
refusals, the numpy oracle pinned to the reference's g9_act_* fixtures, and the C ABI's argument checks."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
from torch import nn

from tests import act_oracle as ao
from tests import goldenio as gio

TRAJ = sorted(p[:-4] for p in os.listdir(gio.GOLDEN) if p.startswith("g9_act_") and p.endswith(".npz") and "recognition" not in p)


def close(a, b, **kw):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), **kw)


# ---------------------------------------------------------------------------------------------------- mapping and refusals
SUPPORTED = [
    (nn.Tanh, (0, 0.0, 0.0)),
    (nn.ReLU, (1, 0.0, 0.0)),
    (functools.partial(nn.ReLU, inplace=True), (1, 0.0, 0.0)),
    (nn.LeakyReLU, (2, 0.01, 0.0)),
    (functools.partial(nn.LeakyReLU, 0.2), (2, 0.2, 0.0)),
    (functools.partial(nn.LeakyReLU, 0.0), (2, 0.0, 0.0)),
    (nn.ELU, (3, 1.0, 0.0)),
    (functools.partial(nn.ELU, 0.5), (3, 0.5, 0.0)),
    (nn.Softplus, (4, 1.0, 20.0)),
    (functools.partial(nn.Softplus, beta=2), (4, 2.0, 20.0)),
    (functools.partial(nn.Softplus, beta=0.5, threshold=30), (4, 0.5, 30.0)),
    (nn.Sigmoid, (5, 0.0, 0.0)),
    (nn.Hardtanh, (6, -1.0, 1.0)),
    (functools.partial(nn.Hardtanh, -2.0, 0.5), (6, -2.0, 0.5)),
    (nn.ReLU6, (6, 0.0, 6.0)),
    pytest.param(lambda: nn.ReLU(), (1, 0.0, 0.0), id="lambda-ReLU"),     # (a fixed id: the repr of a lambda holds its address)
]


class MyReLU(nn.ReLU):
    pass


REFUSED = [nn.GELU, nn.SiLU, nn.Mish, nn.Tanhshrink, nn.SELU, nn.CELU, nn.PReLU, nn.Identity, MyReLU,
           functools.partial(nn.LeakyReLU, -0.1), functools.partial(nn.ELU, 0.0), functools.partial(nn.ELU, -1.0),
           functools.partial(nn.Softplus, beta=0.0), functools.partial(nn.Softplus, beta=-1.0),
           functools.partial(nn.Softplus, threshold=10)]          # (torch itself refuses Hardtanh(min_val >= max_val))


@pytest.mark.parametrize("act,code", SUPPORTED, ids=lambda x: repr(x)[:60])
def test_supported_activation_maps_to_its_code(act, code):
    from vjf_amd.recognition import Recognition, activation_code
    assert activation_code(act()) == pytest.approx(code)
    r = Recognition(10, 3, 2, [8, 5], activation=act)
    assert r.act_code == pytest.approx(code)
    a = r.activation()
    assert (a.kind, a.p0, a.p1) == pytest.approx(code)
    assert isinstance(r.mlp[1], nn.Module) and isinstance(r.mlp[3], nn.Module)     # (the modules stay in mlp, as the reference's)


@pytest.mark.parametrize("act", REFUSED, ids=lambda x: repr(x)[:60])
def test_refused_activation_names_the_supported_set(act):
    from vjf_amd.recognition import Recognition
    with pytest.raises(NotImplementedError, match="supported: Tanh, ReLU, LeakyReLU"):
        Recognition(10, 3, 0, [8], activation=act)


def test_one_activation_for_every_layer():
    from vjf_amd.recognition import Recognition
    it = iter([nn.ReLU(), nn.Sigmoid()])
    with pytest.raises(NotImplementedError, match="one activation"):
        Recognition(10, 3, 0, [8, 8], activation=lambda: next(it))


def test_relu_model_builds_with_reference_weights_and_keys():
    """VJF with a ReLU recognition network: construction no longer raises, the state_dict keys and the seeded initial weights are
    the Tanh model's (activation modules hold no parameters and draw no random numbers)."""
    from vjf_amd import VJF
    from vjf_amd.likelihood import GaussianLikelihood
    from vjf_amd.model import RBFDS
    from vjf_amd.recognition import Recognition
    torch.manual_seed(3)
    m_tanh = VJF(10, 3, GaussianLikelihood(), RBFDS(16, 3, 0), Recognition(10, 3, 0, [8, 8]), lr=1e-3)
    torch.manual_seed(3)
    m_relu = VJF(10, 3, GaussianLikelihood(), RBFDS(16, 3, 0), Recognition(10, 3, 0, [8, 8], activation=nn.ReLU), lr=1e-3)
    a, b = m_tanh.state_dict(), m_relu.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    assert m_relu.recognition.act_code == (1, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------------- the oracle vs the reference
def run_traj(name):
    z, info, s = gio.traj_case(name)
    act = ao.act_of(z)
    u = z["u"] if info["du"] else None
    outs = []
    for t in range(info["T"]):
        mu = outs[-1].mu_t if outs else None
        lv = outs[-1].lv_t if outs else None
        o = ao.filter_step(s, act, z["y"][t], None if u is None else u[t], mu, lv, z["eps"][t, 0], z["eps"][t, 1],
                           sgd=True, update=True, warm_up=info["warm_up"])
        o.rho = float(s.lik_logvar) if s.lik_logvar is not None else 0.0
        o.sigma = float(s.tr_logvar)
        outs.append(o)
    return z, info, s, outs


def test_fixture_set():
    assert len([n for n in TRAJ if n.endswith("_f32")]) >= 12 and len([n for n in TRAJ if n.endswith("_f64")]) >= 12
    kinds = {ao.act_of(gio.load(n)) for n in TRAJ}
    assert {k[0] for k in kinds} == {ao.RELU, ao.LEAKY_RELU, ao.ELU, ao.SOFTPLUS, ao.SIGMOID, ao.HARDTANH}
    assert (ao.HARDTANH, 0.0, 6.0) in kinds                                                           # ReLU6


@pytest.mark.parametrize("name", [n for n in TRAJ if n.endswith("_f64")])
def test_act_oracle_trajectory_f64(name):
    z, info, s, outs = run_traj(name)
    for t, o in enumerate(outs):
        close(o.mu_t, z["out.mu"][t], rtol=1e-8, atol=1e-10)
        close(o.lv_t, z["out.lv"][t], rtol=1e-8, atol=1e-10)
        close([o.loss, o.recon, o.dyn, o.entropy], z["out.loss"][t], rtol=1e-9, atol=1e-10)
        close(o.rho, z["out.rho"][t], rtol=1e-9, atol=1e-10)
        close(o.sigma, z["out.sigma"][t], rtol=1e-8, atol=1e-10)
    for k, v in gio.state_arrays(s).items():
        close(v, z[f"sT.{k}"], rtol=1e-6, atol=1e-9)
    # the recognition weights moved (the derivative is exercised)
    assert np.abs(z["sT.rec_W0"] - z["s0.rec_W0"]).max() > 1e-4


@pytest.mark.parametrize("name", [n for n in TRAJ if n.endswith("_f32")])
def test_act_oracle_trajectory_f32(name):
    z, info, s, outs = run_traj(name)
    assert s.dtype == np.float32
    for t, o in enumerate(outs):
        close(o.mu_t, z["out.mu"][t], rtol=2e-5, atol=2e-5)
        close(o.lv_t, z["out.lv"][t], rtol=2e-5, atol=2e-5)
        close([o.loss, o.recon, o.dyn, o.entropy], z["out.loss"][t], rtol=2e-5, atol=2e-5)
        close(o.sigma, z["out.sigma"][t], rtol=0, atol=2e-5)
        close(o.rho, z["out.rho"][t], rtol=0, atol=2e-5)
    close(s.w_mean, z["sT.w_mean"], rtol=1e-3, atol=2e-5)
    close(s.w_precision, z["sT.w_precision"], rtol=1e-4, atol=1e-4)
    close(s.w_chol, z["sT.w_chol"], rtol=1e-3, atol=2e-5)
    for k in ("mean_W", "lv_W", "lv_b", "dec_W", "dec_b", "rec_W0", "rec_b0"):
        close(gio.state_arrays(s)[k], z[f"sT.{k}"], rtol=1e-4, atol=1e-5)


def test_act_oracle_recognition():
    z = gio.load("g9_act_recognition")
    for i in range(int(z["count"])):
        dy, dz, du, B, *hid = [int(v) for v in z[f"{i}.meta"]]

        class S:
            rec_W = [z[f"{i}.rec_W{k}"] for k in range(len(hid))]
            rec_b = [z[f"{i}.rec_b{k}"] for k in range(len(hid))]
            mean_W, lv_W, lv_b = z[f"{i}.mean_W"], z[f"{i}.lv_W"], z[f"{i}.lv_b"]
        mu, lv = ao.recognition_forward(S, ao.act_of(z, f"{i}."), z[f"{i}.y"], z[f"{i}.mu"], z[f"{i}.lv"], z[f"{i}.u"])
        close(mu, z[f"{i}.out_mu"], rtol=1e-10, atol=1e-12)
        close(lv, z[f"{i}.out_lv"], rtol=1e-10, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- C ABI argument checks
BAD = [(7, 0.0, 0.0), (-1, 0.0, 0.0), (2, -0.1, 0.0), (2, float("nan"), 0.0), (3, 0.0, 0.0), (4, 0.0, 20.0), (4, 1.0, 19.5),
       (4, 1.0, float("nan")), (6, 1.0, 1.0), (6, 2.0, -2.0), (6, float("-inf"), 1.0)]


@pytest.mark.parametrize("bad", BAD)
def test_abi_rejects_bad_activation_before_any_device_call(bad):
    from vjf_amd import _native as N
    L = N.lib()
    a = N.VjfActivation(*bad)
    assert L.vjf_set_activation(None, C.byref(a)) < 0
    assert b"vjf_set_activation" in L.vjf_last_error()
    hid = (C.c_int32 * 1)(8)
    W = (C.c_void_p * 1)(None)
    rc = L.vjf_recognition_forward_act(None, None, None, None, W, W, None, None, None, None, None, 4, 10, 0, 3, 1, hid, C.byref(a), None)
    assert rc < 0
    assert b"vjf_recognition_forward_act" in L.vjf_last_error() and b"null tensor" not in L.vjf_last_error()


def test_abi_accepts_good_activation_arguments():
    """A valid activation passes the checks and then fails on the null context / null tensors (nothing reaches the device)."""
    from vjf_amd import _native as N
    L = N.lib()
    for kind, p0, p1 in [(0, 0, 0), (1, 0, 0), (2, 0.2, 0), (3, 0.5, 0), (4, 2.0, 20.0), (5, 0, 0), (6, 0.0, 6.0)]:
        a = N.VjfActivation(kind, p0, p1)
        assert L.vjf_set_activation(None, C.byref(a)) < 0 and b"null context" in L.vjf_last_error()
        hid = (C.c_int32 * 1)(8)
        W = (C.c_void_p * 1)(None)
        assert L.vjf_recognition_forward_act(None, None, None, None, W, W, None, None, None, None, None, 4, 10, 0, 3, 1, hid,
                                             C.byref(a), None) < 0
        assert b"null tensor" in L.vjf_last_error()
