"""CPU side of the `forecast_sequence` tests: the host logic of vjf_amd/model.py (argument coercion, the order of the draws on the CPU
generator, the scratch tensor, the n_step = 0 path) through a stand-in for the two new exports built on `oracle.forecast`, and, on
the oracle alone, the conditions that keep the GPU tests' yardstick (tests/forecast_cases.py) honest for every case."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import vjf_oracle as orc
from tests import fake_backend
from tests import forecast_cases as fc
from tests import goldenio as gio
from tests.fake_backend import _arr, _opt
from tests.helpers import load_fixture_state, load_oracle_state
from vjf_amd import _native as N

cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="the stand-in backend works on CPU tensors")


def close(a, b, **kw):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), **kw)


class ForecastLib(fake_backend.FakeLib):
    """FakeLib + vjf_forecast_scratch_size / vjf_forecast_seq: the roll-out in fp64 on the fp32 values it is handed, stored as fp32.
    Records every call's shape arguments in `calls`."""
    def __init__(self):
        super().__init__()
        self.calls = []

    def vjf_forecast_scratch_size(self, T, n, dout, out):
        if T < 1 or n < 1 or dout < 1:
            return -20
        out._obj.value = 256 * T
        return 0

    def vjf_forecast_seq(self, x0, u, wn, sn, cen, lw, w_mean, w_chol, tr_logvar, x, scratch, T, B, n, d, dout, stream):
        if any(p is None or not p.value for p in (x0, wn, cen, lw, w_mean, w_chol, x, scratch)):
            self.err = b"vjf_forecast_seq: null tensor"
            return -1
        if T < 1 or B < 1 or n < 1 or dout < 1 or d < dout:
            self.err = b"vjf_forecast_seq: bad shape"
            return -20
        du = d - dout
        self.calls.append(dict(T=T, B=B, n=n, d=d, dout=dout, u=u is not None, state_noise=sn is not None))
        s = orc.OracleState(1, dout, du, n, (1,), orc.GAUSSIAN)
        g = lambda p, *shape: _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        s.centroid, s.logwidth, s.w_mean, s.w_chol = g(cen, n, d), g(lw, n), g(w_mean, n, dout), g(w_chol, n, n)
        s.tr_logvar = g(tr_logvar, 1)[0] if sn is not None else np.float64(0)
        s.dec_W, s.dec_b = np.zeros((1, dout)), np.zeros(1)
        U = _opt(u, T * B * du)
        E = _opt(sn, T * B * dout)
        xs, _ = orc.forecast(s, g(x0, B, dout), None if U is None else U.reshape(T, B, du).astype(np.float64), T, g(wn, T, n, dout),
                             None if E is None else E.reshape(T, B, dout).astype(np.float64))
        _arr(x, (T + 1) * B * dout).reshape(T + 1, B, dout)[...] = xs
        return 0


@pytest.fixture
def fake():
    old = N._lib
    N._lib = ForecastLib()
    yield N._lib
    N._lib = old


# ---------------------------------------------------------------------------------------------------- the yardstick, on the oracle alone
@pytest.mark.parametrize("name", list(fc.CASES))
def test_the_yardstick_of_the_parity_cases(name):
    """Every case, with and without state noise: the fp64 roll-out stays bounded (|x| <= 7 here, < 100 asserted by the rule) and the
    fp32 oracle is within 1e-4 of its scale from it -- `bound` asserts both -- and the fp32 oracle's own distance is of the order the
    GPU test's docstring states (1e-6 .. 1e-5).  It guards the rule's preconditions, not the feature (it needs no native roll-out), and
    is on purpose not `cpu_only`: where a GPU is present the models live there, as in the GPU tests that rely on it."""
    import vjf_amd
    m = fc.make_model(vjf_amd, name)
    a = fc.inputs(name)
    for sn in (None, a["state_noise"]):
        (x64, y64), (x32, y32) = fc.oracles(m, a["x0"], a["u"], a["w_noise"], sn)
        assert np.abs(x64).max() <= 7
        for r64, r32 in ((x64, x32), (y64, y32)):
            b = fc.bound(r64, r32)
            assert 8 * fc.EPS32 * np.abs(r64).max() <= b < 5e-5


# ---------------------------------------------------------------------------------------------------- the host logic
@cpu_only
def test_host_recorded_rollout(fake):
    """Test 2 of the GPU file through the host layer: g8_fit's final state, recorded weight noise, recorded x and y."""
    import vjf_amd
    z = gio.load("g8_fit")
    T, B, dy, dz, du, n = [int(v) for v in z["meta"][:6]]
    hid = [int(v) for v in z["meta"][6:]]
    m = vjf_amd.VJF.make_model(dy, dz, du, n, hid, likelihood="gaussian")
    load_fixture_state(m, z, "sT")
    wn = z["fc_wnoise"]
    x, y = m.forecast_sequence(torch.tensor(z["fc_x0"]), None, wn.shape[0], w_noise=torch.tensor(wn))
    assert x.dtype == y.dtype == torch.float32 and x.shape == z["fc_x"].shape and y.shape == z["fc_y"].shape
    s32 = gio.state_from(z, "sT", ydim=dy, xdim=dz, udim=du, n_rbf=n, hidden=hid, likelihood=orc.GAUSSIAN).cast(np.float32)
    x32, y32 = orc.forecast(s32, z["fc_x0"].astype(np.float32), None, wn.shape[0], wn.astype(np.float32))
    close(x, z["fc_x"], rtol=0, atol=fc.F * fc.bound(z["fc_x"], x32))
    close(y, z["fc_y"], rtol=0, atol=fc.F * fc.bound(z["fc_y"], y32))
    assert fake.calls == [dict(T=wn.shape[0], B=z["fc_x0"].shape[0], n=n, d=dz, dout=dz, u=False, state_noise=False)]


@cpu_only
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "quiet"])
@pytest.mark.parametrize("colmajor", [True, False], ids=["after_rls", "fresh"])
def test_host_draw_order_and_generator_state(fake, colmajor, noise):
    """The draws of `forecast_sequence` are `forecast`'s: per step the weight draw (strided once an RLS update has run), then the
    state draw; the same seed gives the same roll-out and leaves the generator in the same state."""
    import vjf_amd
    xdim, udim, n, ydim, B, T = 3, 2, 9, 5, 6, 7
    torch.manual_seed(17)
    m = vjf_amd.VJF.make_model(ydim, xdim, udim, n, [4], likelihood="gaussian")
    x0, u = torch.randn(B, xdim), torch.randn(T, B, udim)
    if colmajor:
        m.filter(torch.randn(B, ydim), torch.randn(B, udim), update=True)
        assert m.transition.velocity._w_colmajor
    torch.manual_seed(99)
    xa, ya = m.forecast(x0, u, T, noise=noise)
    state_a = torch.get_rng_state()
    torch.manual_seed(99)
    xb, yb = m.forecast_sequence(x0, u, T, noise=noise)
    assert torch.equal(torch.get_rng_state(), state_a)
    assert xa.shape == xb.shape and ya.shape == yb.shape
    # (the stand-in rounds the per-step path's x to fp32 at every step and the sequence's once at the end)
    close(xb, xa, rtol=0, atol=T * 4 * fc.EPS32 * float(xa.abs().max()))
    close(yb, ya, rtol=0, atol=T * 8 * fc.EPS32 * float(ya.abs().max()))
    assert fake.calls[-1] == dict(T=T, B=B, n=n, d=xdim + udim, dout=xdim, u=True, state_noise=noise)
    # given tensors take the place of the draws: nothing is drawn when both are given, only the missing one otherwise
    wn, sn = torch.randn(T, n, xdim), torch.randn(T, B, xdim)
    before = torch.get_rng_state()
    x1 = m.transition.forecast_sequence(x0, u, T, w_noise=wn, state_noise=sn)
    assert torch.equal(torch.get_rng_state(), before) and fake.calls[-1]["state_noise"]
    s64 = load_oracle_state(m, np.float64)
    x64, _ = orc.forecast(s64, x0.numpy().astype(np.float64), u.numpy().astype(np.float64), T, wn.numpy().astype(np.float64),
                          sn.numpy().astype(np.float64))
    close(x1, x64, rtol=0, atol=2 * fc.EPS32 * float(np.abs(x64).max()))
    torch.manual_seed(5)
    m.transition.forecast_sequence(x0, u, T, w_noise=wn, noise=True)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    for _ in range(T):
        torch.randn(B, xdim)
    assert torch.equal(torch.get_rng_state(), after)


@cpu_only
def test_host_device_noise_is_one_draw_per_tensor(fake):
    import vjf_amd
    torch.manual_seed(1)
    m = vjf_amd.VJF.make_model(5, 3, 0, 9, [4], likelihood="gaussian", noise="device")
    # (where the model lives on the CPU, "the device's generator" is the CPU one: one draw per tensor, weights first, shows there)
    torch.manual_seed(2)
    x, y = m.forecast_sequence(torch.zeros(4, 3), None, 6, noise=True)
    after = torch.get_rng_state()
    assert x.shape == (7, 4, 3) and y.shape == (7, 4, 5) and fake.calls[-1]["state_noise"]
    torch.manual_seed(2)
    torch.randn(6, 9, 3), torch.randn(6, 4, 3)
    assert torch.equal(torch.get_rng_state(), after)


@cpu_only
def test_host_argument_coercion(fake):
    import vjf_amd
    xdim, udim, n, ydim, B, T = 3, 2, 9, 5, 6, 7
    torch.manual_seed(3)
    m = vjf_amd.VJF.make_model(ydim, xdim, udim, n, [4], likelihood="gaussian")
    x0, u, wn = torch.randn(B, xdim), torch.randn(T, B, udim), torch.randn(T, n, xdim)
    # n_step = 0: x0 itself and its decoding, no native roll-out
    x, y = m.forecast_sequence(x0, u[:0], 0)
    assert fake.calls == [] and x.shape == (1, B, xdim) and y.shape == (1, B, ydim)
    assert torch.equal(x[0], x0)
    close(y[0], x0.numpy().astype(np.float64) @ m.decoder.decode.weight.detach().numpy().astype(np.float64).T + m.decoder.decode.bias.detach().numpy(),
          rtol=0, atol=1e-6)
    # float64 / numpy / strided inputs, a 1-D x0 with u lacking its batch axis
    full = m.transition.forecast_sequence(x0.double().numpy(), u.double(), T, w_noise=wn.double())
    assert full.dtype == torch.float32 and full.shape == (T + 1, B, xdim)
    one = m.transition.forecast_sequence(x0[4], u[:, 4], T, w_noise=wn)
    assert one.shape == (T + 1, 1, xdim)
    close(one[:, 0], full[:, 4], rtol=0, atol=2 * fc.EPS32 * float(full.abs().max()))
    assert fake.calls[-1]["B"] == 1
    # the scratch tensor is kept and grown on demand
    s = m.transition._fc_scratch
    m.transition.forecast_sequence(x0, u[:3], 3, w_noise=wn[:3])
    assert m.transition._fc_scratch is s
    m.transition.forecast_sequence(x0, torch.randn(2 * T, B, udim), 2 * T, w_noise=torch.randn(2 * T, n, xdim))
    assert m.transition._fc_scratch is not s and m.transition._fc_scratch.numel() >= 256 * 2 * T
    # refusals
    with pytest.raises(TypeError):
        m.forecast_sequence(x0, None, T)
    with pytest.raises(AssertionError):
        m.forecast_sequence(x0, u, T, w_noise=wn[:, :-1])
    with pytest.raises(AssertionError):
        m.forecast_sequence(x0, u, T, w_noise=wn[:-1])
    with pytest.raises(AssertionError):
        m.forecast_sequence(x0, u, T, state_noise=torch.randn(T, B + 1, xdim))
    with pytest.raises(AssertionError):
        m.forecast_sequence(x0, u[:-1], T)
    with pytest.raises(AssertionError):
        m.forecast_sequence(x0[:, :-1], u, T)
    # the stand-in's own refusals mirror the library's codes
    assert fake.vjf_forecast_seq(None, None, None, None, None, None, None, None, None, None, None, 1, 1, 1, 1, 1, None) == -1
    p = C.c_void_p(8)
    assert fake.vjf_forecast_seq(p, None, p, None, p, p, p, p, p, p, p, 0, 1, 1, 1, 1, None) == -20
