"""CPU side of the `forecast_ensemble` tests: the host logic of vjf_amd/model.py (the order of the draws on the CPU generator, the
Gaussian start, argument coercion, the scratch tensor, the n_step = 0 path, the refusals) through a stand-in for the exports built on
`oracle.forecast` in fp64, and, on the oracle alone, the conditions that keep the GPU tests' yardstick (tests/ensemble_cases.py)
honest for every case and mode the GPU file uses."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import vjf_oracle as orc
from tests import ensemble_cases as ec
from tests import fake_backend
from tests import forecast_cases as fc
from tests.fake_backend import _arr
from vjf_amd import _native as N

cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="the stand-in backend works on CPU tensors")


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class EnsembleLib(fake_backend.FakeLib):
    """FakeLib + the forecast exports: vjf_forecast_seq and vjf_forecast_ens roll out in fp64 (oracle.forecast) on the fp32 values they
    are handed and store fp32; the ensemble's moments are np.mean / np.var of the fp64 members.  Records every ensemble call's
    arguments in `calls`."""
    def __init__(self):
        super().__init__()
        self.calls = []

    @staticmethod
    def _fc_state(cen, lw, w_mean, w_chol, tr_logvar, noisy, n, d, dout):
        s = orc.OracleState(1, dout, d - dout, n, (1,), orc.GAUSSIAN)
        g = lambda p, *shape: _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        s.centroid, s.logwidth, s.w_mean, s.w_chol = g(cen, n, d), g(lw, n), g(w_mean, n, dout), g(w_chol, n, n)
        s.tr_logvar = g(tr_logvar, 1)[0] if noisy else np.float64(0)
        s.dec_W, s.dec_b = np.zeros((1, dout)), np.zeros(1)
        return s

    def vjf_forecast_scratch_size(self, T, n, dout, out):
        if T < 1 or n < 1 or dout < 1:
            return -20
        out._obj.value = 256 * T
        return 0

    def vjf_forecast_seq(self, x0, u, wn, sn, cen, lw, w_mean, w_chol, tr_logvar, x, scratch, T, B, n, d, dout, stream):
        du = d - dout
        s = self._fc_state(cen, lw, w_mean, w_chol, tr_logvar, sn is not None, n, d, dout)
        f = lambda p, *shape: None if p is None else _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        xs, _ = orc.forecast(s, f(x0, B, dout), f(u, T, B, du), T, f(wn, T, n, dout), f(sn, T, B, dout))
        _arr(x, (T + 1) * B * dout).reshape(T + 1, B, dout)[...] = xs
        return 0

    def vjf_forecast_ens_scratch_size(self, T, S, B, n, dout, out):
        if T < 0 or S < 1 or B < 1 or n < 1 or dout < 1:
            return -20
        out._obj.value = 256 * (T + 1) * S
        return 0

    def vjf_forecast_ens(self, x0, x0_ms, u, wn, sn, cen, lw, w_mean, w_chol, tr_logvar, dec_W, dec_b, x_mean, x_var, y_mean, y_var,
                         x_members, scratch, T, S, B, n, d, dout, dy, stream):
        null = lambda p: p is None or not p.value                                                 # noqa: E731
        if any(null(p) for p in (x0, cen, lw, w_mean, w_chol, x_mean, x_var, scratch)) or (T > 0 and null(wn)):
            self.err = b"vjf_forecast_ens: null tensor"
            return -1
        if T < 0 or S < 1 or B < 1 or n < 1 or dout < 1 or d < dout or x0_ms not in (0, B * dout):
            self.err = b"vjf_forecast_ens: bad shape"
            return -20
        du = d - dout
        if du > 0 and null(u) and T > 0:
            self.err = b"vjf_forecast_ens: u is required when d > dout"
            return -21
        self.calls.append(dict(T=T, S=S, B=B, n=n, d=d, dout=dout, dy=0 if null(dec_W) else dy, x0_ms=x0_ms, u=not null(u),
                               state_noise=not null(sn), members=not null(x_members)))
        s = self._fc_state(cen, lw, w_mean, w_chol, tr_logvar, not null(sn), n, d, dout)
        f = lambda p, *shape: _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        starts = f(x0, S if x0_ms else 1, B, dout)
        U = None if null(u) or T == 0 else f(u, T, B, du)
        WN = f(wn, S, T, n, dout) if T > 0 else np.zeros((S, 0, n, dout))
        E = None if null(sn) or T == 0 else f(sn, S, T, B, dout)
        xs = np.stack([orc.forecast(s, starts[m if x0_ms else 0], U, T, WN[m], None if E is None else E[m])[0] for m in range(S)])
        if not null(x_members) and T > 0:
            _arr(x_members, xs.size).reshape(xs.shape)[...] = xs
        _arr(x_mean, (T + 1) * B * dout).reshape(T + 1, B, dout)[...] = xs.mean(0)
        _arr(x_var, (T + 1) * B * dout).reshape(T + 1, B, dout)[...] = xs.var(0)
        if not null(dec_W):
            ys = xs @ f(dec_W, dy, dout).T + f(dec_b, dy)
            _arr(y_mean, (T + 1) * B * dy).reshape(T + 1, B, dy)[...] = ys.mean(0)
            _arr(y_var, (T + 1) * B * dy).reshape(T + 1, B, dy)[...] = ys.var(0)
        return 0


@pytest.fixture
def fake():
    old = N._lib
    N._lib = EnsembleLib()
    yield N._lib
    N._lib = old


SMALL = dict(xdim=3, udim=2, n=9, ydim=5, B=6, T=7, S=3)


def small_model(seed=17, **kw):
    import vjf_amd
    c = SMALL
    torch.manual_seed(seed)
    return vjf_amd.VJF.make_model(c["ydim"], c["xdim"], c["udim"], c["n"], [4], likelihood="gaussian", **kw)


# ---------------------------------------------------------------------------------------------------- the yardstick, on the oracle alone
# (case, S, mode) of test_gpu_ensemble.py's parity test
PARITY = [(name, 8, mode) for name in ec.CASES for mode in ("quiet", "noisy")] + \
         [("ragged3", 8, "gaussian"), ("control", 8, "gaussian"), ("wide", 3, "quiet"), ("wide", 3, "noisy")]


@pytest.mark.parametrize("name,S,mode", PARITY)
def test_the_yardstick_of_the_parity_cases(name, S, mode):
    """`fc.bound` asserts max|ref64| < 100 and E <= 1e-4 max|ref64| for each of the four tensors; the scales are the ones the issue
    found (between 0.25 and 37).  It guards the rule's preconditions, not the feature, but shares the feature's case module."""
    import vjf_amd
    assert hasattr(vjf_amd.VJF, "forecast_ensemble")
    m = fc.make_model(vjf_amd, name)
    refs = ec.references(m, name, S, mode)
    for k in ec.TENSORS:
        r64, r32 = refs[k]
        b = fc.bound(r64, r32)
        scale = float(np.abs(r64).max())
        assert 0.1 < scale < 50, (k, scale)
        assert 8 * fc.EPS32 * scale <= b <= 1e-4 * scale
    # the fp32 fold itself: Welford in np.float32 on the fp32 members is the two-pass fp64 result of those members to fp32 rounding
    x32 = refs["x"][1]
    mean, var = ec.welford32(x32)
    np.testing.assert_allclose(mean, x32.astype(np.float64).mean(0), rtol=0, atol=4 * fc.EPS32 * float(np.abs(x32).max()))
    np.testing.assert_allclose(var, x32.astype(np.float64).var(0), rtol=0, atol=16 * fc.EPS32 * max(float(x32.var(0).max()), 1e-30))


# ---------------------------------------------------------------------------------------------------- the host logic
@cpu_only
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "quiet"])
@pytest.mark.parametrize("colmajor", [True, False], ids=["after_rls", "fresh"])
def test_host_draw_order_and_generator_state(fake, colmajor, noise):
    """With a plain x0 and a seed the members are S successive `forecast_sequence` calls under that seed, bit for bit (the stand-in
    computes both alike), and the generator ends in the same state; the moments are those members'."""
    c = SMALL
    m = small_model()
    x0, u = torch.randn(c["B"], c["xdim"]), torch.randn(c["T"], c["B"], c["udim"])
    if colmajor:
        m.filter(torch.randn(c["B"], c["ydim"]), torch.randn(c["B"], c["udim"]), update=True)
        assert m.transition.velocity._w_colmajor
    torch.manual_seed(99)
    seq = [m.forecast_sequence(x0, u, c["T"], noise=noise) for _ in range(c["S"])]
    state = torch.get_rng_state()
    torch.manual_seed(99)
    r = m.forecast_ensemble(x0, u, c["T"], c["S"], noise=noise, return_members=True)
    assert torch.equal(torch.get_rng_state(), state)
    assert r.x.shape == (c["S"], c["T"] + 1, c["B"], c["xdim"]) and r.x.dtype == torch.float32
    for s in range(c["S"]):
        assert same(r.x[s], seq[s][0]), f"member {s}"
    xs, ys = torch.stack([a for a, _ in seq]).double(), torch.stack([b for _, b in seq]).double()
    for got, ref in ((r.x_mean, xs.mean(0)), (r.x_var, xs.var(0, unbiased=False)), (r.y_mean, ys.mean(0)), (r.y_var, ys.var(0, unbiased=False))):
        assert got.shape == ref.shape and got.dtype == torch.float32
        np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=32 * fc.EPS32 * float(ref.abs().max()))
    assert fake.calls[-1] == dict(T=c["T"], S=c["S"], B=c["B"], n=c["n"], d=c["xdim"] + c["udim"], dout=c["xdim"], dy=c["ydim"], x0_ms=0,
                                  u=True, state_noise=noise, members=True)
    # given draws take the place of the generator's: nothing is drawn when all are given, only the missing ones otherwise
    wn, sn = torch.randn(c["S"], c["T"], c["n"], c["xdim"]), torch.randn(c["S"], c["T"], c["B"], c["xdim"])
    before = torch.get_rng_state()
    a = m.forecast_ensemble(x0, u, c["T"], c["S"], w_noise=wn, state_noise=sn, return_members=True)
    assert torch.equal(torch.get_rng_state(), before) and fake.calls[-1]["state_noise"]
    for s in range(c["S"]):
        assert same(a.x[s], m.transition.forecast_sequence(x0, u, c["T"], w_noise=wn[s], state_noise=sn[s]))
    torch.manual_seed(5)
    m.forecast_ensemble(x0, u, c["T"], c["S"], w_noise=wn, noise=True)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    for _ in range(c["S"] * c["T"]):
        torch.randn(c["B"], c["xdim"])
    assert torch.equal(torch.get_rng_state(), after)
    assert a.x is not None and m.forecast_ensemble(x0, u, c["T"], c["S"], w_noise=wn).x is None


@cpu_only
def test_host_gaussian_start_draws_x0_noise_first(fake):
    from vjf_amd import Gaussian
    c = SMALL
    m = small_model()
    mean, u = torch.randn(c["B"], c["xdim"]), torch.randn(c["T"], c["B"], c["udim"])
    q = Gaussian(mean, torch.full_like(mean, ec.LOGVAR0))
    torch.manual_seed(7)
    r = m.forecast_ensemble(q, u, c["T"], c["S"], noise=True, return_members=True)
    state = torch.get_rng_state()
    assert fake.calls[-1]["x0_ms"] == c["B"] * c["xdim"]
    torch.manual_seed(7)
    z = torch.randn(c["S"], c["B"], c["xdim"])                       # first: the starts' noise, one draw
    starts = mean + z * torch.exp(.5 * q.logvar)
    seq = [m.transition.forecast_sequence(starts[s], u, c["T"], noise=True) for s in range(c["S"])]      # then member by member
    assert torch.equal(torch.get_rng_state(), state)
    assert same(r.x[:, 0], starts)
    for s in range(c["S"]):
        assert same(r.x[s], seq[s]), f"member {s}"
    # x0_noise given: not drawn; one start per member given directly is the same call
    before = torch.get_rng_state()
    wn = torch.randn(c["S"], c["T"], c["n"], c["xdim"])
    torch.set_rng_state(before)
    a = m.forecast_ensemble(q, u, c["T"], c["S"], w_noise=wn, x0_noise=z, return_members=True)
    assert torch.equal(torch.get_rng_state(), before)
    b = m.forecast_ensemble(starts, u, c["T"], c["S"], w_noise=wn, return_members=True)
    for k in ("x_mean", "x_var", "y_mean", "y_var", "x"):
        assert same(getattr(a, k), getattr(b, k)), k
    with pytest.raises(AssertionError):
        m.forecast_ensemble(q, u, c["T"], c["S"], w_noise=wn, x0_noise=z[:-1])
    with pytest.raises(AssertionError):
        m.forecast_ensemble(starts[:-1], u, c["T"], c["S"], w_noise=wn)


@cpu_only
def test_host_device_noise_is_one_draw_per_tensor(fake):
    from vjf_amd import Gaussian
    c = SMALL
    import vjf_amd
    torch.manual_seed(1)
    m = vjf_amd.VJF.make_model(5, 3, 0, 9, [4], likelihood="gaussian", noise="device")
    q = Gaussian(torch.zeros(4, 3), torch.zeros(4, 3))
    torch.manual_seed(2)
    r = m.forecast_ensemble(q, None, 6, c["S"], noise=True)
    after = torch.get_rng_state()
    assert r.x_mean.shape == (7, 4, 3) and r.y_var.shape == (7, 4, 5) and r.x is None and fake.calls[-1]["state_noise"]
    torch.manual_seed(2)                                             # (on the CPU "the device's generator" is the CPU one)
    torch.randn(c["S"], 4, 3), torch.randn(c["S"], 6, 9, 3), torch.randn(c["S"], 6, 4, 3)
    assert torch.equal(torch.get_rng_state(), after)


@cpu_only
def test_host_argument_coercion_scratch_and_refusals(fake):
    c = SMALL
    T, S, B, xdim, udim, n, ydim = c["T"], c["S"], c["B"], c["xdim"], c["udim"], c["n"], c["ydim"]
    m = small_model(3)
    x0, u, wn = torch.randn(B, xdim), torch.randn(T, B, udim), torch.randn(S, T, n, xdim)
    # n_step = 0: the start as x_mean[0], its variance across the members, the decoded values; no draw of weights
    before = torch.get_rng_state()
    r = m.forecast_ensemble(x0, u[:0], 0, S, return_members=True)
    assert torch.equal(torch.get_rng_state(), before)
    assert fake.calls[-1]["T"] == 0 and r.x_mean.shape == (1, B, xdim) and r.y_mean.shape == (1, B, ydim) and r.x.shape == (S, 1, B, xdim)
    # (the stand-in's two-pass fp64 variance of S equal values is a rounding residue, not the kernel's exact 0)
    assert torch.equal(r.x_mean[0], x0) and float(r.x_var.abs().max()) < 1e-12 and float(r.y_var.abs().max()) < 1e-12 and same(r.x[1, 0], x0)
    dec = m.decoder.decode
    np.testing.assert_allclose(r.y_mean[0].numpy(), x0.numpy().astype(np.float64) @ dec.weight.detach().numpy().astype(np.float64).T +
                               dec.bias.detach().numpy(), rtol=0, atol=1e-6)
    starts = torch.randn(S, B, xdim)
    r = m.forecast_ensemble(starts, None if udim == 0 else u[:0], 0, S, return_members=True)
    assert same(r.x[:, 0], starts)
    np.testing.assert_allclose(r.x_var[0].numpy(), starts.double().var(0, unbiased=False).numpy(), rtol=0, atol=1e-6)
    # float64 / numpy inputs, RBFDS without a decoder, a 1-D x0 with u lacking its batch axis
    full = m.transition.forecast_ensemble(x0.double().numpy(), u.double(), T, S, w_noise=wn.double().numpy(), return_members=True)
    assert len(full) == 3 and all(t.dtype == torch.float32 for t in full) and fake.calls[-1]["dy"] == 0
    assert full[0].shape == full[1].shape == (T + 1, B, xdim) and full[2].shape == (S, T + 1, B, xdim)
    one = m.transition.forecast_ensemble(x0[4], u[:, 4], T, S, w_noise=wn, state_noise=torch.zeros(S, T, xdim))
    assert one[0].shape == (T + 1, 1, xdim) and one[2] is None and fake.calls[-1]["B"] == 1
    np.testing.assert_allclose(one[0][:, 0].numpy(), full[0][:, 4].numpy(), rtol=0, atol=4 * fc.EPS32 * float(full[0].abs().max()))
    # the scratch tensor is kept and grown on demand
    s = m.transition._fe_scratch
    m.forecast_ensemble(x0, u[:3], 3, S, w_noise=wn[:, :3])
    assert m.transition._fe_scratch is s
    m.forecast_ensemble(x0, u, T, 4 * S, w_noise=torch.randn(4 * S, T, n, xdim))
    assert m.transition._fe_scratch is not s and m.transition._fe_scratch.numel() >= 256 * (T + 1) * 4 * S
    # refusals
    with pytest.raises(ValueError):
        m.forecast_ensemble(x0, u, T, 0)
    with pytest.raises(TypeError):
        m.forecast_ensemble(x0, None, T, S)
    with pytest.raises(AssertionError):
        m.forecast_ensemble(x0, u, T, S, w_noise=wn[:, :, :-1])
    with pytest.raises(AssertionError):
        m.forecast_ensemble(x0, u, T, S, w_noise=wn[:-1])
    with pytest.raises(AssertionError):
        m.forecast_ensemble(x0, u, T, S, w_noise=wn, state_noise=torch.randn(S, T, B + 1, xdim))
    with pytest.raises(AssertionError):
        m.forecast_ensemble(x0, u[:-1], T, S)
    with pytest.raises(AssertionError):
        m.forecast_ensemble(x0[:, :-1], u, T, S)
    # the stand-in's own refusals mirror the library's codes
    p = C.c_void_p(8)
    none = [None] * 16
    assert fake.vjf_forecast_ens(None, 0, *none, 1, 1, 1, 1, 1, 1, 1, None) == -1
    args = [p, 0, None, p, None, p, p, p, p, p, None, None, p, p, None, None, None, p]
    assert fake.vjf_forecast_ens(*args, -1, 1, 1, 1, 1, 1, 0, None) == -20
    assert fake.vjf_forecast_ens(*args, 1, 1, 1, 1, 2, 1, 0, None) == -21


def test_the_library_exports_the_ensemble_and_bounds_its_scratch():
    """Host-only code of the real library: the scratch bound holds whatever T and S are (8 MiB of weight samples + four rows + 32 MiB
    of member states, include/vjf_hip.h), is one member-step where that is less, and the refusal is -20."""
    L = N.lib()
    nbytes = C.c_int64()
    cap = (8 << 20) + (32 << 20) + 4 * 10 * 4 + 512
    assert L.vjf_forecast_ens_scratch_size(10 ** 9, 10 ** 6, 4096, 200, 10, C.byref(nbytes)) == 0 and 0 < nbytes.value <= cap
    assert L.vjf_forecast_ens_scratch_size(1, 1, 1, 20, 3, C.byref(nbytes)) == 0 and 20 * 3 * 4 + 2 * 3 * 4 <= nbytes.value <= 1024
    assert L.vjf_forecast_ens_scratch_size(40, 8, 37, 20, 3, C.byref(nbytes)) == 0
    assert 8 * 40 * 20 * 3 * 4 + 8 * 41 * 37 * 3 * 4 <= nbytes.value <= 8 * 40 * 20 * 3 * 4 + 8 * 41 * 37 * 3 * 4 + 1024
    assert L.vjf_forecast_ens_scratch_size(1, 0, 1, 20, 3, C.byref(nbytes)) == -20
    assert b"vjf_forecast_ens_scratch_size" in L.vjf_last_error()


def test_every_chunking_stays_inside_the_scratch(monkeypatch):
    """Host-only code of the real library, swept over shapes (n_step = 1, the default, included; members, trials and sizes up to where
    each cap binds and beyond) and over the test hooks: the chunk vjf_forecast_ens takes needs no more weight-sample bytes and no more
    state bytes than vjf_forecast_ens_scratch_size provides for its two regions, chunks are never empty, and the bound itself never
    exceeds the documented cap unless one member-step does."""
    L = N.lib()
    W, X = 8 << 20, 32 << 20
    up = lambda v: (v + 255) // 256 * 256                            # noqa: E731
    nbytes, sc, tc = C.c_int64(), C.c_int32(), C.c_int32()
    assert L.vjf_forecast_ens_chunks(0, 1, 1, 1, 1, C.byref(sc), C.byref(tc)) == -20
    count = 0
    for env in ({}, {"VJF_FE_MEMBERS": "7"}, {"VJF_FC_CHUNK": "3"}, {"VJF_FE_MEMBERS": "5", "VJF_FC_CHUNK": "2"}):
        for k in ("VJF_FE_MEMBERS", "VJF_FC_CHUNK"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for T in (1, 2, 3, 15, 16, 17, 200, 5000, 10 ** 9):
            for S in (1, 2, 16, 128, 2000, 4096, 40000, 10 ** 6):
                for B in (1, 3, 4096, 300000):
                    for n, dout in ((20, 3), (200, 10), (1000, 64), (2300, 500)):
                        assert L.vjf_forecast_ens_scratch_size(T, S, B, n, dout, C.byref(nbytes)) == 0
                        assert L.vjf_forecast_ens_chunks(T, S, B, n, dout, C.byref(sc), C.byref(tc)) == 0
                        wstep, xstep = n * dout * 4, B * dout * 4
                        w_region = up(max(min(S * T * wstep, W), wstep) + 16 * dout)       # include/vjf_hip.h: the two regions
                        x_region = up(max(min(S * (T + 1) * xstep, X), 2 * xstep))
                        what = (env, T, S, B, n, dout, sc.value, tc.value)
                        assert nbytes.value == w_region + x_region, what
                        assert 1 <= sc.value <= min(S, 4096) and 1 <= tc.value <= min(T, 4096), what
                        assert sc.value * tc.value * wstep + 16 * dout <= w_region, what
                        assert sc.value * (tc.value + 1) * xstep <= x_region, what
                        assert nbytes.value <= up(max(W, wstep) + 16 * dout) + up(max(X, 2 * xstep)), what
                        count += 1
    assert count == 4 * 9 * 8 * 4 * 4
    # the cases that the bound once missed: one step, many members
    for k in ("VJF_FE_MEMBERS", "VJF_FC_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    assert L.vjf_forecast_ens_chunks(1, 128, 4096, 200, 10, C.byref(sc), C.byref(tc)) == 0
    assert tc.value == 1 and sc.value * 2 * 4096 * 10 * 4 <= X and sc.value >= 64
    assert L.vjf_forecast_ens_chunks(1, 2000, 1, 200, 10, C.byref(sc), C.byref(tc)) == 0
    assert tc.value == 1 and sc.value * 200 * 10 * 4 <= W and sc.value >= 500


@cpu_only
def test_lorenz_example_with_the_ensemble_forecast(fake, capsys):
    """examples/lorenz_fit.py --ensemble 4 end to end on the stand-in: fit, forecast, then the forecast with uncertainty from the last
    posterior (a Gaussian start, one native call) and its printed band."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lorenz_fit_ens", os.path.join(root, "examples", "lorenz_fit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    m, loss = mod.main(["--epochs", "2", "--T", "60", "--n-rbf", "20", "--forecast", "8", "--ensemble", "4"])
    out = capsys.readouterr().out
    assert m.shape == (60, 3) and torch.isfinite(m).all()
    assert fake.calls[-1] == dict(T=8, S=4, B=1, n=20, d=3, dout=3, dy=10, x0_ms=3, u=False, state_noise=True, members=False)
    lines = [ln for ln in out.splitlines() if ln.startswith("ensemble forecast: step")]
    assert len(lines) == 4 and "step    0" in lines[0] and "step    8" in lines[-1]
    for ln in lines:                                                 # mean inside its band, all finite
        x, lo, hi = [float(v) for v in ln.replace("[", " ").replace("]", " ").replace(",", " ").replace("x1 =", " ").split()[4:7]]
        assert np.isfinite([x, lo, hi]).all() and lo <= x <= hi
