"""CPU side of the `sample_posterior` tests: the host logic of vjf_amd/model.py (argument order, shapes and dtypes of the result, a
Gaussian or a pair as q, one-trial input, both lengths of u, the default state_var and an override, `after` / `head` chaining, the two
noise modes, a given noise used as it is, every assertion and refusal, no write to the model) through a stand-in for vjf_smooth_sample
built on tests/sampler_ref.py in fp64, and the planner and the return codes of the real library (host-only code: no GPU is touched
before a refusal)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fake_backend
from tests import sampler_ref as pr
from tests import tile_layouts
from tests.fake_backend import _arr
from tests.test_smoother_host import SMALL, close, cpu_only, inputs, small_model, state_of
from oracle import vjf_oracle as orc
from vjf_amd import _native as N


class SampleLib(fake_backend.FakeLib):
    """FakeLib + vjf_smooth_sample: sampler_ref.sample in fp64 on the fp32 values it is handed, stored as fp32, behind the entry
    point's own argument checks.  Records every call's arguments in `calls`."""
    def __init__(self):
        super().__init__()
        self.calls = []

    def vjf_smooth_sample(self, mu, lv, u, cen, lw, w_mean, noise, after, x, T, S, B, n, d, dout, state_var, stream):
        null = lambda p: p is None or not p.value                                                 # noqa: E731
        if any(null(p) for p in (mu, lv, cen, lw, w_mean, noise, x)):
            self.err = b"vjf_smooth_sample: null tensor"
            return -1
        if T < 1 or S < 1 or B < 1 or n < 1 or dout < 1 or d < dout or not 0 < state_var < np.inf:
            self.err = b"vjf_smooth_sample: bad shape"
            return -20
        du, aft = d - dout, not null(after)
        if du > 0 and null(u) and (T > 1 or aft):
            self.err = b"vjf_smooth_sample: u is required when d > dout"
            return -21
        if dout >= 32:
            self.err = b"vjf_smooth_sample: dout beyond one workgroup's LDS"
            return -11
        f = lambda p, *shape: _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        s = orc.OracleState(1, dout, du, n, (1,), orc.GAUSSIAN)
        s.centroid, s.logwidth, s.w_mean = f(cen, n, d), f(lw, n), f(w_mean, n, dout)
        U = f(u, T + aft, B, du) if du > 0 and not null(u) else None
        A = f(after, S, B, dout) if aft else None
        self.calls.append(dict(T=T, S=S, B=B, n=n, d=d, dout=dout, state_var=state_var, mu=f(mu, T, B, dout), lv=f(lv, T, B, dout), u=U,
                               after=A, noise=f(noise, S, T, B, dout), noise_ptr=noise.value))
        _arr(x, S * T * B * dout).reshape(S, T, B, dout)[...] = pr.sample(s, f(mu, T, B, dout), f(lv, T, B, dout), U, state_var,
                                                                          f(noise, S, T, B, dout), after=A)
        return 0


@pytest.fixture
def fake():
    old = N._lib
    N._lib = SampleLib()
    yield N._lib
    N._lib = old


def noise_of(S, seed=9, T=SMALL["T"], B=SMALL["B"]):
    return torch.randn(S, T, B, SMALL["xdim"], generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------- the host logic
@cpu_only
def test_shapes_dtypes_defaults_and_argument_order(fake):
    import vjf_amd
    c = SMALL
    m = small_model()
    mu, lv, u = inputs()
    z = noise_of(5)
    out = m.sample_posterior((mu, lv), u, 5, noise=z)
    assert type(out).__name__ == "PosteriorSamples" and out._fields == ("x", "head")
    assert isinstance(out, vjf_amd.model.PosteriorSamples)
    T, B, d = c["T"], c["B"], c["xdim"]
    assert out.x.shape == (5, T, B, d) and out.head.shape == (5, B, d) and out.x.dtype == torch.float32
    assert torch.equal(out.head, out.x[:, 0])
    call, = fake.calls
    assert (call["T"], call["S"], call["B"], call["n"], call["d"], call["dout"]) == (T, 5, B, c["n"], d + c["udim"], d)
    assert call["after"] is None
    assert call["state_var"] == pytest.approx(0.02, rel=1e-6)          # the default state noise is the transition's own, exp(logvar)
    np.testing.assert_array_equal(call["mu"], mu.double().numpy())
    np.testing.assert_array_equal(call["lv"], lv.double().numpy())
    np.testing.assert_array_equal(call["u"], u.double().numpy())
    np.testing.assert_array_equal(call["noise"], z.double().numpy())
    assert call["noise_ptr"] == z.data_ptr(), "a given fp32 noise is handed on as it is, not copied"
    s = state_of(m)
    close(out.x, pr.sample(s, mu.double().numpy(), lv.double().numpy(), u.double().numpy(), call["state_var"], z.double().numpy()))
    # the keywords reach the library; float64 and list inputs are coerced; n_sample defaults to 16
    out = m.sample_posterior((mu.double().tolist(), lv.double()), u.double(), state_var=0.5, noise=noise_of(16).double())
    call = fake.calls[-1]
    assert call["state_var"] == 0.5 and call["S"] == 16 and out.x.shape == (16, T, B, d) and out.x.dtype == torch.float32
    close(out.x, pr.sample(s, mu.double().numpy(), lv.double().numpy(), u.double().numpy(), 0.5, noise_of(16).double().numpy()))
    # the transition's own method is the same call
    out2 = m.transition.sample_posterior((mu, lv), u, 16, state_var=0.5, noise=noise_of(16))
    assert torch.equal(out2.x, out.x)
    # zero noise is the smoothed mean
    from tests import smoother_ref as sr
    zero = m.sample_posterior((mu, lv), u, 2, noise=torch.zeros(2, T, B, d))
    close(zero.x[1], sr.smooth(s, mu.double().numpy(), lv.double().numpy(), u.double().numpy(), fake.calls[-1]["state_var"])[0])


@cpu_only
def test_a_gaussian_or_a_pair_and_one_trial(fake):
    import vjf_amd
    c = SMALL
    m = small_model()
    mu, lv, u = inputs()
    z = noise_of(3)
    a, b = m.sample_posterior(vjf_amd.Gaussian(mu, lv), u, 3, noise=z), m.sample_posterior((mu, lv), u, 3, noise=z)
    assert torch.equal(a.x, b.x)
    # one trial given as (T, xdim), u as (T, udim), noise as (S, T, xdim)
    one = m.sample_posterior((mu[:, 2], lv[:, 2]), u[:, 2], 3, noise=z[:, :, 2])
    assert one.x.shape == (3, c["T"], 1, c["xdim"]) and one.head.shape == (3, 1, c["xdim"]) and fake.calls[-1]["B"] == 1
    assert torch.equal(one.x[:, :, 0], b.x[:, :, 2])
    # T = 1: x = mu + sd z
    last = m.sample_posterior((mu[-1:], lv[-1:]), u[-1:], 3, noise=z[:, -1:])
    close(last.x[:, 0], (mu[-1] + torch.exp(0.5 * lv[-1]) * z[:, -1]).numpy(), atol=1e-6)


@cpu_only
def test_both_lengths_of_u_and_after_head_chaining(fake):
    c = SMALL
    m = small_model()
    mu, lv, u = inputs()
    z = noise_of(4)
    whole = m.sample_posterior((mu, lv), u, 4, noise=z)
    m0 = small_model(udim=0)                     # a model without a control input takes no u
    assert m0.sample_posterior((mu, lv), n_sample=4, noise=z).x.shape == (4,) + mu.shape and fake.calls[-1]["u"] is None
    with pytest.raises(TypeError):
        m.sample_posterior((mu, lv), n_sample=4, noise=z)
    with pytest.raises(AssertionError, match="rows"):
        m.sample_posterior((mu, lv), u[:-1], 4, noise=z)
    with pytest.raises(AssertionError):
        m.sample_posterior((mu, lv), u[:, :-1], 4, noise=z)
    with pytest.raises(AssertionError):
        m.sample_posterior((mu, lv), u[:, :, :-1], 4, noise=z)
    # with `after`, u has T + 1 rows -- and T rows are refused
    k = 2
    back = m.sample_posterior((mu[k:], lv[k:]), u[k:], 4, noise=z[:, k:])
    with pytest.raises(AssertionError, match="rows"):
        m.sample_posterior((mu[:k], lv[:k]), u[:k], 4, noise=z[:, :k], after=back.head)
    front = m.sample_posterior((mu[:k], lv[:k]), u[:k + 1], 4, noise=z[:, :k], after=back.head)
    assert fake.calls[-1]["u"].shape == (k + 1, c["B"], c["udim"]) and fake.calls[-1]["after"].shape == (4, c["B"], c["xdim"])
    close(torch.cat([front.x, back.x], 1), whole.x.numpy(), atol=1e-6)
    # three chunks through the heads; a one-trial `after` without its batch axis
    head, parts = None, []
    for lo, hi in ((4, 6), (1, 4), (0, 1)):
        r = m.sample_posterior((mu[lo:hi], lv[lo:hi]), u[lo:hi + (head is not None)], 4, noise=z[:, lo:hi], after=head)
        head = r.head
        parts.insert(0, r.x)
    close(torch.cat(parts, 1), whole.x.numpy(), atol=1e-6)
    one = m.sample_posterior((mu[:2, 0], lv[:2, 0]), u[:3, 0], 4, noise=z[:, :2, 0], after=whole.x[:, 2, 0])
    close(one.x[:, :, 0], whole.x[:, :2, 0].numpy(), atol=1e-6)


@cpu_only
def test_noise_modes(fake):
    c = SMALL
    T, B, d = c["T"], c["B"], c["xdim"]
    m = small_model()
    mu, lv, u = inputs()
    assert m.noise == "reference"
    # "reference": one randn(S, T, B, xdim) on the CPU generator in the default dtype -- a seed fixes the draws
    torch.manual_seed(123)
    a = m.sample_posterior((mu, lv), u, 3)
    state = torch.get_rng_state()
    torch.manual_seed(123)
    want = torch.randn(3, T, B, d, dtype=torch.get_default_dtype())
    assert torch.equal(state, torch.get_rng_state()), "exactly one randn of the full shape is drawn"
    np.testing.assert_array_equal(fake.calls[-1]["noise"], want.float().double().numpy())
    torch.manual_seed(123)
    assert torch.equal(m.sample_posterior((mu, lv), u, 3).x, a.x)
    assert not torch.equal(m.sample_posterior((mu, lv), u, 3).x, a.x)
    old = torch.get_default_dtype()
    try:
        torch.set_default_dtype(torch.float64)
        torch.manual_seed(123)
        m.sample_posterior((mu, lv), u, 3)
        torch.manual_seed(123)
        np.testing.assert_array_equal(fake.calls[-1]["noise"], torch.randn(3, T, B, d, dtype=torch.float64).float().double().numpy())
    finally:
        torch.set_default_dtype(old)
    # a given noise leaves the generator alone
    rng = torch.get_rng_state()
    m.sample_posterior((mu, lv), u, 3, noise=noise_of(3))
    assert torch.equal(rng, torch.get_rng_state())
    # "device": the storage device's generator, not the CPU one in the reference order (here the storage device is the CPU)
    md = small_model()
    md.noise = "device"
    torch.manual_seed(5)
    md.sample_posterior((mu, lv), u, 3)
    torch.manual_seed(5)
    np.testing.assert_array_equal(fake.calls[-1]["noise"], torch.randn(3, T, B, d, dtype=torch.float32).double().numpy())


@cpu_only
def test_assertions_and_refusals_of_the_python_surface(fake):
    import vjf_amd
    c = SMALL
    T, B, d = c["T"], c["B"], c["xdim"]
    m = small_model()
    mu, lv, u = inputs()
    z = noise_of(4)
    for sv in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="state_var"):
            m.sample_posterior((mu, lv), u, 4, state_var=sv, noise=z)
    for S in (0, -3):
        with pytest.raises(ValueError, match="n_sample"):
            m.sample_posterior((mu, lv), u, S)
    with pytest.raises(AssertionError, match=r"noise is .*expected \(5, 6, 4, 3\)"):
        m.sample_posterior((mu, lv), u, 5, noise=z)
    with pytest.raises(AssertionError, match="noise"):
        m.sample_posterior((mu, lv), u, 4, noise=z[:, :-1])
    with pytest.raises(AssertionError, match=r"after is .*expected \(4, 4, 3\)"):
        m.sample_posterior((mu, lv), torch.cat([u, u[:1]]), 4, noise=z, after=torch.zeros(3, B, d))
    with pytest.raises(AssertionError, match="columns"):
        m.sample_posterior((mu[:, :, :-1], lv[:, :, :-1]), u, 4, noise=z[..., :-1])
    with pytest.raises(AssertionError, match="expected two"):
        m.sample_posterior((mu, lv[:-1]), u, 4, noise=z)
    assert fake.calls == []
    big = vjf_amd.VJF.make_model(5, 33, 0, 9, [4], likelihood="gaussian")
    with pytest.raises(NotImplementedError, match="32"):
        big.sample_posterior((torch.zeros(3, 2, 33), torch.zeros(3, 2, 33)), n_sample=2)
    assert fake.calls == []
    # xdim = 32 passes the kernel's bound and is refused by the plan: -11 of the library is NotImplementedError with its message
    big = vjf_amd.VJF.make_model(5, 32, 0, 9, [4], likelihood="gaussian")
    with pytest.raises(NotImplementedError, match="LDS"):
        big.sample_posterior((torch.zeros(3, 2, 32), torch.zeros(3, 2, 32)), n_sample=2)
    fake.vjf_smooth_sample = lambda *a: (setattr(fake, "err", b"vjf_smooth_sample: refused") or -20)
    with pytest.raises(N.VjfError, match="vjf_smooth_sample: refused"):
        m.sample_posterior((mu, lv), u, 4, noise=z)


@cpu_only
def test_no_write_to_the_model(fake):
    m = small_model()
    mu, lv, u = inputs()
    z = noise_of(4)
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if isinstance(v, torch.Tensor)}
    counters = (m.transition.n_sample, m.likelihood.n_sample)
    rng = torch.get_rng_state()
    muc, lvc, uc, zc = mu.clone(), lv.clone(), u.clone(), z.clone()
    m.sample_posterior((mu, lv), u, 4, noise=z)
    after = m.state_dict()
    assert all(torch.equal(v, after[k]) for k, v in before.items())
    assert (m.transition.n_sample, m.likelihood.n_sample) == counters and torch.equal(rng, torch.get_rng_state())
    assert torch.equal(mu, muc) and torch.equal(lv, lvc) and torch.equal(u, uc) and torch.equal(z, zc)


# ---------------------------------------------------------------------------------------------------- the real library's host code
def test_return_codes_of_the_entry_point():
    """Every refusal comes before the first launch, so the real entry point can be asked without a GPU: it reads no tensor."""
    L = N.lib()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)

    def call(mu=p, lv=p, u=p, cen=p, z=p, after=None, x=p, T=4, S=3, B=2, n=9, d=5, dout=3, sv=0.01):
        return L.vjf_smooth_sample(mu, lv, u, cen, p, p, z, after, x, T, S, B, n, d, dout, sv, None)
    for rc, kw in ((-1, dict(mu=None)), (-1, dict(lv=None)), (-1, dict(cen=None)), (-1, dict(z=None)), (-1, dict(x=None)),
                   (-20, dict(T=0)), (-20, dict(S=0)), (-20, dict(B=0)), (-20, dict(n=0)), (-20, dict(d=2)), (-20, dict(dout=0)),
                   (-20, dict(sv=0.0)), (-20, dict(sv=-1.0)), (-20, dict(sv=float("nan"))), (-20, dict(sv=float("inf"))),
                   (-21, dict(u=None)), (-21, dict(u=None, T=1, after=p)),
                   (-11, dict(n=9, d=33, dout=33)),                       # dout beyond the kernel's 32
                   (-11, dict(n=9, d=32, dout=32)),                       # dout = 32: beyond the plan whatever n is
                   (-11, dict(n=1000, d=64, dout=64)),                    # configs[4]'s dimensions
                   (-11, dict(n=3000, d=3, dout=3))):                     # an n that cannot fit
        assert call(**kw) == rc, kw
        assert b"vjf_smooth_sample" in L.vjf_last_error()


def plan(n, d, dout, S):
    sc, lds = C.c_int32(-1), C.c_int64(-1)
    return N.lib().vjf_smooth_sample_plan(n, d, dout, S, C.byref(sc), C.byref(lds)), sc.value, lds.value


floats = tile_layouts.sample          # the layout of DESIGN.md section 3 "Posterior draws" added up


def test_the_planner_admits_every_shape_the_smoother_does(monkeypatch):
    monkeypatch.delenv("VJF_SMS_MEMBERS", raising=False)
    L = N.lib()
    for S in (1, 16, 64, 1000):
        for n, d, dout in ((256, 32, 24), (200, 10, 10), (300, 5, 5), (40, 24, 24), (9, 1, 1), (37, 7, 5), (70, 18, 17), (200, 28, 28),
                           (753, 24, 24), (360, 28, 28), (141, 30, 30), (20, 3, 3)):
            assert L.vjf_smooth_plan(n, d, dout, None) == 0
            rc, sc, lds = plan(n, d, dout, S)
            assert rc == 0 and 1 <= sc <= S and lds <= 159 * 1024, (n, d, dout, S, rc, sc, lds)
            assert any(lds == 4 * floats(n, d, dout, vg, sc, cl) for vg in range(1, dout + 1) for cl in (False, True)), (n, d, dout, S)
            # the largest chunk that fits: one member more is beyond the budget beside the smallest pass, or S is reached
            assert sc == S or 4 * floats(n, d, dout, min(dout, 4), sc + 1, False) > 159 * 1024, (n, d, dout, S, sc)
    for dout in range(1, 25):                     # the guaranteed corner: n = 256, eight control inputs
        rc, sc, lds = plan(256, dout + 8, dout, 16)
        assert rc == 0 and sc >= 1 and lds <= 159 * 1024, dout
    # a Lorenz-sized model carries 64 members in one workgroup; the corner carries several
    assert plan(20, 3, 3, 64)[:2] == (0, 64)
    assert plan(256, 32, 24, 16)[1] >= 4
    # refused where the smoother is refused, with messages naming the limit
    for n, d, dout in ((9, 33, 33), (9, 32, 32), (200, 32, 32), (3000, 3, 3), (1000, 64, 64), (754, 24, 24)):
        assert L.vjf_smooth_plan(n, d, dout, None) == -11
        assert plan(n, d, dout, 8)[0] == -11 and b"vjf_smooth_sample_plan" in L.vjf_last_error(), (n, d, dout)
    assert plan(9, 33, 33, 8)[0] == -11 and b"32" in L.vjf_last_error()
    assert plan(3000, 3, 3, 8)[0] == -11 and b"LDS" in L.vjf_last_error()
    assert plan(9, 2, 3, 4)[0] == -20 and plan(0, 3, 3, 4)[0] == -20 and plan(9, 3, 0, 4)[0] == -20 and plan(9, 3, 3, 0)[0] == -20
    assert L.vjf_smooth_sample_plan(200, 10, 10, 16, None, None) == 0


def test_the_override_of_the_members_per_workgroup(monkeypatch):
    free = plan(200, 10, 10, 64)[1]
    for forced in (1, 3, 16):
        monkeypatch.setenv("VJF_SMS_MEMBERS", str(forced))
        rc, sc, lds = plan(200, 10, 10, 64)
        assert (rc, sc) == (0, min(forced, free)) and any(lds == 4 * floats(200, 10, 10, vg, sc, cl) for vg in range(1, 11) for cl in (False, True))
        assert plan(200, 10, 10, 2)[1] == min(forced, 2), "never above S"
    monkeypatch.setenv("VJF_SMS_MEMBERS", "100000")
    assert plan(200, 10, 10, 64)[1] == free, "never above what fits"
    monkeypatch.setenv("VJF_SMS_MEMBERS", "0")
    assert plan(200, 10, 10, 64)[1] == free
