"""CPU side of the `smooth` tests: the host logic of vjf_amd/model.py (argument order, shapes and dtypes of the result, a Gaussian or a
pair as q, one-trial input, the coercion of u and both of its lengths, the default state_var and an override, `after` / `head` chaining,
`gaussian()`, every refusal, no write to the model) through a stand-in for vjf_smooth built on tests/smoother_ref.py in fp64, and the
planner and the return codes of the real library (host-only code: no GPU is touched before a refusal)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import fake_backend
from tests import smoother_ref as sr
from tests import tile_layouts
from tests.fake_backend import _arr
from oracle import vjf_oracle as orc
from vjf_amd import _native as N

cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="the stand-in backend works on CPU tensors")


class SmoothLib(fake_backend.FakeLib):
    """FakeLib + vjf_smooth: smoother_ref.smooth in fp64 on the fp32 values it is handed, stored as fp32, behind the entry point's own
    argument checks.  Records every call's arguments in `calls`."""
    def __init__(self):
        super().__init__()
        self.calls = []

    def vjf_smooth(self, mu, lv, u, cen, lw, w_mean, a_mean, a_cov, mean, var, cov, cov0, T, B, n, d, dout, state_var, stream):
        null = lambda p: p is None or not p.value                                                 # noqa: E731
        if any(null(p) for p in (mu, lv, cen, lw, w_mean, mean, var, cov0)):
            self.err = b"vjf_smooth: null tensor"
            return -1
        if T < 1 or B < 1 or n < 1 or dout < 1 or d < dout or not 0 < state_var < np.inf or null(a_mean) != null(a_cov):
            self.err = b"vjf_smooth: bad shape"
            return -20
        du, after = d - dout, not null(a_mean)
        if du > 0 and null(u) and (T > 1 or after):
            self.err = b"vjf_smooth: u is required when d > dout"
            return -21
        if dout > 32:
            self.err = b"vjf_smooth: dout beyond dout <= 32 (VJF_SM_MAXDOUT)"
            return -11
        f = lambda p, *shape: _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        s = orc.OracleState(1, dout, du, n, (1,), orc.GAUSSIAN)
        s.centroid, s.logwidth, s.w_mean = f(cen, n, d), f(lw, n), f(w_mean, n, dout)
        U = f(u, T + after, B, du) if du > 0 and not null(u) else None
        aft = (f(a_mean, B, dout), f(a_cov, B, dout, dout)) if after else None
        self.calls.append(dict(T=T, B=B, n=n, d=d, dout=dout, state_var=state_var, cov=not null(cov), mu=f(mu, T, B, dout),
                               lv=f(lv, T, B, dout), u=U, after=aft))
        m, v, c = sr.smooth(s, f(mu, T, B, dout), f(lv, T, B, dout), U, state_var, after=aft)
        _arr(mean, T * B * dout).reshape(T, B, dout)[...] = m
        _arr(var, T * B * dout).reshape(T, B, dout)[...] = v
        _arr(cov0, B * dout * dout).reshape(B, dout, dout)[...] = c[0]
        if not null(cov):
            _arr(cov, T * B * dout * dout).reshape(T, B, dout, dout)[...] = c
        return 0


@pytest.fixture
def fake():
    old = N._lib
    N._lib = SmoothLib()
    yield N._lib
    N._lib = old


SMALL = dict(xdim=3, udim=2, n=9, ydim=5, B=4, T=6)


def small_model(udim=SMALL["udim"], seed=17):
    import vjf_amd
    c = SMALL
    torch.manual_seed(seed)
    m = vjf_amd.VJF.make_model(c["ydim"], c["xdim"], udim, c["n"], [4], likelihood="gaussian")
    g = torch.Generator().manual_seed(seed + 1)
    m.transition.velocity.w_mean.copy_(0.5 * torch.randn(c["n"], c["xdim"], generator=g))
    m.transition.logvar.fill_(math.log(0.02))
    return m


def state_of(m):
    vel = m.transition.velocity
    n, d = vel.feature.centroid.shape
    s = orc.OracleState(1, vel.n_output, d - vel.n_output, n, (1,), orc.GAUSSIAN)
    g = lambda t: t.detach().cpu().numpy().astype(np.float64)      # noqa: E731
    s.centroid, s.logwidth, s.w_mean = g(vel.feature.centroid), g(vel.feature.logwidth), g(vel.w_mean).reshape(n, vel.n_output)
    return s


def inputs(udim=SMALL["udim"], seed=3, T=SMALL["T"], B=SMALL["B"]):
    g = torch.Generator().manual_seed(seed)
    mu = 0.5 * torch.randn(T, B, SMALL["xdim"], generator=g)
    lv = -3.0 + torch.rand(T, B, SMALL["xdim"], generator=g)
    return mu, lv, (torch.randn(T, B, udim, generator=g) if udim else None)


def close(a, b, atol=2e-6):
    np.testing.assert_allclose(a.detach().cpu().numpy().astype(np.float64), np.asarray(b, np.float64), rtol=0, atol=atol)


# ---------------------------------------------------------------------------------------------------- the host logic
@cpu_only
def test_shapes_dtypes_defaults_and_argument_order(fake):
    import vjf_amd
    c = SMALL
    m = small_model()
    mu, lv, u = inputs()
    out = m.smooth((mu, lv), u)
    assert type(out).__name__ == "SmoothResult" and out._fields == ("mean", "var", "cov", "head")
    assert isinstance(out, vjf_amd.model.SmoothResult)
    T, B, d = c["T"], c["B"], c["xdim"]
    assert out.mean.shape == (T, B, d) and out.var.shape == (T, B, d) and out.cov is None
    assert out.head[0].shape == (B, d) and out.head[1].shape == (B, d, d)
    assert all(t.dtype == torch.float32 for t in (out.mean, out.var, out.head[0], out.head[1]))
    call, = fake.calls
    assert (call["T"], call["B"], call["n"], call["d"], call["dout"], call["cov"]) == (T, B, c["n"], d + c["udim"], d, False)
    assert call["after"] is None
    # the default state noise is the transition's own, exp(logvar)
    assert call["state_var"] == pytest.approx(0.02, rel=1e-6)
    np.testing.assert_array_equal(call["mu"], mu.double().numpy())
    np.testing.assert_array_equal(call["lv"], lv.double().numpy())
    np.testing.assert_array_equal(call["u"], u.double().numpy())
    s = state_of(m)
    mean, var, cov = sr.smooth(s, mu.double().numpy(), lv.double().numpy(), u.double().numpy(), call["state_var"])
    close(out.mean, mean); close(out.var, var); close(out.head[1], cov[0])
    assert torch.equal(out.head[0], out.mean[0])
    # the keywords reach the library; float64 and list inputs are coerced; the covariances when asked for
    out = m.smooth((mu.double().tolist(), lv.double()), u.double(), state_var=0.5, return_cov=True)
    call = fake.calls[-1]
    assert call["state_var"] == 0.5 and call["cov"] is True
    assert out.cov.shape == (T, B, d, d) and out.cov.dtype == torch.float32
    close(out.cov, sr.smooth(s, mu.double().numpy(), lv.double().numpy(), u.double().numpy(), 0.5)[2])
    assert torch.equal(out.cov[0], out.head[1])
    # the transition's own method is the same call
    out2 = m.transition.smooth((mu, lv), u, state_var=0.5, return_cov=True)
    assert torch.equal(out2.mean, out.mean) and torch.equal(out2.cov, out.cov)


@cpu_only
def test_a_gaussian_or_a_pair_and_one_trial(fake):
    import vjf_amd
    c = SMALL
    m = small_model()
    mu, lv, u = inputs()
    a, b = m.smooth(vjf_amd.Gaussian(mu, lv), u), m.smooth((mu, lv), u)
    assert torch.equal(a.mean, b.mean) and torch.equal(a.var, b.var)
    # one trial given as (T, xdim), u as (T, udim)
    one = m.smooth((mu[:, 2], lv[:, 2]), u[:, 2], return_cov=True)
    assert one.mean.shape == (c["T"], 1, c["xdim"]) and one.cov.shape == (c["T"], 1, c["xdim"], c["xdim"])
    assert fake.calls[-1]["B"] == 1
    assert torch.equal(one.mean[:, 0], b.mean[:, 2])
    # T = 1
    last = m.smooth((mu[-1:], lv[-1:]), u[-1:])
    assert torch.equal(last.mean, mu[-1:]) and last.var.shape == (1, c["B"], c["xdim"])


@cpu_only
def test_coercion_of_u_and_both_lengths(fake):
    c = SMALL
    m = small_model()
    mu, lv, u = inputs()
    whole = m.smooth((mu, lv), u, return_cov=True)
    # a model without a control input takes no u
    m0 = small_model(udim=0)
    assert m0.smooth((mu, lv)).mean.shape == mu.shape and fake.calls[-1]["u"] is None
    with pytest.raises(TypeError):
        m.smooth((mu, lv))
    with pytest.raises(AssertionError, match="rows"):
        m.smooth((mu, lv), u[:-1])
    with pytest.raises(AssertionError):
        m.smooth((mu, lv), u[:, :-1])
    with pytest.raises(AssertionError):
        m.smooth((mu, lv), u[:, :, :-1])
    with pytest.raises(AssertionError, match="columns"):
        m.smooth((mu[:, :, :-1], lv[:, :, :-1]), u)
    with pytest.raises(AssertionError):
        m.smooth((mu, lv[:-1]), u)
    # with `after`, u has T + 1 rows -- and T rows are refused
    k = 2
    back = m.smooth((mu[k:], lv[k:]), u[k:])
    with pytest.raises(AssertionError, match="rows"):
        m.smooth((mu[:k], lv[:k]), u[:k], after=back.head)
    front = m.smooth((mu[:k], lv[:k]), u[:k + 1], after=back.head, return_cov=True)
    assert fake.calls[-1]["u"].shape == (k + 1, c["B"], c["udim"]) and fake.calls[-1]["after"] is not None
    close(torch.cat([front.mean, back.mean]), whole.mean.numpy(), atol=1e-6)
    close(front.cov, whole.cov[:k].numpy(), atol=1e-6)


@cpu_only
def test_after_head_chaining_and_gaussian(fake):
    import vjf_amd
    m = small_model(udim=0)
    mu, lv, _ = inputs(udim=0)
    whole = m.smooth((mu, lv), return_cov=True)
    heads, parts = None, []
    for lo, hi in ((4, 6), (1, 4), (0, 1)):
        r = m.smooth((mu[lo:hi], lv[lo:hi]), after=heads)
        heads = r.head
        parts.insert(0, r)
    close(torch.cat([p.mean for p in parts]), whole.mean.numpy(), atol=1e-6)
    close(torch.cat([p.var for p in parts]), whole.var.numpy(), atol=1e-6)
    close(parts[0].head[1], whole.cov[0].numpy(), atol=1e-6)
    # a one-trial `after` given without its batch axis
    one = m.smooth((mu[:2, 0], lv[:2, 0]), after=(whole.mean[2, 0], whole.cov[2, 0]))
    close(one.mean[:, 0], whole.mean[:2, 0].numpy(), atol=1e-6)
    with pytest.raises(AssertionError, match="after"):
        m.smooth((mu[:2], lv[:2]), after=(whole.mean[2, :-1], whole.cov[2, :-1]))
    g = whole.gaussian()
    assert isinstance(g, vjf_amd.Gaussian) and torch.equal(g.mean, whole.mean) and torch.equal(g.logvar, whole.var.log())


@cpu_only
def test_refusals_of_the_python_surface(fake):
    import vjf_amd
    m = small_model()
    mu, lv, u = inputs()
    for sv in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="state_var"):
            m.smooth((mu, lv), u, state_var=sv)
    assert fake.calls == []
    big = vjf_amd.VJF.make_model(5, 33, 0, 9, [4], likelihood="gaussian")
    with pytest.raises(NotImplementedError, match="32"):
        big.smooth((torch.zeros(3, 2, 33), torch.zeros(3, 2, 33)))
    assert fake.calls == []
    # -11 of the library (a shape beyond the plan) is NotImplementedError with the library's message; other codes are VjfError
    fake.vjf_smooth = lambda *a: (setattr(fake, "err", b"vjf_smooth: n=3000 beyond one workgroup's LDS") or -11)
    with pytest.raises(NotImplementedError, match="LDS"):
        m.smooth((mu, lv), u)
    fake.vjf_smooth = lambda *a: (setattr(fake, "err", b"vjf_smooth: refused") or -20)
    with pytest.raises(N.VjfError, match="vjf_smooth: refused"):
        m.smooth((mu, lv), u)


@cpu_only
def test_no_write_to_the_model_or_the_generators(fake):
    m = small_model()
    mu, lv, u = inputs()
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if isinstance(v, torch.Tensor)}
    counters = (m.transition.n_sample, m.likelihood.n_sample)
    rng = torch.get_rng_state()
    muc, lvc, uc = mu.clone(), lv.clone(), u.clone()
    m.smooth((mu, lv), u, return_cov=True)
    after = m.state_dict()
    assert all(torch.equal(v, after[k]) for k, v in before.items())
    assert (m.transition.n_sample, m.likelihood.n_sample) == counters and torch.equal(rng, torch.get_rng_state())
    assert torch.equal(mu, muc) and torch.equal(lv, lvc) and torch.equal(u, uc)


# ---------------------------------------------------------------------------------------------------- the real library's host code
def test_return_codes_of_the_entry_point():
    """Every refusal comes before the first launch, so the real entry point can be asked without a GPU: it reads no tensor."""
    L = N.lib()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)

    def call(mu=p, lv=p, u=p, cen=p, am=None, ac=None, mean=p, var=p, cov0=p, T=4, B=2, n=9, d=5, dout=3, sv=0.01):
        return L.vjf_smooth(mu, lv, u, cen, p, p, am, ac, mean, var, None, cov0, T, B, n, d, dout, sv, None)
    for rc, kw in ((-1, dict(mu=None)), (-1, dict(lv=None)), (-1, dict(cen=None)), (-1, dict(mean=None)), (-1, dict(var=None)),
                   (-1, dict(cov0=None)), (-20, dict(T=0)), (-20, dict(B=0)), (-20, dict(n=0)), (-20, dict(d=2)), (-20, dict(dout=0)),
                   (-20, dict(sv=0.0)), (-20, dict(sv=-1.0)), (-20, dict(sv=float("nan"))), (-20, dict(sv=float("inf"))),
                   (-20, dict(am=p)), (-20, dict(ac=p)), (-21, dict(u=None)), (-21, dict(u=None, T=1, am=p, ac=p)),
                   (-11, dict(n=9, d=33, dout=33)),                       # dout beyond the kernel's 32
                   (-11, dict(n=1000, d=64, dout=64)),                    # configs[4]'s dimensions
                   (-11, dict(n=3000, d=3, dout=3))):                     # an n that cannot fit
        assert call(**kw) == rc, kw
        assert b"vjf_smooth" in L.vjf_last_error()


def test_the_planner_admits_the_guaranteed_shapes():
    """Every dout <= 24 with n <= 256 and d - dout <= 8 is accepted and the LDS the plan asks for is what the layout in DESIGN.md
    section 3 adds up to, inside a workgroup's 160 KiB; dout = 33 and an n that cannot fit are refused with messages naming the limit."""
    L = N.lib()
    lds = C.c_int64()
    plan = lambda n, d, dout: L.vjf_smooth_plan(n, d, dout, C.byref(lds))      # noqa: E731

    floats = tile_layouts.smooth
    for n, d, dout in ((256, 32, 24), (200, 10, 10), (300, 5, 5), (40, 24, 24), (9, 1, 1), (37, 7, 5), (70, 18, 17)):
        assert plan(n, d, dout) == 0, (n, d, dout)
        assert lds.value <= 159 * 1024
        assert any(lds.value == 4 * floats(n, d, dout, vg, cl) for vg in range(1, dout + 1) for cl in (False, True)), (n, d, dout)
    for dout in range(1, 25):                     # the guaranteed corner: n = 256, eight control inputs
        assert plan(256, dout + 8, dout) == 0 and lds.value <= 159 * 1024, dout
    # (the corner: the shared operands stay in global memory, and the columns of A take several passes)
    assert plan(256, 32, 24) == 0 and any(lds.value == 4 * floats(256, 32, 24, vg, False) for vg in range(1, 24))
    assert plan(200, 10, 10) == 0 and lds.value == 4 * floats(200, 10, 10, 10, True)
    assert plan(200, 28, 28) == 0 and lds.value <= 159 * 1024
    assert plan(9, 33, 33) == -11 and b"vjf_smooth_plan" in L.vjf_last_error() and b"32" in L.vjf_last_error()
    assert plan(3000, 3, 3) == -11 and b"vjf_smooth_plan" in L.vjf_last_error() and b"LDS" in L.vjf_last_error()
    assert plan(200, 32, 32) == -11 and b"LDS" in L.vjf_last_error()
    assert plan(1000, 64, 64) == -11
    assert plan(9, 2, 3) == -20 and plan(0, 3, 3) == -20 and plan(9, 3, 0) == -20
    assert L.vjf_smooth_plan(200, 10, 10, None) == 0
