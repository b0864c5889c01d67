"""CPU side of the `laplace_filter` tests: the host logic of vjf_amd/model.py (argument order, shapes and dtypes of the result, the
forms of x0, `before` / `head` chaining, one-trial input, the coercion of u and `observed`, the defaults, `gaussian()` and
`log_likelihood()`, every refusal, no write to the model) through a stand-in for vjf_laplace_filter built on tests/laplace_ref.py in
fp64, and the planner and the return codes of the real library (host-only code: no GPU is touched before a refusal)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import fake_backend
from tests import laplace_cases as lc
from tests import laplace_ref as lr
from tests.fake_backend import _arr
from oracle import vjf_oracle as orc
from vjf_amd import _native as N

cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="the stand-in backend works on CPU tensors")


class LaplaceLib(fake_backend.FakeLib):
    """FakeLib + vjf_laplace_filter: laplace_ref.laplace_filter in fp64 on the fp32 values it is handed, stored as fp32, behind the
    entry point's own argument checks.  Records every call's arguments in `calls`."""
    def __init__(self):
        super().__init__()
        self.calls = []

    def vjf_laplace_filter(self, y, u, observed, cen, lw, w_mean, dec_W, dec_b, p_mean, p_lv, p_cov, mean, var, cov, loglik, gnorm,
                           cov_last, T, B, n, d, dout, dy, n_iter, state_var, stream):
        null = lambda p: p is None or not p.value                                                 # noqa: E731
        if any(null(p) for p in (y, cen, lw, w_mean, dec_W, dec_b, p_mean, mean, var, loglik, gnorm, cov_last)):
            self.err = b"vjf_laplace_filter: null tensor"
            return -1
        if (T < 1 or B < 1 or n < 1 or dout < 1 or d < dout or dy < 1 or not 1 <= n_iter <= 64 or not 0 < state_var < np.inf
                or null(p_lv) == null(p_cov)):
            self.err = b"vjf_laplace_filter: bad shape"
            return -20
        du = d - dout
        if du > 0 and null(u):
            self.err = b"vjf_laplace_filter: u is required when d > dout"
            return -21
        if dout > 24:
            self.err = b"vjf_laplace_filter: dout beyond dout <= 24 (VJF_LAP_MAXDOUT)"
            return -11
        f = lambda p, *shape: _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        s = orc.OracleState(1, dout, du, n, (1,), orc.GAUSSIAN)
        s.centroid, s.logwidth, s.w_mean = f(cen, n, d), f(lw, n), f(w_mean, n, dout)
        U = f(u, T, B, du) if du > 0 else None
        obs = None
        if not null(observed):
            obs = np.ctypeslib.as_array((C.c_uint8 * (T * B)).from_address(observed.value)).reshape(T, B).copy()
        Y = f(y, T, B, dy)
        prior = dict(prior_logvar=f(p_lv, B, dout)) if null(p_cov) else dict(prior_cov=f(p_cov, B, dout, dout))
        self.calls.append(dict(T=T, B=B, n=n, d=d, dout=dout, dy=dy, n_iter=n_iter, state_var=state_var, cov=not null(cov), y=Y, u=U,
                               observed=obs, prior_mean=f(p_mean, B, dout), C=f(dec_W, dy, dout), b=f(dec_b, dy), **prior))
        m, v, c, ll, gn = lr.laplace_filter(s, f(dec_W, dy, dout), f(dec_b, dy), Y, U, state_var, f(p_mean, B, dout), observed=obs,
                                            n_iter=n_iter, **prior)
        _arr(mean, T * B * dout).reshape(T, B, dout)[...] = m
        _arr(var, T * B * dout).reshape(T, B, dout)[...] = v
        _arr(loglik, T * B).reshape(T, B)[...] = ll
        _arr(gnorm, T * B).reshape(T, B)[...] = gn
        _arr(cov_last, B * dout * dout).reshape(B, dout, dout)[...] = c[-1]
        if not null(cov):
            _arr(cov, T * B * dout * dout).reshape(T, B, dout, dout)[...] = c
        return 0


@pytest.fixture
def fake():
    old = N._lib
    N._lib = LaplaceLib()
    yield N._lib
    N._lib = old


SMALL = dict(xdim=3, udim=2, n=9, ydim=5, B=4, T=6)


def small_model(udim=SMALL["udim"], seed=17, likelihood="poisson"):
    import vjf_amd
    c = SMALL
    torch.manual_seed(seed)
    m = vjf_amd.VJF.make_model(c["ydim"], c["xdim"], udim, c["n"], [4], likelihood=likelihood)
    g = torch.Generator().manual_seed(seed + 1)
    m.transition.velocity.w_mean.copy_(0.5 * torch.randn(c["n"], c["xdim"], generator=g))
    m.transition.logvar.fill_(math.log(0.02))
    m.decoder.decode.weight.copy_(0.5 * torch.randn(c["ydim"], c["xdim"], generator=g))
    m.decoder.decode.bias.copy_(0.5 + 0.1 * torch.randn(c["ydim"], generator=g))
    return m


def inputs(udim=SMALL["udim"], seed=3, T=SMALL["T"], B=SMALL["B"]):
    g = torch.Generator().manual_seed(seed)
    y = torch.poisson(torch.full((T, B, SMALL["ydim"]), 2.0), generator=g)
    return y, (torch.randn(T, B, udim, generator=g) if udim else None)


def close(a, b, atol=2e-6):
    np.testing.assert_allclose(a.detach().cpu().numpy().astype(np.float64), np.asarray(b, np.float64), rtol=0, atol=atol)


# ---------------------------------------------------------------------------------------------------- the host logic
@cpu_only
def test_shapes_dtypes_defaults_and_argument_order(fake):
    import vjf_amd
    c = SMALL
    m = small_model()
    y, u = inputs()
    out = m.laplace_filter(y, u)
    assert isinstance(out, vjf_amd.model.LaplaceFilterResult)
    assert out._fields == ("mean", "var", "cov", "loglik", "grad_norm", "head")
    T, B, d = c["T"], c["B"], c["xdim"]
    assert out.mean.shape == (T, B, d) and out.var.shape == (T, B, d) and out.cov is None
    assert out.loglik.shape == (T, B) and out.grad_norm.shape == (T, B)
    assert out.head[0].shape == (B, d) and out.head[1].shape == (B, d, d)
    assert all(t.dtype == torch.float32 for t in (out.mean, out.var, out.loglik, out.grad_norm, out.head[0], out.head[1]))
    call, = fake.calls
    assert (call["T"], call["B"], call["n"], call["d"], call["dout"], call["dy"], call["cov"]) == (T, B, c["n"], d + c["udim"], d, c["ydim"], False)
    assert call["observed"] is None and "prior_logvar" in call
    # the defaults: the model's own state variance and `prior`, eight iterations
    assert call["state_var"] == pytest.approx(0.02, rel=1e-6) and call["n_iter"] == 8
    p = m.prior(y[0])
    np.testing.assert_array_equal(call["prior_mean"], p.mean.double().numpy())
    np.testing.assert_array_equal(call["prior_logvar"], p.logvar.double().numpy())
    np.testing.assert_array_equal(call["y"], y.double().numpy())
    np.testing.assert_array_equal(call["u"], u.double().numpy())
    s, Cm, b = lc.state_of(m)
    np.testing.assert_array_equal(call["C"], Cm)
    np.testing.assert_array_equal(call["b"], b)
    ref = lr.laplace_filter(s, Cm, b, y.double().numpy(), u.double().numpy(), call["state_var"], call["prior_mean"],
                            prior_logvar=call["prior_logvar"])
    close(out.mean, ref[0]); close(out.var, ref[1]); close(out.loglik, ref[3], atol=2e-5); close(out.grad_norm, ref[4])
    close(out.head[1], ref[2][-1])
    assert torch.equal(out.head[0], out.mean[-1])
    # the keywords reach the library; float64 and list inputs are coerced; the covariances when asked for
    out = m.laplace_filter(y.double().tolist(), u.double(), state_var=0.5, n_iter=3, return_cov=True)
    call = fake.calls[-1]
    assert call["state_var"] == 0.5 and call["n_iter"] == 3 and call["cov"] is True
    assert out.cov.shape == (T, B, d, d) and out.cov.dtype == torch.float32
    assert torch.equal(out.cov[-1], out.head[1])
    assert torch.equal(torch.diagonal(out.cov, dim1=-2, dim2=-1), out.var)


@cpu_only
def test_the_forms_of_x0_and_before_head_chaining(fake):
    import vjf_amd
    c = SMALL
    m = small_model()
    y, u = inputs()
    g = torch.Generator().manual_seed(9)
    x0 = vjf_amd.Gaussian(torch.randn(c["B"], c["xdim"], generator=g), -2.0 + torch.rand(c["B"], c["xdim"], generator=g))
    whole = m.laplace_filter(y, u, x0=x0, return_cov=True)
    call = fake.calls[-1]
    np.testing.assert_array_equal(call["prior_mean"], x0.mean.double().numpy())
    np.testing.assert_array_equal(call["prior_logvar"], x0.logvar.double().numpy())
    same = m.laplace_filter(y, u, before=(x0.mean, torch.diag_embed(x0.logvar.exp())), return_cov=True)
    assert "prior_cov" in fake.calls[-1] and "prior_logvar" not in fake.calls[-1]
    close(same.mean, whole.mean.numpy(), atol=1e-6)
    close(same.cov, whole.cov.numpy(), atol=1e-6)
    head, parts = None, []
    for lo, hi in ((0, 1), (1, 4), (4, 6)):
        r = m.laplace_filter(y[lo:hi], u[lo:hi], x0=x0 if head is None else None, before=head)
        head = r.head
        parts.append(r)
    close(torch.cat([p.mean for p in parts]), whole.mean.numpy(), atol=1e-6)
    close(torch.cat([p.var for p in parts]), whole.var.numpy(), atol=1e-6)
    close(torch.cat([p.loglik for p in parts]), whole.loglik.numpy(), atol=1e-5)
    close(parts[-1].head[1], whole.cov[-1].numpy(), atol=1e-6)
    with pytest.raises(ValueError, match="not both"):
        m.laplace_filter(y, u, x0=x0, before=whole.head)
    with pytest.raises(AssertionError, match="prior mean"):
        m.laplace_filter(y, u, x0=vjf_amd.Gaussian(x0.mean[:-1], x0.logvar[:-1]))
    with pytest.raises(AssertionError, match="before"):
        m.laplace_filter(y, u, before=(x0.mean, whole.cov[0, :-1]))


@cpu_only
def test_one_trial_and_the_coercion_of_u_and_observed(fake):
    c = SMALL
    m = small_model()
    y, u = inputs()
    obs = torch.ones(c["T"], c["B"], dtype=torch.bool)
    obs[0, 1] = obs[2:4, 2] = obs[-1, 0] = False
    obs[:, 3] = False
    whole = m.laplace_filter(y, u, observed=obs, return_cov=True)
    call = fake.calls[-1]
    assert call["observed"].dtype == np.uint8 and (call["observed"] == obs.numpy()).all()
    assert bool((whole.loglik[~obs] == 0).all()) and bool((whole.loglik[obs] != 0).all()) and bool((whole.grad_norm[~obs] == 0).all())
    for form in (obs.float(), obs.long() * 3, obs.tolist(), obs.numpy()):
        again = m.laplace_filter(y, u, observed=form)
        assert (fake.calls[-1]["observed"] == obs.numpy()).all() and torch.equal(again.mean, whole.mean)
    ynan = y.clone()
    ynan[~obs] = float("nan")
    assert torch.equal(m.laplace_filter(ynan, u, observed=obs).mean, whole.mean)
    one = m.laplace_filter(y[:, 2], u[:, 2], observed=obs[:, 2], return_cov=True)
    assert one.mean.shape == (c["T"], 1, c["xdim"]) and one.cov.shape == (c["T"], 1, c["xdim"], c["xdim"]) and one.loglik.shape == (c["T"], 1)
    assert fake.calls[-1]["B"] == 1
    assert torch.equal(one.mean[:, 0], whole.mean[:, 2])
    m0 = small_model(udim=0)
    assert m0.laplace_filter(y).mean.shape == (c["T"], c["B"], c["xdim"]) and fake.calls[-1]["u"] is None
    with pytest.raises(TypeError):
        m.laplace_filter(y)
    with pytest.raises(AssertionError, match="rows"):
        m.laplace_filter(y, u[:-1])
    with pytest.raises(AssertionError):
        m.laplace_filter(y, u[:, :-1])
    with pytest.raises(AssertionError, match="observed"):
        m.laplace_filter(y, u, observed=obs[:-1])
    with pytest.raises(AssertionError, match="y is"):
        m.laplace_filter(y[:, :, :-1], u)


@cpu_only
def test_gaussian_and_log_likelihood(fake):
    import vjf_amd
    m = small_model(udim=0)
    y, _ = inputs(udim=0)
    out = m.laplace_filter(y, return_cov=True)
    g = out.gaussian()
    assert isinstance(g, vjf_amd.Gaussian) and torch.equal(g.mean, out.mean) and torch.equal(g.logvar, out.var.log())
    ev = out.log_likelihood()
    assert ev.dtype == torch.float64 and ev.shape == (SMALL["B"],)
    np.testing.assert_array_equal(ev.numpy(), out.loglik.numpy().astype(np.float64).sum(axis=0))


@cpu_only
def test_refusals_of_the_python_surface(fake):
    import vjf_amd
    m = small_model()
    y, u = inputs()
    for v in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="state_var"):
            m.laplace_filter(y, u, state_var=v)
    for v in (0, -1, 65, 2.5):
        with pytest.raises(ValueError, match="n_iter"):
            m.laplace_filter(y, u, n_iter=v)
    assert fake.calls == []
    big = vjf_amd.VJF.make_model(5, 25, 0, 9, [4], likelihood="poisson")
    with pytest.raises(NotImplementedError, match="24"):
        big.laplace_filter(torch.zeros(3, 2, 5))
    gaussian = small_model(likelihood="gaussian")
    with pytest.raises(NotImplementedError, match="ekf"):
        gaussian.laplace_filter(y, u)
    with pytest.raises(NotImplementedError, match="Poisson"):
        m.ekf(y, u)
    assert fake.calls == []
    fake.vjf_laplace_filter = lambda *a: (setattr(fake, "err", b"vjf_laplace_filter: n=3000 beyond one workgroup's LDS") or -11)
    with pytest.raises(NotImplementedError, match="LDS"):
        m.laplace_filter(y, u)
    fake.vjf_laplace_filter = lambda *a: (setattr(fake, "err", b"vjf_laplace_filter: refused") or -20)
    with pytest.raises(N.VjfError, match="vjf_laplace_filter: refused"):
        m.laplace_filter(y, u)


@cpu_only
def test_no_write_to_the_model_or_the_generators(fake):
    m = small_model()
    y, u = inputs()
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if isinstance(v, torch.Tensor)}
    counters = m.transition.n_sample
    rng = torch.get_rng_state()
    yc, uc = y.clone(), u.clone()
    m.laplace_filter(y, u, return_cov=True)
    after = m.state_dict()
    assert all(torch.equal(v, after[k]) for k, v in before.items())
    assert m.transition.n_sample == counters and torch.equal(rng, torch.get_rng_state())
    assert torch.equal(y, yc) and torch.equal(u, uc)


# ---------------------------------------------------------------------------------------------------- the real library's host code
def test_return_codes_of_the_entry_point():
    """Every refusal comes before the first launch, so the real entry point can be asked without a GPU: it reads no tensor."""
    L = N.lib()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)

    def call(y=p, u=p, cen=p, W=p, b=p, pm=p, plv=p, pc=None, mean=p, var=p, ll=p, gn=p, last=p, T=4, B=2, n=9, d=5, dout=3, dy=7, it=8,
             sv=0.01):
        return L.vjf_laplace_filter(y, u, None, cen, p, p, W, b, pm, plv, pc, mean, var, None, ll, gn, last, T, B, n, d, dout, dy, it, sv,
                                    None)
    for rc, kw in ((-1, dict(y=None)), (-1, dict(cen=None)), (-1, dict(W=None)), (-1, dict(b=None)), (-1, dict(pm=None)),
                   (-1, dict(mean=None)), (-1, dict(var=None)), (-1, dict(ll=None)), (-1, dict(gn=None)), (-1, dict(last=None)),
                   (-20, dict(T=0)), (-20, dict(B=0)), (-20, dict(n=0)), (-20, dict(d=2)), (-20, dict(dout=0)), (-20, dict(dy=0)),
                   (-20, dict(it=0)), (-20, dict(it=-3)), (-20, dict(it=65)),
                   (-20, dict(sv=0.0)), (-20, dict(sv=-1.0)), (-20, dict(sv=float("nan"))), (-20, dict(sv=float("inf"))),
                   (-20, dict(pc=p)), (-20, dict(plv=None)), (-21, dict(u=None)),
                   (-11, dict(n=9, d=25, dout=25)),                       # dout beyond the kernel's 24
                   (-11, dict(n=1000, d=64, dout=64)),                    # configs[4]'s dimensions
                   (-11, dict(n=3000, d=3, dout=3))):                     # an n that cannot fit
        assert call(**kw) == rc, kw
        assert b"vjf_laplace_filter" in L.vjf_last_error()
    assert not buf.any()


def _largest_n(plan, d, dout, dy):
    """The largest n the planner accepts at (d, dout, dy), by bisection: accepted at n, refused at n + 1."""
    lo, hi = 1, 1 << 16
    assert plan(lo, d, dout, dy) == 0 and plan(hi, d, dout, dy) == -11
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan(mid, d, dout, dy) == 0 else (lo, mid)
    return lo


def test_the_planner_admits_the_guaranteed_shapes():
    """Every xdim <= 16 with n_rbf <= 256 and udim <= 8 is accepted whatever ydim is; the LDS the plan asks for is what the layout in
    DESIGN.md section 3 adds up to, inside a workgroup's 160 KiB; at its edges n is accepted and n + 1 refused, the smallest form of
    n fitting the budget and that of n + 1 not; xdim = 25 and an n that cannot fit are refused with messages naming the limit."""
    L = N.lib()
    lds = C.c_int64()
    plan = lambda n, d, dout, dy: L.vjf_laplace_filter_plan(n, d, dout, dy, C.byref(lds))      # noqa: E731
    floats = lc.lds_floats
    budget = 159 * 1024
    for n, d, dout, dy in ((256, 24, 16, 7), (200, 10, 10, 200), (300, 5, 5, 7), (40, 24, 24, 7), (9, 1, 1, 3), (37, 7, 5, 21), (70, 18, 17, 33),
                           (256, 32, 24, 50)):
        assert plan(n, d, dout, dy) == 0, (n, d, dout, dy)
        assert lds.value <= budget
        assert any(lds.value == 4 * floats(n, d, dout, dy, vg, cl, dl) for vg in range(1, dout + 1) for cl in (False, True)
                   for dl in (False, True)), (n, d, dout, dy)
    for dout in range(1, 17):                     # the guaranteed corner: n = 256, eight control inputs, a small and a huge ydim
        for dy in (1, 50, 1 << 20):
            assert plan(256, dout + 8, dout, dy) == 0 and lds.value <= budget, (dout, dy)
    assert plan(200, 10, 10, 200) == 0 and lds.value == 4 * floats(200, 10, 10, 200, 10, True, True)      # configs[2]'s dimensions
    assert plan(200, 10, 10, 1 << 20) == 0 and lds.value == 4 * floats(200, 10, 10, 1 << 20, 10, True, False)
    for d, dout in ((3, 3), (24, 16), (16, 16), (24, 24), (32, 24), (1, 1)):          # the edges in n
        n = _largest_n(plan, d, dout, 50)
        assert plan(n, d, dout, 50) == 0 and lds.value == 4 * floats(n, d, dout, 50, 1, False, False) <= budget
        assert 4 * floats(n + 1, d, dout, 50, 1, False, False) > budget
        assert plan(n + 1, d, dout, 50) == -11 and b"LDS" in L.vjf_last_error()
        print(f"laplace plan: d = {d} dout = {dout}: n <= {n}")
        assert n >= 256
    assert plan(9, 25, 25, 5) == -11 and b"vjf_laplace_filter_plan" in L.vjf_last_error() and b"24" in L.vjf_last_error()
    assert plan(3000, 3, 3, 5) == -11 and b"vjf_laplace_filter_plan" in L.vjf_last_error() and b"LDS" in L.vjf_last_error()
    assert plan(1000, 64, 64, 5) == -11
    assert plan(9, 2, 3, 5) == -20 and plan(0, 3, 3, 5) == -20 and plan(9, 3, 0, 5) == -20 and plan(9, 3, 3, 0) == -20
    assert L.vjf_laplace_filter_plan(200, 10, 10, 50, None) == 0
