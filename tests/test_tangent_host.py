"""CPU side of the `lyapunov` / `jacobian` tests: the host logic of vjf_amd/model.py (shapes, dtypes and defaults, a Gaussian start, the
burn-in split, `dt`, continuation, n_step = 0, argument coercion and refusals) through a stand-in for vjf_tangent_rollout built on
tests/tangent_ref.py in fp64, and the planner and the return codes of the real library (host-only code: no GPU is touched before a
refusal)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fake_backend
from tests import tangent_ref as tr
from tests.fake_backend import _arr
from oracle import vjf_oracle as orc
from vjf_amd import _native as N

cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="the stand-in backend works on CPU tensors")


class TangentLib(fake_backend.FakeLib):
    """FakeLib + vjf_tangent_rollout: tangent_ref.rollout in fp64 on the fp32 values it is handed, stored as fp32, behind the entry
    point's own argument checks.  Records every call's arguments in `calls`."""
    def __init__(self):
        super().__init__()
        self.calls = []

    def vjf_tangent_rollout(self, x0, u, q0, cen, lw, w_mean, x_out, q_out, lsum, lhist, T, B, n, d, dout, m, qr, accumulate, stream):
        null = lambda p: p is None or not p.value                                                 # noqa: E731
        if any(null(p) for p in (x0, cen, lw, w_mean, x_out, q_out)) or (qr > 0 and null(lsum)):
            self.err = b"vjf_tangent_rollout: null tensor"
            return -1
        if T < 0 or B < 1 or n < 1 or dout < 1 or d < dout or m < 1 or m > dout or qr < 0 or (qr == 0 and not null(lhist)):
            self.err = b"vjf_tangent_rollout: bad shape"
            return -20
        du = d - dout
        if du > 0 and null(u) and T > 0:
            self.err = b"vjf_tangent_rollout: u is required when d > dout"
            return -21
        f = lambda p, *shape: _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        s = orc.OracleState(1, dout, du, n, (1,), orc.GAUSSIAN)
        s.centroid, s.logwidth, s.w_mean = f(cen, n, d), f(lw, n), f(w_mean, n, dout)
        U = None if null(u) or T == 0 else f(u, T, B, du)
        self.calls.append(dict(T=T, B=B, n=n, d=d, dout=dout, m=m, qr=qr, accumulate=accumulate, q0=not null(q0), history=not null(lhist),
                               x0=f(x0, B, dout), u=U))
        x, Q, hist, ls = tr.rollout(s, f(x0, B, dout), U, None if null(q0) else f(q0, B, dout, m), T, m, qr,
                                    f(lsum, B, m) if accumulate and not null(lsum) else None)
        _arr(x_out, B * dout).reshape(B, dout)[...] = x
        _arr(q_out, B * dout * m).reshape(B, dout, m)[...] = Q
        if not null(lsum):
            _arr(lsum, B * m).reshape(B, m)[...] = ls
        if not null(lhist):
            _arr(lhist, hist.size).reshape(hist.shape)[...] = hist
        return 0


@pytest.fixture
def fake():
    old = N._lib
    N._lib = TangentLib()
    yield N._lib
    N._lib = old


SMALL = dict(xdim=3, udim=2, n=9, ydim=5, B=6, T=7)


def small_model(udim=SMALL["udim"], seed=17):
    import vjf_amd
    c = SMALL
    torch.manual_seed(seed)
    m = vjf_amd.VJF.make_model(c["ydim"], c["xdim"], udim, c["n"], [4], likelihood="gaussian")
    g = torch.Generator().manual_seed(seed + 1)
    m.transition.velocity.w_mean.copy_(0.5 * torch.randn(c["n"], c["xdim"], generator=g))
    return m


def state_of(m):
    vel = m.transition.velocity
    n, d = vel.feature.centroid.shape
    s = orc.OracleState(1, vel.n_output, d - vel.n_output, n, (1,), orc.GAUSSIAN)
    g = lambda t: t.detach().cpu().numpy().astype(np.float64)      # noqa: E731
    s.centroid, s.logwidth, s.w_mean = g(vel.feature.centroid), g(vel.feature.logwidth), g(vel.w_mean).reshape(n, vel.n_output)
    return s


def inputs(T, udim=SMALL["udim"], seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(SMALL["B"], SMALL["xdim"], generator=g), (torch.randn(T, SMALL["B"], udim, generator=g) if udim else None)


def close(a, b, atol=2e-6):
    np.testing.assert_allclose(a.detach().cpu().numpy().astype(np.float64), np.asarray(b, np.float64), rtol=0, atol=atol)


# ---------------------------------------------------------------------------------------------------- the host logic
@cpu_only
def test_shapes_dtypes_and_defaults(fake):
    c = SMALL
    m = small_model()
    x0, u = inputs(c["T"])
    out = m.lyapunov(x0, u, c["T"])
    assert type(out).__name__ == "LyapunovResult" and out._fields == ("exponents", "x", "q", "log_stretch")
    assert out.exponents.shape == (c["B"], c["xdim"]) and out.x.shape == (c["B"], c["xdim"]) and out.q.shape == (c["B"], c["xdim"], c["xdim"])
    assert out.log_stretch is None and all(t.dtype == torch.float32 for t in out[:3])
    call, = fake.calls
    assert (call["T"], call["m"], call["qr"], call["accumulate"], call["q0"], call["history"]) == (c["T"], c["xdim"], 1, 0, False, False)
    x, Q, hist, ls = tr.rollout(state_of(m), x0.double().numpy(), u.double().numpy(), None, c["T"], c["xdim"], 1)
    close(out.exponents, ls / c["T"]); close(out.x, x); close(out.q, Q)
    # n_exponent, qr_every, the history: ceil(7 / 3) = 3 rows; float64 and list inputs are coerced
    out = m.lyapunov(x0.double().tolist(), u.double(), c["T"], n_exponent=2, qr_every=3, return_history=True)
    assert out.exponents.shape == (c["B"], 2) and out.q.shape == (c["B"], c["xdim"], 2) and out.log_stretch.shape == (3, c["B"], 2)
    assert out.log_stretch.dtype == torch.float32
    x, Q, hist, ls = tr.rollout(state_of(m), x0.double().numpy(), u.double().numpy(), None, c["T"], 2, 3)
    close(out.log_stretch, hist); close(out.exponents, ls / c["T"])
    close(out.log_stretch.sum(0), ls)
    # the transition's own method is the same call
    out2 = m.transition.lyapunov(x0, u, c["T"], n_exponent=2, qr_every=3)
    assert torch.equal(out2.exponents, out.exponents)


@cpu_only
def test_jacobian(fake):
    c = SMALL
    m = small_model()
    x0, u = inputs(1)
    J = m.jacobian(x0, u[0])
    assert J.shape == (c["B"], c["xdim"], c["xdim"]) and J.dtype == torch.float32
    call = fake.calls[-1]
    assert (call["T"], call["m"], call["qr"], call["q0"], call["history"]) == (1, c["xdim"], 0, False, False)
    close(J, tr.jacobian(state_of(m), x0.double().numpy(), u[0].double().numpy()))
    # J[b, i, j] = d f_i / d x_j: autograd on torch's own forward of the mean map
    s = state_of(m)
    for b in range(2):
        xb = x0[b].double().clone().requires_grad_(True)

        def fmap(x):
            xu = torch.cat([x, u[0, b].double()])
            d2 = ((xu[None, :] - torch.tensor(s.centroid)) ** 2).sum(1)
            return x + torch.exp(-0.5 * d2 / torch.exp(torch.tensor(s.logwidth)) ** 2) @ torch.tensor(s.w_mean)
        close(J[b], torch.autograd.functional.jacobian(fmap, xb).numpy())
    # one trial given 1-D, and a model without a control input
    J1 = m.jacobian(x0[2], u[0, 2])
    assert J1.shape == (1, c["xdim"], c["xdim"]) and torch.equal(J1[0], J[2])
    m0 = small_model(udim=0)
    assert m0.jacobian(x0).shape == (c["B"], c["xdim"], c["xdim"])
    with pytest.raises(TypeError):
        m.jacobian(x0)
    with pytest.raises(AssertionError):
        m.jacobian(x0[:, :-1], u[0])


@cpu_only
def test_a_gaussian_start_stands_for_its_mean(fake):
    import vjf_amd
    m = small_model()
    x0, u = inputs(SMALL["T"])
    q = vjf_amd.Gaussian(x0, torch.full_like(x0, -2.0))
    a, b = m.lyapunov(q, u, SMALL["T"]), m.lyapunov(x0, u, SMALL["T"])
    assert torch.equal(a.exponents, b.exponents) and torch.equal(a.q, b.q)
    assert torch.equal(m.jacobian(q, u[0]), m.jacobian(x0, u[0]))


@cpu_only
def test_burn_in_is_a_first_call_whose_sums_are_discarded(fake):
    c = SMALL
    m = small_model()
    T0, T = 4, c["T"]
    x0, u = inputs(T0 + T)
    out = m.lyapunov(x0, u, T, burn_in=T0, n_exponent=2, qr_every=2, return_history=True)
    first, second = fake.calls
    assert (first["T"], first["history"], first["accumulate"], first["q0"]) == (T0, False, 0, False)
    assert (second["T"], second["history"], second["accumulate"], second["q0"]) == (T, True, 0, True)
    np.testing.assert_array_equal(first["u"], u[:T0].double().numpy())
    np.testing.assert_array_equal(second["u"], u[T0:].double().numpy())
    s = state_of(m)
    xb, Qb, _, _ = tr.rollout(s, x0.double().numpy(), u[:T0].double().numpy(), None, T0, 2, 2)
    close(torch.as_tensor(second["x0"]), xb)
    x, Q, hist, ls = tr.rollout(s, xb, u[T0:].double().numpy(), Qb, T, 2, 2)
    close(out.exponents, ls / T); close(out.x, x); close(out.q, Q); close(out.log_stretch, hist)
    assert out.log_stretch.shape == (4, c["B"], 2)
    with pytest.raises(AssertionError):
        m.lyapunov(x0, u[:-1], T, burn_in=T0)
    with pytest.raises(AssertionError):
        m.lyapunov(x0, u, T, burn_in=-1)


@cpu_only
def test_dt_scales_the_exponents(fake):
    m = small_model()
    x0, u = inputs(SMALL["T"])
    a, b = m.lyapunov(x0, u, SMALL["T"]), m.lyapunov(x0, u, SMALL["T"], dt=0.25)
    close(b.exponents, 4 * a.exponents.double().numpy(), atol=1e-6)
    assert torch.equal(a.q, b.q)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            m.lyapunov(x0, u, SMALL["T"], dt=bad)


@cpu_only
def test_continuation_from_the_returned_state_and_frame(fake):
    c = SMALL
    m = small_model()
    T, k = 8, 4
    x0, u = inputs(T)
    whole = m.lyapunov(x0, u, T, n_exponent=2, qr_every=2, return_history=True)
    head = m.lyapunov(x0, u[:k], k, n_exponent=2, qr_every=2, return_history=True)
    tail = m.lyapunov(head.x, u[k:], T - k, n_exponent=2, qr_every=2, q0=head.q, return_history=True)
    assert fake.calls[-1]["q0"] is True
    close(tail.x, whole.x.double().numpy(), atol=1e-6); close(tail.q, whole.q.double().numpy(), atol=1e-6)
    close(torch.cat([head.log_stretch, tail.log_stretch]), whole.log_stretch.double().numpy(), atol=1e-6)
    close((head.exponents * k + tail.exponents * (T - k)) / T, whole.exponents.double().numpy(), atol=1e-6)
    # q0 of one trial without its batch axis; a wrong shape is refused
    one = m.lyapunov(x0[1], u[:, 1], T, n_exponent=2, q0=torch.eye(c["xdim"], 2))
    assert one.q.shape == (1, c["xdim"], 2)
    with pytest.raises(AssertionError):
        m.lyapunov(x0, u, T, n_exponent=2, q0=torch.zeros(c["B"], c["xdim"], 3))


@cpu_only
def test_no_step(fake):
    c = SMALL
    m = small_model()
    x0, u = inputs(0)
    q0 = torch.randn(c["B"], c["xdim"], 2, generator=torch.Generator().manual_seed(5))
    out = m.lyapunov(x0, u, 0, n_exponent=2, q0=q0, return_history=True)
    assert torch.equal(out.x, x0) and out.log_stretch.shape == (0, c["B"], 2) and torch.isnan(out.exponents).all()
    close(out.q, tr.mgs(q0.double().numpy())[0])
    assert fake.calls[-1]["T"] == 0


@cpu_only
def test_refusals_of_the_python_surface(fake):
    c = SMALL
    m = small_model()
    x0, u = inputs(c["T"])
    for kw in (dict(n_exponent=0), dict(n_exponent=c["xdim"] + 1), dict(qr_every=0), dict(qr_every=-2)):
        with pytest.raises(ValueError):
            m.lyapunov(x0, u, c["T"], **kw)
    with pytest.raises(TypeError):
        m.lyapunov(x0, None, c["T"])
    with pytest.raises(AssertionError):
        m.lyapunov(x0, u, -1)
    with pytest.raises(AssertionError):
        m.lyapunov(x0[:, :-1], u, c["T"])
    with pytest.raises(AssertionError):
        m.lyapunov(x0, u[:, :-1], c["T"])
    assert fake.calls == []
    # a return code of the library surfaces as VjfError with the library's message
    fake.vjf_tangent_rollout = lambda *a: (setattr(fake, "err", b"vjf_tangent_rollout: refused") or -11)
    with pytest.raises(N.VjfError, match="vjf_tangent_rollout: refused"):
        m.lyapunov(x0, u, c["T"])


# ---------------------------------------------------------------------------------------------------- the real library's host code
def test_return_codes_of_the_entry_point():
    """Every refusal comes before the first launch, so the real entry point can be asked without a GPU: it reads no tensor."""
    L = N.lib()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)

    def call(x0=p, u=p, cen=p, x_out=p, q_out=p, lsum=p, lhist=None, T=5, B=2, n=9, d=5, dout=3, m=3, qr=1):
        return L.vjf_tangent_rollout(x0, u, None, cen, p, p, x_out, q_out, lsum, lhist, T, B, n, d, dout, m, qr, 0, None)
    for rc, kw in ((-1, dict(x0=None)), (-1, dict(cen=None)), (-1, dict(x_out=None)), (-1, dict(q_out=None)), (-1, dict(lsum=None)),
                   (-20, dict(T=-1)), (-20, dict(B=0)), (-20, dict(n=0)), (-20, dict(d=2)), (-20, dict(m=0)), (-20, dict(m=4)),
                   (-20, dict(qr=-1)), (-20, dict(qr=0, lhist=p)), (-21, dict(u=None)),
                   (-11, dict(n=1000, d=64, dout=64, m=64)),              # configs[4]'s dimensions with a full frame
                   (-11, dict(n=9, d=65, dout=65, m=1))):                 # dout beyond the kernel's 64
        assert call(**kw) == rc, kw
        assert b"vjf_tangent_rollout" in L.vjf_last_error()


def test_the_planner_admits_the_baseline_configs():
    """BASELINE configs[0]-[3]'s model dimensions with m = xdim in one pass; configs[4]'s (xdim 64, RBF 1000) with m >= 4; the LDS the
    plan asks for is what the layout in DESIGN.md section 3 adds up to and stays inside a workgroup's 160 KiB."""
    L = N.lib()
    vg, lds = C.c_int32(), C.c_int64()
    plan = lambda n, d, dout, m: L.vjf_tangent_plan(n, d, dout, m, C.byref(vg), C.byref(lds))      # noqa: E731

    def floats(n, d, dout, m, v, cl):
        doutp = (dout + 15) // 16 * 16
        return 17 * (n + d + 4 * doutp + m * dout + 2 * m + 4 * v * doutp) + 2 * n + (n * d + n * dout if cl else 0)
    for n, d, dout in ((100, 3, 3), (200, 10, 10), (200, 12, 10), (20, 3, 3)):
        assert plan(n, d, dout, dout) == 0 and vg.value == dout
        assert lds.value == 4 * floats(n, d, dout, dout, dout, True)
    for m in (1, 4, 8):
        assert plan(1000, 64, 64, m) == 0 and 1 <= vg.value <= m and lds.value <= 159 * 1024
        assert lds.value == 4 * floats(1000, 64, 64, m, vg.value, False)
        assert 4 * floats(1000, 64, 64, m, vg.value + 1, False) > 159 * 1024 or vg.value == m      # (as many per pass as fit)
    assert plan(1000, 64, 64, 64) == -11 and b"vjf_tangent_plan" in L.vjf_last_error()
    assert plan(9, 3, 3, 4) == -20 and plan(9, 2, 3, 1) == -20 and plan(0, 3, 3, 1) == -20
    assert L.vjf_tangent_plan(200, 10, 10, 10, None, None) == 0


def test_the_planner_follows_the_overrides(monkeypatch):
    L = N.lib()
    vg, lds, lds0 = C.c_int32(), C.c_int64(), C.c_int64()
    assert L.vjf_tangent_plan(200, 10, 10, 10, C.byref(vg), C.byref(lds)) == 0
    monkeypatch.setenv("VJF_FC_CENTROID_LDS", "0")
    assert L.vjf_tangent_plan(200, 10, 10, 10, C.byref(vg), C.byref(lds0)) == 0 and vg.value == 10
    assert lds.value - lds0.value == 4 * (200 * 10 + 200 * 10)
