"""CPU side of the `fixed_points` tests: the host logic of vjf_amd/model.py (argument order, shapes and dtypes of the result, a Gaussian
start, the coercion of u, every refusal, `unique`, no write to the model) through a stand-in for vjf_fixed_points built on
tests/fixed_point_ref.py in fp64, and the planner and the return codes of the real library (host-only code: no GPU is touched before a
refusal)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fake_backend
from tests import fixed_point_cases as fpc
from tests import fixed_point_ref as fr
from tests import tile_layouts
from tests.fake_backend import _arr
from oracle import vjf_oracle as orc
from vjf_amd import _native as N

cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="the stand-in backend works on CPU tensors")


def _iarr(p, n):
    return np.ctypeslib.as_array((C.c_int32 * int(n)).from_address(p.value))


class FixedPointLib(fake_backend.FakeLib):
    """FakeLib + vjf_fixed_points: fixed_point_ref.solve in fp64 on the fp32 values it is handed, stored as fp32 / int32, behind the
    entry point's own argument checks.  Records every call's arguments in `calls`."""
    def __init__(self):
        super().__init__()
        self.calls = []

    def vjf_fixed_points(self, x0, u, cen, lw, w_mean, x, residual, n_iter, converged, jac, B, n, d, dout, max_iter, tol, lam0, stream):
        null = lambda p: p is None or not p.value                                                 # noqa: E731
        if any(null(p) for p in (x0, cen, lw, w_mean, x, residual, n_iter, converged)):
            self.err = b"vjf_fixed_points: null tensor"
            return -1
        if B < 1 or n < 1 or dout < 1 or d < dout or max_iter < 0 or not 0 < tol < np.inf or not 0 < lam0 < np.inf:
            self.err = b"vjf_fixed_points: bad shape"
            return -20
        du = d - dout
        if du > 0 and null(u):
            self.err = b"vjf_fixed_points: u is required when d > dout"
            return -21
        f = lambda p, *shape: _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        s = orc.OracleState(1, dout, du, n, (1,), orc.GAUSSIAN)
        s.centroid, s.logwidth, s.w_mean = f(cen, n, d), f(lw, n), f(w_mean, n, dout)
        U = f(u, B, du) if du > 0 else None
        self.calls.append(dict(B=B, n=n, d=d, dout=dout, max_iter=max_iter, tol=tol, lam0=lam0, jac=not null(jac), x0=f(x0, B, dout), u=U))
        X, res, nit, conv, _ = fr.solve(s, f(x0, B, dout), U, max_iter, tol, lam0)
        _arr(x, B * dout).reshape(B, dout)[...] = X
        _arr(residual, B)[...] = res
        _iarr(n_iter, B)[...] = nit
        _iarr(converged, B)[...] = conv
        if not null(jac):
            _arr(jac, B * dout * dout).reshape(B, dout, dout)[...] = fr.jacobian(s, X, U)
        return 0


@pytest.fixture
def fake():
    old = N._lib
    N._lib = FixedPointLib()
    yield N._lib
    N._lib = old


SMALL = dict(xdim=3, udim=2, n=9, ydim=5, B=6)


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


def inputs(udim=SMALL["udim"], seed=3):
    g = torch.Generator().manual_seed(seed)
    return 0.5 * torch.randn(SMALL["B"], SMALL["xdim"], generator=g), (torch.randn(SMALL["B"], udim, generator=g) if udim else None)


def close(a, b, atol=2e-6):
    np.testing.assert_allclose(a.detach().cpu().numpy().astype(np.float64), np.asarray(b, np.float64), rtol=0, atol=atol)


# ---------------------------------------------------------------------------------------------------- the host logic
@cpu_only
def test_shapes_dtypes_defaults_and_argument_order(fake):
    c = SMALL
    m = small_model()
    x0, u = inputs()
    out = m.fixed_points(x0, u)
    assert type(out).__name__ == "FixedPointResult" and out._fields == ("x", "residual", "converged", "n_iter", "jacobian")
    assert out.x.shape == (c["B"], c["xdim"]) and out.residual.shape == (c["B"],) and out.converged.shape == (c["B"],)
    assert out.n_iter.shape == (c["B"],) and out.jacobian.shape == (c["B"], c["xdim"], c["xdim"])
    assert (out.x.dtype, out.residual.dtype, out.converged.dtype, out.n_iter.dtype, out.jacobian.dtype) == \
        (torch.float32, torch.float32, torch.bool, torch.int32, torch.float32)
    call, = fake.calls
    assert (call["B"], call["n"], call["d"], call["dout"], call["max_iter"], call["jac"]) == (c["B"], c["n"], c["xdim"] + c["udim"], c["xdim"], 64, True)
    assert call["tol"] == pytest.approx(1e-5) and call["lam0"] == pytest.approx(1e-3)
    np.testing.assert_array_equal(call["x0"], x0.double().numpy())
    np.testing.assert_array_equal(call["u"], u.double().numpy())
    s = state_of(m)
    X, res, nit, conv, _ = fr.solve(s, x0.double().numpy(), u.double().numpy(), 64, 1e-5, 1e-3)
    close(out.x, X); close(out.residual, res); close(out.jacobian, fr.jacobian(s, X, u.double().numpy()))
    assert np.array_equal(out.n_iter.numpy(), nit) and np.array_equal(out.converged.numpy(), conv)
    # the keywords reach the library; float64 and list inputs are coerced; no Jacobian when it is not asked for
    out = m.fixed_points(x0.double().tolist(), u.double(), max_iter=3, tol=1e-3, damping=0.5, return_jacobian=False)
    call = fake.calls[-1]
    assert (call["max_iter"], call["jac"]) == (3, False) and call["tol"] == pytest.approx(1e-3) and call["lam0"] == 0.5
    assert out.jacobian is None and (out.n_iter <= 3).all()
    # the transition's own method is the same call
    out2 = m.transition.fixed_points(x0, u, max_iter=3, tol=1e-3, damping=0.5, return_jacobian=False)
    assert torch.equal(out2.x, out.x) and torch.equal(out2.residual, out.residual)


@cpu_only
def test_a_gaussian_start_stands_for_its_mean(fake):
    import vjf_amd
    m = small_model()
    x0, u = inputs()
    a, b = m.fixed_points(vjf_amd.Gaussian(x0, torch.full_like(x0, -2.0)), u, max_iter=4), m.fixed_points(x0, u, max_iter=4)
    assert torch.equal(a.x, b.x) and torch.equal(a.jacobian, b.jacobian)


@cpu_only
def test_coercion_of_u(fake):
    c = SMALL
    m = small_model()
    x0, u = inputs()
    # one trial given 1-D
    one = m.fixed_points(x0[2], u[2], max_iter=4)
    assert one.x.shape == (1, c["xdim"]) and one.jacobian.shape == (1, c["xdim"], c["xdim"])
    assert torch.equal(one.x[0], m.fixed_points(x0, u, max_iter=4).x[2])
    # a model without a control input takes no u
    m0 = small_model(udim=0)
    assert m0.fixed_points(x0, max_iter=2).x.shape == (c["B"], c["xdim"]) and fake.calls[-1]["u"] is None
    with pytest.raises(TypeError):
        m.fixed_points(x0)
    with pytest.raises(AssertionError):
        m.fixed_points(x0, u[:-1])
    with pytest.raises(AssertionError):
        m.fixed_points(x0, u[:, :-1])
    with pytest.raises(AssertionError):
        m.fixed_points(x0[:, :-1], u)


@cpu_only
def test_refusals_of_the_python_surface(fake):
    import vjf_amd
    m = small_model()
    x0, u = inputs()
    for kw in (dict(max_iter=-1), dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")), dict(damping=0.0),
               dict(damping=-1e-3), dict(damping=float("nan")), dict(damping=float("inf"))):
        with pytest.raises(ValueError):
            m.fixed_points(x0, u, **kw)
    assert fake.calls == []
    big = vjf_amd.VJF.make_model(5, 33, 0, 9, [4], likelihood="gaussian")
    with pytest.raises(NotImplementedError, match="32"):
        big.fixed_points(torch.zeros(2, 33))
    assert fake.calls == []
    # a return code of the library surfaces as VjfError with the library's message
    fake.vjf_fixed_points = lambda *a: (setattr(fake, "err", b"vjf_fixed_points: refused") or -11)
    with pytest.raises(N.VjfError, match="vjf_fixed_points: refused"):
        m.fixed_points(x0, u)


@cpu_only
def test_no_write_to_the_model_or_the_generators(fake):
    m = small_model()
    x0, u = inputs()
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if isinstance(v, torch.Tensor)}
    counters = (m.transition.n_sample, m.likelihood.n_sample)
    rng = torch.get_rng_state()
    x0c, uc = x0.clone(), u.clone()
    m.fixed_points(x0, u, max_iter=5)
    after = m.state_dict()
    assert all(torch.equal(v, after[k]) for k, v in before.items())
    assert (m.transition.n_sample, m.likelihood.n_sample) == counters and torch.equal(rng, torch.get_rng_state())
    assert torch.equal(x0, x0c) and torch.equal(u, uc)


def test_unique_counts_and_order():
    from vjf_amd.model import FixedPointResult
    x = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 5e-4], [9.0, 9.0], [1.0, 1.0 + 2e-3], [1.0002, 1.0], [0.0, 0.0]])
    conv = torch.tensor([True, True, True, False, True, True, True])
    J = torch.arange(7 * 4, dtype=torch.float32).reshape(7, 2, 2)
    r = FixedPointResult(x, torch.zeros(7), conv, torch.zeros(7, dtype=torch.int32), J)
    ux, uj, count = r.unique()
    assert torch.equal(ux, x[[0, 1, 4]]) and torch.equal(uj, J[[0, 1, 4]]) and count.tolist() == [3, 2, 1]      # (row 3 has not converged)
    ux, uj, count = r.unique(merge_tol=0.1)
    assert torch.equal(ux, x[[0, 1]]) and count.tolist() == [3, 3]
    ux, uj, count = r._replace(jacobian=None).unique(merge_tol=1e-5)
    assert uj is None and torch.equal(ux, x[[0, 1, 2, 4, 5]]) and count.tolist() == [2, 1, 1, 1, 1]
    none = r._replace(converged=torch.zeros(7, dtype=torch.bool)).unique()
    assert none[0].shape == (0, 2) and none[1].shape == (0, 2, 2) and none[2].tolist() == []


# ---------------------------------------------------------------------------------------------------- the real library's host code
def test_return_codes_of_the_entry_point():
    """Every refusal comes before the first launch, so the real entry point can be asked without a GPU: it reads no tensor."""
    L = N.lib()
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)

    def call(x0=p, u=p, cen=p, x=p, res=p, nit=p, conv=p, B=2, n=9, d=5, dout=3, max_iter=5, tol=1e-5, lam0=1e-3):
        return L.vjf_fixed_points(x0, u, cen, p, p, x, res, nit, conv, None, B, n, d, dout, max_iter, tol, lam0, None)
    for rc, kw in ((-1, dict(x0=None)), (-1, dict(cen=None)), (-1, dict(x=None)), (-1, dict(res=None)), (-1, dict(nit=None)),
                   (-1, dict(conv=None)), (-20, dict(B=0)), (-20, dict(n=0)), (-20, dict(d=2)), (-20, dict(dout=0)), (-20, dict(max_iter=-1)),
                   (-20, dict(tol=0.0)), (-20, dict(tol=-1.0)), (-20, dict(tol=float("nan"))), (-20, dict(tol=float("inf"))),
                   (-20, dict(lam0=0.0)), (-20, dict(lam0=float("nan"))), (-20, dict(lam0=float("inf"))), (-21, dict(u=None)),
                   (-11, dict(n=9, d=33, dout=33)),                       # dout beyond the kernel's 32
                   (-11, dict(n=1000, d=64, dout=64)),                    # configs[4]'s dimensions
                   (-11, dict(n=3000, d=3, dout=3))):                     # an n that cannot fit
        assert call(**kw) == rc, kw
        assert b"vjf_fixed_points" in L.vjf_last_error()


def test_the_planner_admits_the_cases_and_the_baseline_config():
    """The five case shapes and configs[1]'s dimensions are accepted, the LDS the plan asks for is what the layout in DESIGN.md
    section 3 adds up to and stays inside a workgroup's 160 KiB; dout = 33 and an n that cannot fit are refused."""
    L = N.lib()
    lds = C.c_int64()
    plan = lambda n, d, dout: L.vjf_fixed_points_plan(n, d, dout, C.byref(lds))      # noqa: E731

    floats = tile_layouts.fixed_points
    shapes = [(n, xdim + udim, xdim) for xdim, udim, n, ydim, B, T in fpc.CASES.values()] + [(200, 10, 10), (100, 3, 3)]
    for n, d, dout in shapes:
        assert plan(n, d, dout) == 0, (n, d, dout)
        assert lds.value <= 159 * 1024
        if dout <= 10:                                                    # every column of A in one pass, the shared operands in LDS
            assert lds.value == 4 * floats(n, d, dout, dout, True)
        else:                                                             # (wide: 17 columns of two output tiles do not fit one pass)
            vgs = [vg for vg in range(1, dout + 1) if lds.value == 4 * floats(n, d, dout, vg, True)]
            assert len(vgs) == 1 and (vgs[0] == dout or 4 * floats(n, d, dout, vgs[0] + 1, True) > 159 * 1024)
    # dout = 32 fits beside a few hundred features, with fewer columns per pass
    assert plan(200, 32, 32) == 0 and lds.value <= 159 * 1024
    assert any(lds.value == 4 * floats(200, 32, 32, vg, False) for vg in range(1, 33))
    assert plan(9, 33, 33) == -11 and b"vjf_fixed_points_plan" in L.vjf_last_error() and b"32" in L.vjf_last_error()
    assert plan(3000, 3, 3) == -11 and b"vjf_fixed_points_plan" in L.vjf_last_error() and b"LDS" in L.vjf_last_error()
    assert plan(1000, 64, 64) == -11
    assert plan(9, 2, 3) == -20 and plan(0, 3, 3) == -20 and plan(9, 3, 0) == -20
    assert L.vjf_fixed_points_plan(200, 10, 10, None) == 0
