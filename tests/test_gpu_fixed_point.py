"""`fixed_points` (vjf_fixed_points): the fixed points of the learned mean map in one native call.

  1. one damped step against the fp64 reference (tests/fixed_point_cases.py: the cases, the rule);
  2. convergence of the near starts: every trial, the fp64 residual of the returned x, the reported residual;
  3. the distance of the returned x to the true root (fp64 Newton from it);
  4. `jacobian` against the fp64 reference at the returned x;
  5. bitwise properties: permuted rows, sub-batches, tile-mates, another stream, a repeat;
  6. never worse than the start;  7. max_iter = 0, a NaN row, a root as the start;
  8. refusals through the real library and no side effects.

All tests need a real MI355X:  pytest -m gpu."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import fixed_point_cases as fpc
from tests import fixed_point_ref as fr
from tests import tangent_cases as tc
from tests.margins import check_close

pytestmark = pytest.mark.gpu
NAMES = list(fpc.CASES)
F = fpc.F


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_CACHE = {}


def case(vjf, name):
    """(model, {kind: {x0, u} as device tensors}, the fp64 twin of the model's state): built once per module."""
    if name not in _CACHE:
        m = fpc.make_model(vjf, name)
        t = {kind: {k: None if v is None else torch.as_tensor(v).cuda() for k, v in fpc.inputs(name, kind).items()} for kind in fpc.PERT}
        _CACHE[name] = (m, t, tc.model_state(m))
    return _CACHE[name]


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def same_bits(a, b, what=""):
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} against {tuple(b.shape)}"
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert torch.equal(a, b), f"{what}: differs"


def same_result(a, b, what, rows=None):
    for k in ("x", "residual", "converged", "n_iter", "jacobian"):
        want = getattr(b, k)
        same_bits(getattr(a, k), want if rows is None else want[rows], f"{what}: {k}")


def by_rule(what, got, ref64, other):
    """max|got - ref64| <= F max(E, 8 eps max(1, max|ref64|)), E = max|other - ref64|; prints the achieved ratio before it asserts."""
    b = fpc.bound(ref64, other)
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    err = float(np.abs(g - ref64).max())
    print(f"fixed-point margin: {what}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    check_close(g, np.asarray(ref64, np.float64), rtol=0, atol=F * b, what=f"{what} [ratio = used * {F}]")


def by_ratio(what, ratio):
    """ratio <= F per trial, the ratio being an error over its own bound; prints the worst before it asserts."""
    ratio = np.asarray(ratio, np.float64)
    print(f"fixed-point margin: {what}: worst ratio {ratio.max():.3f} (F = {F})")
    check_close(np.maximum(ratio, 0.0), np.zeros_like(ratio), rtol=0, atol=F, what=f"{what} [ratio = used * {F}]")


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", NAMES)
def test_one_step_against_the_fp64_reference(vjf, name):
    """max_iter = 1, damping = 1 (K is well conditioned): the kernel's g, A, A^T A, Cholesky factor and solves, not the problem's
    conditioning."""
    model, t, s64 = case(vjf, name)
    a = fpc.inputs(name, "far")
    out = model.fixed_points(t["far"]["x0"], t["far"]["u"], max_iter=1, damping=1.0)
    r64, r32 = fpc.references(s64, a["x0"], a["u"], max_iter=1, tol=fpc.TOL, lam0=1.0)
    assert np.abs(r64[0] - a["x0"]).max() > 1e-2          # (a step was taken)
    by_rule(f"{name} one step x", out.x, r64[0], r32[0])
    by_rule(f"{name} one step residual", out.residual, r64[1], r32[1])
    assert np.array_equal(host(out.n_iter), r64[2])


# ------------------------------------------------------------------ 2, 3, 4
_NEAR = {}


def near(vjf, name):
    """The convergence run of the case, once: near starts, tol = 1e-5, max_iter = 40."""
    if name not in _NEAR:
        model, t, _ = case(vjf, name)
        _NEAR[name] = model.fixed_points(t["near"]["x0"], t["near"]["u"], max_iter=fpc.MAX_ITER, tol=fpc.TOL)
        torch.cuda.synchronize()
    return _NEAR[name]


@pytest.mark.parametrize("name", NAMES)
def test_near_starts_converge(vjf, name):
    model, t, s64 = case(vjf, name)
    xdim, udim, n, ydim, B, T = fpc.CASES[name]
    out = near(vjf, name)
    assert out.x.shape == (B, xdim) and out.residual.shape == (B,) and out.n_iter.dtype == torch.int32 and out.converged.dtype == torch.bool
    print(f"{name}: n_iter max {int(out.n_iter.max())}, residual max {float(out.residual.max()):.3e}")
    assert bool(out.converged.all()) and int(out.n_iter.max()) <= fpc.MAX_ITER
    Eg, g64 = fpc.g_error(s64, host(out.x), host(t["near"]["u"]))
    res64 = np.sqrt((g64 * g64).sum(1))
    by_ratio(f"{name} fp64 residual of x beyond tol", (res64 - fpc.TOL) / Eg)
    by_ratio(f"{name} reported residual", np.abs(host(out.residual).astype(np.float64) - res64) / Eg)


@pytest.mark.parametrize("name", NAMES)
def test_distance_to_the_true_root(vjf, name):
    """x** = fp64 Newton from the returned x (residual < 1e-13):  |x - x**| <= 1.5 |A(x**)^-1|_2 |g64(x)|, the first-order bound with
    half again for the curvature term; a trial is left out only where cond(A(x**)) > 1e5, at most a tenth of the case's."""
    model, t, s64 = case(vjf, name)
    out = near(vjf, name)
    dist, lim, cond = fpc.root_distance(s64, host(out.x), host(t["near"]["u"]))
    keep = cond <= 1e5
    assert (~keep).sum() <= len(keep) // 10, f"cond(A) > 1e5 in {(~keep).sum()} of {len(keep)} trials"
    print(f"{name}: cond median {np.median(cond):.1f} max {cond.max():.1f}; worst |x - x**| / bound {(dist / lim)[keep].max():.3f}")
    assert (dist[keep] <= lim[keep]).all()


@pytest.mark.parametrize("name", NAMES)
def test_jacobian_against_the_fp64_reference(vjf, name):
    model, t, s64 = case(vjf, name)
    xdim, udim, n, ydim, B, T = fpc.CASES[name]
    out = near(vjf, name)
    assert out.jacobian.shape == (B, xdim, xdim)
    x, u = host(out.x), host(t["near"]["u"])
    c = lambda v, dt: None if v is None else np.asarray(v, dt)          # noqa: E731
    J64 = fr.jacobian(s64, c(x, np.float64), c(u, np.float64))
    J32 = fr.jacobian(s64.cast(np.float32), x, u)
    assert np.abs(J64 - np.eye(xdim)).max() > 0.02           # (not the identity map: `wide` has the smallest A, 0.043)
    by_rule(f"{name} jacobian", out.jacobian, J64, J32)
    no = model.fixed_points(t["near"]["x0"], t["near"]["u"], max_iter=fpc.MAX_ITER, tol=fpc.TOL, return_jacobian=False)
    assert no.jacobian is None
    same_bits(no.x, out.x, "x without the Jacobian")


# ------------------------------------------------------------------ 5
BITWISE = ["ragged3", "wide", "control"]


def run(model, t, rows=None, x0=None, **kw):
    kw = {"max_iter": 3, **kw}
    x0 = t["x0"] if x0 is None else x0
    u = t["u"]
    if rows is not None:
        x0, u = x0[rows].contiguous(), None if u is None else u[rows].contiguous()
    return model.transition.fixed_points(x0, u, **kw)


@contextlib.contextmanager
def own_stream():
    """A stream of the test's own, destroyed behind it.  A stream from torch's pool lives for the rest of the process, and every live
    stream that has run something holds a share of the runtime's few hardware queues: three more of them before the filter routes'
    tests moved the streams of the multi-stream route onto one queue, where its kernels wait for each other until they time out
    (tests/test_gpu_parity.py::test_nonfinite_component_on_the_sharded_route failed on that)."""
    with open("/proc/self/maps") as f:
        path = sorted({line.split()[-1] for line in f if "libamdhip64" in line})[0]
    hip, s = ctypes.CDLL(path), ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        yield torch.cuda.ExternalStream(s.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(s) == 0


@pytest.fixture(scope="module")
def full(vjf):
    return {name: run(case(vjf, name)[0], case(vjf, name)[1]["far"]) for name in BITWISE}


@pytest.mark.parametrize("name", BITWISE)
def test_bits_permuted_rows_repeat_and_stream(vjf, full, name):
    model, t, _ = case(vjf, name)
    perm = torch.randperm(t["far"]["x0"].shape[0], generator=torch.Generator().manual_seed(3)).cuda()
    same_result(run(model, t["far"], rows=perm), full[name], "permuted rows", perm)
    same_result(run(model, t["far"]), full[name], "a repeat")
    torch.cuda.synchronize()
    with own_stream() as side:
        with torch.cuda.stream(side):
            out = run(model, t["far"])
        side.synchronize()
    same_result(out, full[name], "side stream")


def test_bits_sub_batches(vjf, full):
    """Rows 3 .. 19 of ragged3 (two tiles, both ragged) and a single trial."""
    model, t, _ = case(vjf, "ragged3")
    for lo, hi in ((3, 20), (35, 36)):
        rows = torch.arange(lo, hi).cuda()
        same_result(run(model, t["far"], rows=rows), full["ragged3"], f"trials [{lo}:{hi}]", rows)


@pytest.mark.parametrize("name", ["ragged3", "control"])
def test_bits_do_not_depend_on_the_tile_mates(vjf, full, name):
    """Far starts, max_iter = 3: a trial beside tile-mates that converge at once (planted roots) or never (NaN rows)."""
    model, t, _ = case(vjf, name)
    x0 = t["far"]["x0"]
    roots = torch.as_tensor(fpc.roots(name), dtype=torch.float32).cuda()
    for mates in (roots[torch.arange(x0.shape[0]) % len(roots)], torch.full_like(x0, float("nan"))):
        mixed = mates.clone()
        keep = torch.tensor([1, 6, 17, x0.shape[0] - 1]).cuda()
        mixed[keep] = x0[keep]
        out = run(model, t["far"], x0=mixed)
        for k in ("x", "residual", "converged", "n_iter", "jacobian"):
            same_bits(getattr(out, k)[keep], getattr(full[name], k)[keep], f"{k} beside other tile-mates")


@pytest.mark.parametrize("name", NAMES)
def test_bits_the_forms_of_the_kernel_agree(vjf, name, monkeypatch):
    """The form for shapes beyond the LDS budget (centroids and w_mean read from global memory), forced at the test shapes: the same
    MFMA steps on the same operands in the same order, so the same bits -- and so the parity above holds for it."""
    model, t, _ = case(vjf, name)
    want = run(model, t["far"], max_iter=6)
    monkeypatch.setenv("VJF_FC_CENTROID_LDS", "0")
    same_result(run(model, t["far"], max_iter=6), want, "VJF_FC_CENTROID_LDS=0")


def test_at_the_limit_of_xdim(vjf):
    """xdim = 32 (VJF_FP_MAXDOUT): two full rows per lane in the per-trial linear algebra, columns of A in several passes.  One damped
    step against the fp64 reference as in test 1, and three steps never worse than the start."""
    from tests import forecast_cases as fc
    from tests.helpers import model_arrays
    xdim, n, ydim, B = 32, 45, 9, 19
    torch.manual_seed(5)
    model = vjf.VJF.make_model(ydim, xdim, 0, n, fc.HIDDEN, likelihood="gaussian")
    views = model_arrays(model)
    for k, a in fc.synthetic_state(1900, xdim, 0, n, ydim).items():
        views[k].copy_(torch.as_tensor(a).reshape(views[k].shape).to(views[k].device))
    views["w_mean"].mul_(tc.W_SCALE)
    s64 = tc.model_state(model)
    x0 = np.random.default_rng(1901).uniform(-1.5, 1.5, (B, xdim)).astype(np.float32)
    out = model.fixed_points(torch.as_tensor(x0).cuda(), max_iter=1, damping=1.0)
    r64, r32 = fpc.references(s64, x0, None, max_iter=1, tol=fpc.TOL, lam0=1.0)
    assert np.abs(r64[0] - x0).max() > 1e-2
    by_rule("xdim = 32 one step x", out.x, r64[0], r32[0])
    by_rule("xdim = 32 one step residual", out.residual, r64[1], r32[1])
    by_rule("xdim = 32 jacobian", out.jacobian, fr.jacobian(s64, r64[0]), fr.jacobian(s64.cast(np.float32), r32[0]))
    more, start = (model.fixed_points(torch.as_tensor(x0).cuda(), max_iter=k, return_jacobian=False) for k in (3, 0))
    assert bool((more.residual <= start.residual).all()) and bool((more.residual < start.residual).any())


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("name", NAMES)
def test_never_worse_than_the_start(vjf, name):
    model, t, _ = case(vjf, name)
    out = run(model, t["far"], return_jacobian=False)
    start = run(model, t["far"], max_iter=0, return_jacobian=False)
    assert bool((out.residual <= start.residual).all())
    assert bool((out.n_iter[~out.converged] == 3).all()) and bool((out.n_iter <= 3).all())
    assert bool((~out.converged).any())                      # (three steps from a far start do not end every search)


# ------------------------------------------------------------------ 7
def test_edge_cases(vjf):
    model, t, s64 = case(vjf, "control")
    x0, u = t["far"]["x0"], t["far"]["u"]
    out = run(model, t["far"], max_iter=0)
    same_bits(out.x, x0, "max_iter = 0: x")
    assert not bool(out.converged.any()) and int(out.n_iter.max()) == 0
    g0 = fr.g_and_A(s64, host(x0).astype(np.float64), host(u).astype(np.float64))[0]
    np.testing.assert_allclose(host(out.residual), np.sqrt((g0 * g0).sum(1)), rtol=1e-4)
    # a NaN row returns itself and leaves its tile-mates' bits alone
    clean = run(model, t["far"], max_iter=5)
    bad = x0.clone()
    bad[4, 1] = float("nan")
    got = run(model, t["far"], x0=bad, max_iter=5)
    others = torch.tensor([r for r in range(x0.shape[0]) if r != 4]).cuda()
    for k in ("x", "residual", "converged", "n_iter", "jacobian"):
        same_bits(getattr(got, k)[others], getattr(clean, k)[others], f"{k} beside a NaN row")
    same_bits(got.x[4], bad[4], "the NaN row's x")
    assert bool(torch.isinf(got.residual[4])) and not bool(got.converged[4])
    # a planted root as the start
    roots = torch.as_tensor(fpc.roots("control"), dtype=torch.float32).cuda()
    at = model.fixed_points(roots, u[:len(roots)], max_iter=fpc.MAX_ITER, tol=fpc.TOL)
    assert bool(at.converged.all()) and int(at.n_iter.max()) <= 1


# ------------------------------------------------------------------ 8
def test_refusals_and_no_side_effects(vjf):
    from vjf_amd import _native as N
    L = N.lib()
    model, t, _ = case(vjf, "control")
    xdim, udim, n, ydim, B, T = fpc.CASES["control"]
    x0, u = t["near"]["x0"], t["near"]["u"]
    model._ensure_ctx(B)
    before = model._blob.clone()
    counters = (model.transition.n_sample, model.likelihood.n_sample)
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    with pytest.raises(TypeError):
        model.fixed_points(x0)
    for kw in (dict(max_iter=-1), dict(tol=0.0), dict(damping=float("inf"))):
        with pytest.raises(ValueError):
            model.fixed_points(x0, u, **kw)
    vel = model.transition.velocity
    new = lambda *s, dtype=torch.float32: torch.empty(*s, device="cuda", dtype=dtype)      # noqa: E731
    x, res, nit, conv = new(B, xdim), new(B), new(B, dtype=torch.int32), new(B, dtype=torch.int32)
    p = N.ptr

    def call(x0=x0, u=u, B=B, n=n, d=xdim + udim, dout=xdim, max_iter=fpc.MAX_ITER, tol=fpc.TOL, lam0=1e-3):
        return L.vjf_fixed_points(p(x0), p(u), p(vel.feature.centroid), p(vel.feature.logwidth), p(vel.w_mean), p(x), p(res), p(nit), p(conv),
                                  None, B, n, d, dout, max_iter, tol, lam0, None)
    for rc, kw in ((-1, dict(x0=None)), (-20, dict(max_iter=-1)), (-20, dict(tol=0.0)), (-20, dict(lam0=float("nan"))), (-20, dict(B=0)),
                   (-21, dict(u=None)), (-11, dict(n=9, d=33, dout=33, u=None)), (-11, dict(n=1000, d=64, dout=64, u=None)),
                   (-11, dict(n=3000, d=3, dout=3, u=None))):
        assert call(**kw) == rc, kw                      # (every refusal comes before the first launch: nothing is read or written)
        assert b"vjf_fixed_points" in L.vjf_last_error()
    lds = ctypes.c_int64()
    assert L.vjf_fixed_points_plan(9, 33, 33, ctypes.byref(lds)) == -11
    assert L.vjf_fixed_points_plan(200, 10, 10, ctypes.byref(lds)) == 0 and lds.value <= 159 * 1024
    assert call() == 0
    torch.cuda.synchronize()
    out = near(vjf, "control")
    same_bits(x, out.x, "raw call: x")
    same_bits(res, out.residual, "raw call: residual")
    assert torch.equal(nit, out.n_iter) and torch.equal(conv != 0, out.converged)
    assert torch.equal(before.view(torch.int32), model._blob.view(torch.int32))
    assert (model.transition.n_sample, model.likelihood.n_sample) == counters
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(gpu_rng, torch.cuda.get_rng_state())
    assert model.status() == 0
