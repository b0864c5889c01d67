"""`lyapunov` / `jacobian` (vjf_tangent_rollout): the tangent dynamics of the learned mean map in one native call.

  1. parity of exponents, x, q and log_stretch against the fp64 reference (tests/tangent_cases.py: the cases, the rule);
  2. `jacobian` against the fp64 reference;
  3. the log-determinant identity on the GPU's own sums;
  4. bitwise properties: permuted rows, sub-batches, chunking, a split horizon, another stream, the forms of the kernel;
  5. orthonormality of the returned frame;
  6. the final x against `forecast_sequence` without noise (the same map on another kernel);
  7. no side effects on the model or the generators;
  8. refusals;  9. n_step = 0.

All tests need a real MI355X:  pytest -m gpu."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tangent_cases as tc
from tests import tangent_ref as tr
from tests.margins import check_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_CACHE, _REFS = {}, {}


def case(vjf, name):
    """(model, {x0, u} as device tensors, the fp64 twin of the model's state): built once per module."""
    if name not in _CACHE:
        m = tc.make_model(vjf, name)
        t = {k: None if v is None else torch.as_tensor(v).cuda() for k, v in tc.inputs(name).items()}
        _CACHE[name] = (m, t, tc.model_state(m))
    return _CACHE[name]


def refs(vjf, name, mm, qr):
    """{tensor: (ref64, ref32)} of the whole horizon of the case: computed once, never modified."""
    if (name, mm, qr) not in _REFS:
        m, t, s64 = case(vjf, name)
        a = tc.inputs(name)
        _REFS[name, mm, qr] = tc.references(s64, a["x0"], a["u"], tc.CASES[name][5], mm, qr)
    return _REFS[name, mm, qr]


def same_bits(a, b, what=""):
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} against {tuple(b.shape)}"
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), \
        f"{what}: differs by {float((a.double() - b.double()).abs().max()):.3e}"


def by_rule(what, got, ref64, other, F=tc.F):
    """max|got - ref64| <= F max(E, 8 eps max(1, max|ref64|)), E = max|other - ref64|; prints the achieved ratio before it asserts."""
    b = tc.bound(ref64, other)
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    err = float(np.abs(g - ref64).max())
    print(f"tangent margin: {what}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    check_close(g, np.asarray(ref64, np.float64), rtol=0, atol=F * b, what=f"{what} [ratio = used * {F}]")


def dims(name, m):
    xdim, udim, n, ydim, B, T = tc.CASES[name]
    return xdim, B, T, (xdim if m is None else m)


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("m,qr", tc.PARITY)
@pytest.mark.parametrize("name", list(tc.CASES))
def test_parity_against_the_fp64_reference(vjf, name, m, qr):
    xdim, B, T, mm = dims(name, m)
    model, t, _ = case(vjf, name)
    r = refs(vjf, name, mm, qr)
    out = model.lyapunov(t["x0"], t["u"], T, n_exponent=mm, qr_every=qr, return_history=True)
    assert out.exponents.shape == (B, mm) and out.x.shape == (B, xdim) and out.q.shape == (B, xdim, mm)
    assert out.log_stretch.shape == (-(-T // qr), B, mm)
    tag = f"{name} m={mm} qr={qr}"
    by_rule(f"{tag} exponents", out.exponents, r["lsum"][0] / T, r["lsum"][1].astype(np.float64) / T)
    by_rule(f"{tag} x", out.x, *r["x"])
    by_rule(f"{tag} q", out.q, *r["q"])
    by_rule(f"{tag} log_stretch", out.log_stretch, *r["log_stretch"])


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", list(tc.CASES))
def test_jacobian_against_the_fp64_reference(vjf, name):
    xdim, B, T, _ = dims(name, None)
    model, t, s64 = case(vjf, name)
    a = tc.inputs(name)
    u0 = None if a["u"] is None else a["u"][0]
    J = model.jacobian(t["x0"], None if t["u"] is None else t["u"][0])
    assert J.shape == (B, xdim, xdim)
    c = lambda v, dt: None if v is None else np.asarray(v, dt)          # noqa: E731
    J64 = tr.jacobian(s64, c(a["x0"], np.float64), c(u0, np.float64))
    J32 = tr.jacobian(s64.cast(np.float32), a["x0"], u0)
    assert np.abs(J64 - np.eye(xdim)).max() > 0.05           # (not the identity map)
    by_rule(f"{name} jacobian", J, J64, J32)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", list(tc.CASES))
def test_log_determinant_identity(vjf, name):
    """m = xdim: sum_v lsum[b, v] is sum_t log|det J_t| along the trajectory, whatever the intervals are (qr_every = 3)."""
    xdim, B, T, mm = dims(name, None)
    model, t, s64 = case(vjf, name)
    a = tc.inputs(name)
    out = model.lyapunov(t["x0"], t["u"], T, qr_every=3)
    got = (out.exponents.double() * T).sum(1)
    want = tc.logdet_sum(s64, a["x0"].astype(np.float64), None if a["u"] is None else a["u"].astype(np.float64), T)
    by_rule(f"{name} sum of log-stretches", got, want, refs(vjf, name, mm, 3)["lsum"][1].astype(np.float64).sum(1))


# ------------------------------------------------------------------ 4
BITWISE = ["ragged3", "wide"]


def run(model, t, T, rows=None, x0=None, q0=None, t0=0, m=None, qr=3):
    """lyapunov on the case's inputs with the history: steps t0 .. t0 + T - 1, trials `rows` (an index tensor)."""
    pick = (lambda a: a) if rows is None else (lambda a: a[:, rows].contiguous())
    u = None if t["u"] is None else pick(t["u"][t0:t0 + T])
    x0 = t["x0"] if x0 is None else x0
    if rows is not None:
        x0 = x0[rows].contiguous()
        q0 = None if q0 is None else q0[rows].contiguous()
    return model.transition.lyapunov(x0, u, T, n_exponent=m, qr_every=qr, q0=q0, return_history=True)


def full_run(vjf, name):
    model, t, _ = case(vjf, name)
    return run(model, t, tc.CASES[name][5])


@pytest.fixture(scope="module")
def full(vjf):
    return {name: full_run(vjf, name) for name in BITWISE}


def same_result(a, b, what, rows=None):
    for k in ("exponents", "x", "q", "log_stretch"):
        want = getattr(b, k)
        if rows is not None:
            want = want[:, rows] if k == "log_stretch" else want[rows]
        same_bits(getattr(a, k), want, f"{what}: {k}")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_permuted_rows(vjf, full, name):
    model, t, _ = case(vjf, name)
    perm = torch.randperm(t["x0"].shape[0], generator=torch.Generator().manual_seed(3)).cuda()
    same_result(run(model, t, tc.CASES[name][5], rows=perm), full[name], "permuted rows", perm)


def test_bits_sub_batches(vjf, full):
    """Rows 3 .. 19 of ragged3 (two tiles, both ragged) and a single trial."""
    model, t, _ = case(vjf, "ragged3")
    T = tc.CASES["ragged3"][5]
    for lo, hi in ((3, 20), (35, 36)):
        rows = torch.arange(lo, hi).cuda()
        same_result(run(model, t, T, rows=rows), full["ragged3"], f"trials [{lo}:{hi}]", rows)


@pytest.mark.parametrize("name", BITWISE)
def test_bits_chunking(vjf, full, name, monkeypatch):
    """Launches of six steps (two intervals of three) against one launch; of two (shorter than an interval: cut inside it) as well."""
    model, t, _ = case(vjf, name)
    for chunk in ("6", "2"):
        monkeypatch.setenv("VJF_FC_CHUNK", chunk)
        same_result(run(model, t, tc.CASES[name][5]), full[name], f"VJF_FC_CHUNK={chunk}")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_split_horizon(vjf, full, name):
    """T steps in one call = k steps, then T - k from the returned x and q with the sums carried; k a multiple of qr_every = 3."""
    model, t, _ = case(vjf, name)
    T = tc.CASES[name][5]
    k = 24 if T > 24 else 12
    head = run(model, t, k)
    tail = run(model, t, T - k, x0=head.x, q0=head.q, t0=k)
    whole = full[name]
    same_bits(torch.cat([head.log_stretch, tail.log_stretch]), whole.log_stretch, "history rows")
    same_bits(tail.x, whole.x, "x")
    same_bits(tail.q, whole.q, "q")
    # the sums carried: the raw entry point goes on from head's sums
    from vjf_amd import _native as N
    vel = model.transition.velocity
    B, xdim = t["x0"].shape
    n, d = vel.feature.centroid.shape
    # (exponents * k need not give back the sums' bits: the head's history summed in interval order does, as the kernel sums it)
    lsum = torch.zeros_like(head.exponents)
    for row in head.log_stretch:
        lsum = lsum + row
    x, q = torch.empty_like(head.x), torch.empty_like(head.q)
    u = None if t["u"] is None else t["u"][k:].contiguous()
    p = N.ptr
    assert N.lib().vjf_tangent_rollout(p(head.x), p(u), p(head.q), p(vel.feature.centroid), p(vel.feature.logwidth), p(vel.w_mean), p(x),
                                       p(q), p(lsum), None, T - k, B, n, d, xdim, xdim, 3, 1, None) == 0
    torch.cuda.synchronize()
    same_bits(lsum / T, whole.exponents, "carried sums")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_other_stream(vjf, full, name):
    model, t, _ = case(vjf, name)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = run(model, t, tc.CASES[name][5])
    side.synchronize()
    same_result(out, full[name], "side stream")


@pytest.mark.parametrize("env", ["VJF_FC_LOOKAHEAD", "VJF_FC_CENTROID_LDS"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_bits_the_forms_of_the_kernel_agree(vjf, name, env, monkeypatch):
    """The forms for shapes beyond the register / LDS budgets, forced at the test shapes: the same MFMA steps on the same operands in
    the same order, so the same bits -- and so the parity above holds for them."""
    model, t, _ = case(vjf, name)
    T = tc.CASES[name][5]
    want = run(model, t, T)
    monkeypatch.setenv(env, "0")
    same_result(run(model, t, T), want, f"{env}=0")


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("name", list(tc.CASES))
def test_the_returned_frame_is_orthonormal(vjf, name):
    """|Q^T Q - I| of the GPU's frame against the fp32 reference's own deviation, under the rule."""
    xdim, B, T, mm = dims(name, None)
    model, t, _ = case(vjf, name)
    out = model.lyapunov(t["x0"], t["u"], T, qr_every=3)
    gram = lambda Q: np.einsum("bjv,bjw->bvw", Q, Q) - np.eye(Q.shape[2])          # noqa: E731
    r64, r32 = refs(vjf, name, mm, 3)["q"]
    by_rule(f"{name} Q^T Q - I", gram(out.q.double().cpu().numpy()), gram(r64), gram(r32.astype(np.float64)))


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("name", list(tc.CASES))
def test_final_state_against_forecast_sequence(vjf, name):
    """The same map on another kernel: forecast_sequence with zero weight noise and no state noise ends where lyapunov ends.  The two
    final states against each other under the rule's bound of x (E from the fp32 reference), and lyapunov's against the fp64
    trajectory with E the roll-out kernel's own distance from it.  Every case: the two kernels share one x step and one planner of
    its forms, `beyond256` being the shape at which both have to take the streamed one."""
    xdim, udim, n, ydim, B, T = tc.CASES[name]
    model, t, _ = case(vjf, name)
    xs = model.transition.forecast_sequence(t["x0"], t["u"], T, w_noise=torch.zeros(T, n, xdim, device="cuda"))
    out = model.lyapunov(t["x0"], t["u"], T, n_exponent=1, qr_every=4)
    x64, x32 = refs(vjf, name, xdim, 1)["x"]
    b = tc.bound(x64, x32)
    got, other = out.x.double().cpu().numpy(), xs[-1].double().cpu().numpy()
    err = float(np.abs(got - other).max())
    print(f"tangent margin: {name} x minus forecast_sequence's x: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {tc.F})")
    check_close(got, other, rtol=0, atol=tc.F * b, what=f"{name} x minus forecast_sequence's x [ratio = used * {tc.F}]")
    by_rule(f"{name} x against forecast_sequence", out.x, x64, other)


# ------------------------------------------------------------------ 7
def test_no_side_effects(vjf):
    model, t, _ = case(vjf, "control")
    model._ensure_ctx(t["x0"].shape[0])
    before = model._blob.clone()
    counters = (model.transition.n_sample, model.likelihood.n_sample)
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    model.lyapunov(t["x0"], t["u"], tc.CASES["control"][5], qr_every=2, burn_in=0, return_history=True)
    model.jacobian(t["x0"], t["u"][0])
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), model._blob.view(torch.int32))
    assert (model.transition.n_sample, model.likelihood.n_sample) == counters
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(gpu_rng, torch.cuda.get_rng_state())
    assert model.status() == 0


# ------------------------------------------------------------------ 8
def test_refusals(vjf):
    from vjf_amd import _native as N
    L = N.lib()
    model, t, _ = case(vjf, "control")
    xdim, udim, n, ydim, B, T = tc.CASES["control"]
    with pytest.raises(ValueError):
        model.lyapunov(t["x0"], t["u"], T, n_exponent=xdim + 1)
    with pytest.raises(ValueError):
        model.lyapunov(t["x0"], t["u"], T, qr_every=-1)
    with pytest.raises(TypeError):
        model.lyapunov(t["x0"], None, T)
    with pytest.raises(AssertionError):
        model.lyapunov(t["x0"], t["u"][:-1], T)
    vel = model.transition.velocity
    x, q, lsum = torch.empty(B, xdim, device="cuda"), torch.empty(B, xdim, xdim, device="cuda"), torch.zeros(B, xdim, device="cuda")
    hist = torch.empty(T, B, xdim, device="cuda")
    p = N.ptr

    def call(x0=t["x0"], u=t["u"], T=T, B=B, n=n, d=xdim + udim, dout=xdim, m=xdim, qr=1, lhist=None):
        return L.vjf_tangent_rollout(p(x0), p(u), None, p(vel.feature.centroid), p(vel.feature.logwidth), p(vel.w_mean), p(x), p(q),
                                     p(lsum), p(lhist), T, B, n, d, dout, m, qr, 0, None)
    for rc, kw in ((-1, dict(x0=None)), (-20, dict(m=xdim + 1)), (-20, dict(m=0)), (-20, dict(qr=-1)), (-20, dict(qr=0, lhist=hist)),
                   (-20, dict(T=-1)), (-20, dict(B=0)), (-21, dict(u=None)),
                   (-11, dict(n=1000, d=64, dout=64, m=64, u=None))):       # configs[4]'s dimensions with a full frame
        assert call(**kw) == rc, kw                      # (every refusal comes before the first launch: nothing is read or written)
        assert b"vjf_tangent_rollout" in L.vjf_last_error()
    vg, lds = ctypes.c_int32(), ctypes.c_int64()
    assert L.vjf_tangent_plan(1000, 64, 64, 64, ctypes.byref(vg), ctypes.byref(lds)) == -11
    assert L.vjf_tangent_plan(1000, 64, 64, 4, ctypes.byref(vg), ctypes.byref(lds)) == 0 and 1 <= vg.value <= 4 and lds.value <= 159 * 1024
    assert call() == 0
    torch.cuda.synchronize()
    same_bits(lsum / T, model.lyapunov(t["x0"], t["u"], T).exponents, "raw call")


# ------------------------------------------------------------------ 9
def test_no_step(vjf):
    """n_step = 0: x0 itself, q0 orthonormalised once (its log R_vv in no history row), exponents NaN."""
    xdim, udim, n, ydim, B, T = tc.CASES["wide"]
    model, t, _ = case(vjf, "wide")
    q0 = torch.randn(B, xdim, 5, generator=torch.Generator().manual_seed(11)).cuda()
    out = model.lyapunov(t["x0"], t["u"][:0], 0, n_exponent=5, q0=q0, return_history=True)
    same_bits(out.x, t["x0"], "x")
    assert out.log_stretch.shape == (0, B, 5) and torch.isnan(out.exponents).all()
    Q64, _ = tr.mgs(q0.double().cpu().numpy())
    Q32, _ = tr.mgs(q0.cpu().numpy())
    by_rule("n_step = 0 frame", out.q, Q64, Q32)
