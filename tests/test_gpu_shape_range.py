"""`fixed_points`, `smooth`, `sample_posterior` and `ekf` over the shape classes their planners admit and the family tests never run
(tests/shape_range_cases.py has the table: n < 9, xdim 2, 15, 16, 23, 25 to 32, udim = 8, the guaranteed corner, and the largest n
admitted at xdim 24, 27, 30 and 32, where a pass holds one column of A and the plan fills the LDS budget to the last KiB).

  1. parity of every op at every shape of its column against the fp64 reference, by the families' rule;
  2. exact properties at every shape: the smoother's last row and the EKF's head, symmetry, the diagonal, positivity, eigenvalues;
     three steps of the fixed-point search never worse than the start;
  3. bitwise invariances at x16u8, x27u8, x30u8 and corner: VJF_FC_CENTROID_LDS, the tile-mates, chunks joined by a head (a full
     covariance staged at dout > 24), the members per workgroup;
  4. a Cholesky pivot that fails at j >= 16: the trial is NaN, every other trial keeps its bits.

All tests need a real MI355X:  pytest -m gpu."""
import numpy as np
import pytest
import torch

from tests import ekf_cases as ec
from tests import fixed_point_cases as fpc
from tests import sampler_cases as pc
from tests import shape_range_cases as rc
from tests import smoother_cases as sc
from tests.margins import check_close

pytestmark = pytest.mark.gpu
EPS32 = sc.EPS32
INVARIANCE = ("x16u8", "x27u8", "x30u8", "corner")
# (op, shape) whose free plan keeps the centroids and w_mean in LDS (asserted in the test: a planner that moves one fails it)
CL_BY_PLAN = [(op, name) for name, ops in (("x16u8", rc.ALL), ("x27u8", rc.NO_EKF), ("x30u8", (rc.FP,))) for op in ops]


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_MODEL, _IN, _OUT = {}, {}, {}


def model_of(vjf, name):
    """One model per shape, shared by the four ops (smoother_cases' state: nothing is planted)."""
    if name not in _MODEL:
        _MODEL[name] = sc.make_model(vjf, name)
    return _MODEL[name]


def cuda(d):
    return {k: (torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def dev(op, name, kind="typical"):
    """The op's inputs of the shape as device tensors: once per module."""
    key = (op, name, kind)
    if key not in _IN:
        if op == rc.EKF:
            t = cuda(ec.inputs(name, kind))
            t["obs"] = torch.as_tensor(ec.observed(name)).cuda()
        elif op == rc.FP:
            t = cuda(rc.fp_inputs(name))
        else:
            t = cuda(sc.inputs(name, kind))
            t["z"] = torch.as_tensor(pc.noise(name)).cuda()
        _IN[key] = t
    return _IN[key]


def cut(t, rows, lo=0, hi=None):
    """(T, B, ...) -> its time rows [lo, hi) and trials `rows`, contiguous; None stays None."""
    if t is None:
        return None
    t = t[lo:hi]
    return (t if rows is None else t[:, rows]).contiguous()


def smooth(vjf, name, kind="typical", rows=None, lo=0, hi=None, after=None, **kw):
    t = dev(rc.SM, name, kind)
    hu = None if hi is None else hi + (after is not None)
    return model_of(vjf, name).smooth((cut(t["mu"], rows, lo, hi), cut(t["lv"], rows, lo, hi)), cut(t["u"], rows, lo, hu), state_var=sc.Q,
                                      after=after, **{"return_cov": True, **kw})


def sample(vjf, name, kind="typical", rows=None):
    t = dev(rc.SM, name, kind)
    z = t["z"] if rows is None else t["z"][:, :, rows].contiguous()
    return model_of(vjf, name).sample_posterior((cut(t["mu"], rows), cut(t["lv"], rows)), cut(t["u"], rows), z.shape[0], state_var=pc.Q, noise=z)


def ekf(vjf, name, regime="typical", gaps=True, rows=None, lo=0, hi=None, before=None, **kw):
    t = dev(rc.EKF, name, regime)
    x0, lv0 = (t["x0"], t["lv0"]) if rows is None else (t["x0"][rows].contiguous(), t["lv0"][rows].contiguous())
    start = {"x0": vjf.Gaussian(x0, lv0)} if before is None else {"before": before}
    return model_of(vjf, name).ekf(cut(t["y"], rows, lo, hi), cut(t["u"], rows, lo, hi), state_var=t["q"], obs_var=t["r"],
                                   observed=cut(t["obs"], rows, lo, hi) if gaps else None, **start, **{"return_cov": True, **kw})


def fixed_points(vjf, name, rows=None, **kw):
    t = dev(rc.FP, name)
    x0, u = t["x0"], t["u"]
    if rows is not None:
        x0, u = x0[rows].contiguous(), None if u is None else u[rows].contiguous()
    return model_of(vjf, name).fixed_points(x0, u, **kw)


CALL = {rc.SM: smooth, rc.SP: sample, rc.EKF: ekf, rc.FP: lambda vjf, name, kind=None, **kw: fixed_points(vjf, name, max_iter=3, **kw)}
KIND = {rc.SM: "mixed", rc.SP: "mixed", rc.EKF: "typical", rc.FP: None}          # the inputs of the invariance tests
FIELDS = {rc.SM: ("mean", "var", "cov"), rc.SP: ("x",), rc.EKF: ec.TENSORS, rc.FP: ("x", "residual", "converged", "n_iter", "jacobian")}
TRIAL_AXIS = {rc.SM: 1, rc.SP: 2, rc.EKF: 1, rc.FP: 0}


def full(vjf, op, name, kind=None, *more):
    """The undivided call of the op at the shape: once per module."""
    key = (op, name, kind) + more
    if key not in _OUT:
        _OUT[key] = CALL[op](vjf, name, kind, *more) if kind is not None else CALL[op](vjf, name)
        torch.cuda.synchronize()
    return _OUT[key]


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert torch.equal(a, b), f"{what}: differs"


def same_result(op, a, b, what, rows=None, lo=0, hi=None):
    """a against b's trials `rows` and (the sequences) time rows [lo, hi), bit for bit, and a's head against its own edge row."""
    for k in FIELDS[op]:
        want = getattr(b, k)
        if op in (rc.SM, rc.EKF):
            want = want[lo:hi]
        if rows is not None:
            want = want.index_select(TRIAL_AXIS[op], rows)
        same_bits(getattr(a, k), want, f"{what}: {k}")
    if op == rc.SM:
        same_bits(a.head[0], a.mean[0], f"{what}: head mean")
        same_bits(a.head[1], a.cov[0], f"{what}: head cov")
    elif op == rc.EKF:
        same_bits(a.head[0], a.mean[-1], f"{what}: head mean")
        same_bits(a.head[1], a.cov[-1], f"{what}: head cov")
    elif op == rc.SP:
        same_bits(a.head, a.x[:, 0], f"{what}: head")


def by_rule(op, what, got, b, ref64):
    """max|got - ref64| <= F[op] b, b the family's bound(); prints the achieved ratio before it asserts."""
    g = host(got).astype(np.float64)
    err = float(np.abs(g - ref64).max())
    print(f"shape-range margin: {op} {what}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {rc.F[op]})")
    check_close(g, np.asarray(ref64, np.float64), rtol=0, atol=rc.F[op] * b, what=f"{op} {what} [ratio = used * {rc.F[op]}]")


def spectrum_ok(cov, what):
    ev = np.linalg.eigvalsh(host(cov).astype(np.float64))
    print(f"{what}: smallest eigenvalue over the largest, worst {float((ev[..., 0] / ev[..., -1]).min()):.3e}")
    assert (ev[..., 0] >= -8 * EPS32 * ev[..., -1]).all()


# ------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("name,kind", rc.smooth_cases())
def test_smooth_parity_and_exact_properties(vjf, name, kind):
    xdim, udim, n, ydim, B, T = rc.shape(name)
    out = full(vjf, rc.SM, name, kind)
    assert out.mean.shape == (T, B, xdim) and out.var.shape == (T, B, xdim) and out.cov.shape == (T, B, xdim, xdim)
    ref = sc.references(name, kind)
    for what in ("mean", "var", "cov"):
        by_rule(rc.SM, f"{name} {kind} {what}", getattr(out, what), sc.bound(what, *ref[what]), ref[what][0])
    same_bits(out.mean[-1], dev(rc.SM, name, kind)["mu"][-1], "the last row's mean")
    lv = sc.inputs(name, kind)["lv"][-1]
    by_rule(rc.SM, f"{name} {kind} last var", out.var[-1], sc.bound("var", np.exp(lv.astype(np.float64)), np.exp(lv)), np.exp(lv.astype(np.float64)))
    same_bits(out.cov, out.cov.transpose(-1, -2), "cov against its transpose")
    same_bits(torch.diagonal(out.cov, dim1=-2, dim2=-1), out.var, "the diagonal of cov against var")
    same_bits(out.head[0], out.mean[0], "head mean")
    same_bits(out.head[1], out.cov[0], "head cov")
    assert bool((out.var > 0).all()) and bool(torch.isfinite(out.cov).all())
    spectrum_ok(out.cov, f"smooth {name} {kind}")


@pytest.mark.parametrize("name,kind", rc.sample_cases())
def test_sample_parity(vjf, name, kind):
    xdim, udim, n, ydim, B, T = rc.shape(name)
    out = full(vjf, rc.SP, name, kind)
    assert out.x.shape == (rc.MEMBERS[name], T, B, xdim) and out.x.dtype == torch.float32
    same_bits(out.head, out.x[:, 0], "head")
    r64, r32 = pc.references(name, kind)
    by_rule(rc.SP, f"{name} {kind} x", out.x, pc.bound(r64, r32), r64)


@pytest.mark.parametrize("name,regime,gaps", rc.ekf_cases())
def test_ekf_parity_and_exact_properties(vjf, name, regime, gaps):
    xdim, udim, n, ydim, B, T = rc.shape(name)
    out = full(vjf, rc.EKF, name, regime, gaps)
    assert out.mean.shape == (T, B, xdim) and out.cov.shape == (T, B, xdim, xdim) and out.loglik.shape == (T, B)
    ref = ec.references(name, regime, gaps)
    for what in ec.TENSORS:
        by_rule(rc.EKF, f"{name} {regime} {'gaps' if gaps else 'all'} {what}", getattr(out, what), ec.bound(what, *ref[what]), ref[what][0])
    if gaps:
        obs = dev(rc.EKF, name, regime)["obs"].bool()
        assert bool((out.loglik[~obs] == 0).all()) and bool((out.loglik[obs] != 0).all())
    same_bits(out.cov, out.cov.transpose(-1, -2), "cov against its transpose")
    same_bits(torch.diagonal(out.cov, dim1=-2, dim2=-1), out.var, "the diagonal of cov against var")
    same_bits(out.head[0], out.mean[-1], "head mean")
    same_bits(out.head[1], out.cov[-1], "head cov")
    assert bool((out.var > 0).all()) and bool(torch.isfinite(out.cov).all()) and bool(torch.isfinite(out.loglik).all())
    spectrum_ok(out.cov, f"ekf {name} {regime}")


@pytest.mark.parametrize("name", rc.names(rc.FP))
def test_fixed_points_one_step_and_never_worse(vjf, name):
    """One damped step (max_iter = 1, damping = 1) and the Jacobian against the fp64 reference; three steps never worse than the start."""
    xdim, udim, n, ydim, B, T = rc.shape(name)
    ref = rc.fp_references(name)
    out = fixed_points(vjf, name, max_iter=1, damping=1.0)
    assert out.x.shape == (B, xdim) and out.jacobian.shape == (B, xdim, xdim)
    for what in ("x", "residual", "jacobian"):
        by_rule(rc.FP, f"{name} one step {what}", getattr(out, what), fpc.bound(*ref[what]), ref[what][0])
    assert np.array_equal(host(out.n_iter), ref["n_iter"])
    more, start = (fixed_points(vjf, name, max_iter=k, return_jacobian=False) for k in (3, 0))
    same_bits(start.x, dev(rc.FP, name)["x0"], "max_iter = 0: x")
    assert bool((more.residual <= start.residual).all()) and bool((more.residual < start.residual).any())


# ------------------------------------------------------------------ 3
def test_the_plans_the_invariances_count_on():
    for name in INVARIANCE:
        for op in rc.SHAPES[name][2]:
            assert rc.form_of(op, name)[1] == ((op, name) in CL_BY_PLAN), (op, name)


@pytest.mark.parametrize("op,name", CL_BY_PLAN)
def test_bits_centroids_in_global_memory(vjf, op, name, monkeypatch):
    whole = full(vjf, op, name, KIND[op])
    monkeypatch.setenv("VJF_FC_CENTROID_LDS", "0")
    same_result(op, CALL[op](vjf, name, *([KIND[op]] if KIND[op] else [])), whole, "VJF_FC_CENTROID_LDS=0")


@pytest.mark.parametrize("op,name", [(op, name) for name in INVARIANCE for op in rc.SHAPES[name][2]])
def test_bits_do_not_depend_on_the_tile_mates(vjf, op, name):
    whole = full(vjf, op, name, KIND[op])
    for lo, hi in ((0, 1), (0, 16), (16, 17)):
        rows = torch.arange(lo, hi).cuda()
        same_result(op, CALL[op](vjf, name, *([KIND[op]] if KIND[op] else []), rows=rows), whole, f"trials [{lo}:{hi}]", rows)


@pytest.mark.parametrize("name", INVARIANCE)
def test_bits_smooth_in_two_chunks(vjf, name):
    whole = full(vjf, rc.SM, name, "mixed")
    T = rc.shape(name)[5]
    for k in (T // 2, T - 1):
        back = smooth(vjf, name, "mixed", lo=k)
        front = smooth(vjf, name, "mixed", hi=k, after=back.head)
        same_result(rc.SM, back, whole, f"rows [{k}:]", lo=k)
        same_result(rc.SM, front, whole, f"rows [:{k}] with after", hi=k)


@pytest.mark.parametrize("name", [name for name in INVARIANCE if rc.EKF in rc.SHAPES[name][2]])
def test_bits_ekf_in_two_chunks(vjf, name):
    whole = full(vjf, rc.EKF, name, "typical")
    T = rc.shape(name)[5]
    for k in (T // 2, 1):
        front = ekf(vjf, name, hi=k)
        back = ekf(vjf, name, lo=k, before=front.head)
        same_result(rc.EKF, front, whole, f"rows [:{k}]", hi=k)
        same_result(rc.EKF, back, whole, f"rows [{k}:] with before", lo=k)


@pytest.mark.parametrize("name", INVARIANCE)
def test_bits_one_member_per_workgroup(vjf, name, monkeypatch):
    whole = full(vjf, rc.SP, name, "mixed")
    monkeypatch.setenv("VJF_SMS_MEMBERS", "1")
    same_result(rc.SP, sample(vjf, name, "mixed"), whole, "VJF_SMS_MEMBERS=1")


# ------------------------------------------------------------------ 4
def poisoned(cov, pivots):
    """`cov` (B, dout, dout) with the trials of `pivots` replaced by their own L D L^T, D[j, j] = -1: indefinite from pivot j on."""
    cov = cov.clone()
    for trial, j in pivots.items():
        cov[trial] = torch.as_tensor(rc.indefinite(host(cov[trial]), j)).cuda()
    return cov


@pytest.mark.parametrize("name", list(rc.PIVOTS))
def test_smooth_a_pivot_failing_beyond_the_first_sixteen(vjf, name):
    """Runs to completion: an indefinite `after` covariance is data the library documents, not a fault."""
    whole = full(vjf, rc.SM, name, "typical")
    B, k, pivots = rc.shape(name)[4], 2, rc.PIVOTS[name]
    others = torch.tensor([r for r in range(B) if r not in pivots]).cuda()
    out = smooth(vjf, name, hi=k, after=(whole.mean[k], poisoned(whole.cov[k], pivots)))
    torch.cuda.synchronize()
    for f in ("mean", "var", "cov"):
        same_bits(getattr(out, f)[:, others], getattr(whole, f)[:k, others], f"{f} of the other trials")
        for trial, j in pivots.items():
            assert bool(torch.isnan(getattr(out, f)[:, trial]).all()), f"{f} of trial {trial}, pivot {j}"
    for trial, j in pivots.items():
        assert bool(torch.isnan(out.head[0][trial]).all()) and bool(torch.isnan(out.head[1][trial]).all()), f"head of trial {trial}, pivot {j}"


@pytest.mark.parametrize("name", list(rc.PIVOTS))
def test_ekf_a_pivot_failing_beyond_the_first_sixteen(vjf, name):
    """With the gap pattern: rows 2 and 3 of trials 9 and 13 are not observed, so their means there are predictions, which read no
    covariance -- NaN only because the failed pivot was seen."""
    whole = full(vjf, rc.EKF, name, "typical")
    B, k, pivots = rc.shape(name)[4], 2, rc.PIVOTS[name]
    others = torch.tensor([r for r in range(B) if r not in pivots]).cuda()
    out = ekf(vjf, name, lo=k, before=(whole.mean[k - 1], poisoned(whole.cov[k - 1], pivots)))
    torch.cuda.synchronize()
    for f in ec.TENSORS:
        same_bits(getattr(out, f)[:, others], getattr(whole, f)[k:, others], f"{f} of the other trials")
        for trial, j in pivots.items():
            assert bool(torch.isnan(getattr(out, f)[:, trial]).all()), f"{f} of trial {trial}, pivot {j}"
    for trial, j in pivots.items():
        assert bool(torch.isnan(out.head[0][trial]).all()) and bool(torch.isnan(out.head[1][trial]).all()), f"head of trial {trial}, pivot {j}"
