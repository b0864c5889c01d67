"""`smooth` (vjf_smooth): the extended Rauch-Tung-Striebel pass over a filtered sequence in one native call.

  1. parity of mean, var and cov against the fp64 reference (tests/smoother_cases.py: the cases, the kinds, the rule);
  2. exact properties: the last row, T = 1, symmetry, the diagonal, positivity, return_cov = False;
  3. `tiny` variances and a huge state noise return the filtered mean;
  4. bitwise invariances: the row index, the batch size, the tile-mates, the stream, VJF_FC_CENTROID_LDS, chunks with `after`;
  5. poisoning: a NaN row and an indefinite after-covariance;
  6. refusals through the real library and no side effects.

All tests need a real MI355X:  pytest -m gpu."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import smoother_cases as sc
from tests.margins import check_close

pytestmark = pytest.mark.gpu
NAMES = list(sc.CASES)
KINDS = list(sc.KINDS)
F = sc.F
EPS32 = sc.EPS32


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_MODEL, _IN, _OUT = {}, {}, {}


def model_of(vjf, name):
    if name not in _MODEL:
        _MODEL[name] = sc.make_model(vjf, name)
    return _MODEL[name]


def dev(name, kind="typical"):
    """{mu, lv, u} of the case as device tensors: once per module."""
    if (name, kind) not in _IN:
        _IN[(name, kind)] = {k: None if v is None else torch.as_tensor(v).cuda() for k, v in sc.inputs(name, kind).items()}
    return _IN[(name, kind)]


def full(vjf, name, kind="typical"):
    """The undivided call of the case with the covariances: once per module."""
    if (name, kind) not in _OUT:
        t = dev(name, kind)
        _OUT[(name, kind)] = model_of(vjf, name).smooth((t["mu"], t["lv"]), t["u"], state_var=sc.Q, return_cov=True)
        torch.cuda.synchronize()
    return _OUT[(name, kind)]


def run(vjf, name, kind="typical", rows=None, lo=0, hi=None, mu=None, **kw):
    """`smooth` on the trials `rows` and the time rows [lo, hi) of the case (u cut to match, one more row with `after`)."""
    t = dev(name, kind)
    mu = t["mu"] if mu is None else mu
    lv, u = t["lv"], t["u"]
    hi = mu.shape[0] if hi is None else hi
    hu = hi + (kw.get("after") is not None)
    mu, lv, u = mu[lo:hi], lv[lo:hi], None if u is None else u[lo:hu]
    if rows is not None:
        mu, lv, u = mu[:, rows], lv[:, rows], None if u is None else u[:, rows]
    kw = {"state_var": sc.Q, "return_cov": True, **kw}
    return model_of(vjf, name).transition.smooth((mu.contiguous(), lv.contiguous()), None if u is None else u.contiguous(), **kw)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def same_bits(a, b, what=""):
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} against {tuple(b.shape)}"
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f"{what}: differs"


def same_result(a, b, what, rows=None, lo=0, hi=None):
    """a against b's trials `rows` and time rows [lo, hi), bit for bit: mean, var, cov and (lo = 0) the head."""
    for k in ("mean", "var", "cov"):
        want = getattr(b, k)[lo:hi]
        same_bits(getattr(a, k), want if rows is None else want[:, rows], f"{what}: {k}")
    same_bits(a.head[0], a.mean[0], f"{what}: head mean")
    same_bits(a.head[1], a.cov[0], f"{what}: head cov")


def by_rule(what, tensor, got, ref64, other):
    """max|got - ref64| <= F max(E, 8 eps scale), E = max|other - ref64|; prints the achieved ratio before it asserts."""
    b = sc.bound(tensor, ref64, other)
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    err = float(np.abs(g - ref64).max())
    print(f"smoother margin: {what}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    check_close(g, np.asarray(ref64, np.float64), rtol=0, atol=F * b, what=f"{what} [ratio = used * {F}]")


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_parity_against_the_fp64_reference(vjf, name, kind):
    xdim, udim, n, ydim, B, T = sc.CASES[name]
    out = full(vjf, name, kind)
    assert out.mean.shape == (T, B, xdim) and out.var.shape == (T, B, xdim) and out.cov.shape == (T, B, xdim, xdim)
    assert out.head[1].shape == (B, xdim, xdim)
    ref = sc.references(name, kind)
    for what in ("mean", "var", "cov"):
        by_rule(f"{name} {kind} {what}", what, getattr(out, what), *ref[what])


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_exact_properties(vjf, name, kind):
    out = full(vjf, name, kind)
    t = dev(name, kind)
    same_bits(out.mean[-1], t["mu"][-1], "the last row's mean")
    lv = sc.inputs(name, kind)["lv"][-1]
    by_rule(f"{name} {kind} last var", "var", out.var[-1], np.exp(lv.astype(np.float64)), np.exp(lv))
    same_bits(out.cov, out.cov.transpose(-1, -2), "cov against its transpose")
    same_bits(torch.diagonal(out.cov, dim1=-2, dim2=-1), out.var, "the diagonal of cov against var")
    same_bits(out.head[0], out.mean[0], "head mean")
    same_bits(out.head[1], out.cov[0], "head cov")
    assert bool((out.var > 0).all()) and bool(torch.isfinite(out.cov).all())
    ev = np.linalg.eigvalsh(host(out.cov).astype(np.float64))
    worst = float((ev[..., 0] / ev[..., -1]).min())
    print(f"{name} {kind}: smallest eigenvalue over the largest, worst {worst:.3e}")
    assert (ev[..., 0] >= -8 * EPS32 * ev[..., -1]).all()
    no = run(vjf, name, kind, return_cov=False)
    assert no.cov is None
    same_bits(no.mean, out.mean, "mean without cov")
    same_bits(no.var, out.var, "var without cov")
    same_bits(no.head[1], out.cov[0], "head cov without cov")


@pytest.mark.parametrize("name", ["control", "x24"])
def test_one_row_returns_the_filtered_moments(vjf, name):
    t = dev(name)
    T = t["mu"].shape[0]
    one = run(vjf, name, lo=T - 1)
    whole = full(vjf, name)
    same_bits(one.mean[0], t["mu"][-1], "T = 1: mean")
    same_result(one, whole, "T = 1", lo=T - 1)
    off = one.cov[0] - torch.diag_embed(one.var[0])
    assert bool((off == 0).all())


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", NAMES)
def test_tiny_variances_return_the_filtered_mean(vjf, name):
    out = full(vjf, name, "tiny")
    ref = sc.references(name, "tiny")
    b = sc.bound("mean", *ref["mean"])
    err = float((out.mean - dev(name, "tiny")["mu"]).abs().max())
    print(f"smoother margin: {name} tiny mean against the filtered: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    assert err <= F * b


@pytest.mark.parametrize("name", ["control", "wide", "scalar"])
def test_a_huge_state_noise_returns_the_filtered_moments(vjf, name):
    a = sc.inputs(name)
    out = run(vjf, name, state_var=1e12)
    mu64 = a["mu"].astype(np.float64)
    b = 8 * EPS32 * max(1.0, float(np.abs(mu64).max()))
    err = float(np.abs(host(out.mean) - mu64).max())
    print(f"smoother margin: {name} state_var = 1e12 mean: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    assert err <= F * b
    by_rule(f"{name} state_var = 1e12 var", "var", out.var, np.exp(a["lv"].astype(np.float64)), np.exp(a["lv"]))


# ------------------------------------------------------------------ 4
@contextlib.contextmanager
def own_stream():
    """A stream of the test's own, destroyed behind it (tests/test_gpu_fixed_point.py says why it is not one of torch's pool)."""
    with open("/proc/self/maps") as f:
        path = sorted({line.split()[-1] for line in f if "libamdhip64" in line})[0]
    hip, s = ctypes.CDLL(path), ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        yield torch.cuda.ExternalStream(s.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(s) == 0


@pytest.mark.parametrize("name", ["ragged3", "control", "wide"])
def test_bits_row_index_repeat_and_stream(vjf, name):
    whole = full(vjf, name, "mixed")
    B = sc.CASES[name][4]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).cuda()
    same_result(run(vjf, name, "mixed", rows=perm), whole, "permuted trials", perm)
    same_result(run(vjf, name, "mixed"), whole, "a repeat")
    torch.cuda.synchronize()
    with own_stream() as side:
        with torch.cuda.stream(side):
            out = run(vjf, name, "mixed")
        side.synchronize()
    same_result(out, whole, "side stream")


@pytest.mark.parametrize("B", [1, 15, 16, 17, 37])
def test_bits_batch_size(vjf, B):
    """The first B trials of ragged3 (37 trials) and B trials from its middle: a trial's rows do not depend on the batch."""
    whole = full(vjf, "ragged3")
    for lo in (0, 37 - B):
        rows = torch.arange(lo, lo + B).cuda()
        same_result(run(vjf, "ragged3", rows=rows), whole, f"trials [{lo}:{lo + B}]", rows)


@pytest.mark.parametrize("name", ["ragged3", "control"])
def test_bits_do_not_depend_on_the_tile_mates(vjf, name):
    """Four trials beside tile-mates whose means are others' (shifted by 3) or NaN."""
    whole = full(vjf, name)
    mu = dev(name)["mu"]
    keep = torch.tensor([1, 6, 17, mu.shape[1] - 1]).cuda()
    for mates in (mu + 3.0, torch.full_like(mu, float("nan"))):
        mixed = mates.clone()
        mixed[:, keep] = mu[:, keep]
        out = run(vjf, name, mu=mixed)
        for k in ("mean", "var", "cov"):
            same_bits(getattr(out, k)[:, keep], getattr(whole, k)[:, keep], f"{k} beside other tile-mates")


@pytest.mark.parametrize("name", NAMES)
def test_bits_the_forms_of_the_kernel_agree(vjf, name, monkeypatch):
    """The form for shapes beyond the LDS budget (centroids and w_mean read from global memory), forced at the test shapes."""
    whole = full(vjf, name, "mixed")
    monkeypatch.setenv("VJF_FC_CENTROID_LDS", "0")
    same_result(run(vjf, name, "mixed"), whole, "VJF_FC_CENTROID_LDS=0")


@pytest.mark.parametrize("name", ["control", "x24", "ragged3"])
def test_bits_chunked_with_after(vjf, name):
    whole = full(vjf, name)
    T = sc.CASES[name][5]
    for k in (T // 2, 1, T - 1):
        back = run(vjf, name, lo=k)
        front = run(vjf, name, hi=k, after=back.head)
        same_result(back, whole, f"rows [{k}:]", lo=k)
        same_result(front, whole, f"rows [:{k}] with after", hi=k)
        # the head of a call without the covariances, and `after` as (mean[k], cov[k]) of the undivided call
        front = run(vjf, name, hi=k, after=run(vjf, name, lo=k, return_cov=False).head)
        same_result(front, whole, f"rows [:{k}] after a head without cov", hi=k)
        same_result(run(vjf, name, hi=k, after=(whole.mean[k], whole.cov[k])), whole, f"rows [:{k}] after (mean[k], cov[k])", hi=k)
    # a row at a time
    head = None
    for t in range(T - 1, max(T - 9, -1), -1):
        r = run(vjf, name, lo=t, hi=t + 1, after=head)
        same_result(r, whole, f"row {t} alone", lo=t, hi=t + 1)
        head = r.head
    # only the lower triangle of the after-covariance is read
    junk = whole.cov[2] + torch.triu(torch.full_like(whole.cov[2], float("nan")), 1)
    same_result(run(vjf, name, hi=2, after=(whole.mean[2], junk)), whole, "junk above the diagonal", hi=2)


# ------------------------------------------------------------------ 5
def test_poisoning_by_a_nan_row(vjf):
    name = "control"
    whole = full(vjf, name)
    T, bad, t0 = sc.CASES[name][5], 5, sc.CASES[name][5] // 2
    others = torch.tensor([r for r in range(sc.CASES[name][4]) if r != bad]).cuda()
    for field in ("mu", "lv", "u"):
        t = {k: (None if v is None else v.clone()) for k, v in dev(name).items()}
        t[field][t0 + (field == "u"), bad, 1] = float("nan")          # (u[t0 + 1] drives the step out of row t0)
        out = model_of(vjf, name).smooth((t["mu"], t["lv"]), t["u"], state_var=sc.Q, return_cov=True)
        for k in ("mean", "var", "cov"):
            got, want = getattr(out, k), getattr(whole, k)
            same_bits(got[:, others], want[:, others], f"NaN in {field}: {k} of the other trials")
            same_bits(got[t0 + 1:, bad], want[t0 + 1:, bad], f"NaN in {field}: {k} behind the row")
            assert bool(torch.isnan(got[:t0 + 1, bad]).all()), f"NaN in {field}: {k} from the row back"
        assert bool(torch.isnan(out.head[1][bad]).all())
    # the last row itself
    t = {k: (None if v is None else v.clone()) for k, v in dev(name).items()}
    t["lv"][T - 1, bad, 0] = float("inf")
    out = model_of(vjf, name).smooth((t["mu"], t["lv"]), t["u"], state_var=sc.Q, return_cov=True)
    assert bool(torch.isnan(out.mean[:, bad]).all()) and bool(torch.isnan(out.cov[:, bad]).all())
    same_bits(out.mean[:, others], whole.mean[:, others], "inf in the last lv: the other trials")


def test_poisoning_by_an_indefinite_after_covariance(vjf):
    name = "control"
    whole = full(vjf, name)
    k, bad = 7, 5
    others = torch.tensor([r for r in range(sc.CASES[name][4]) if r != bad]).cuda()
    cov = whole.cov[k].clone()
    cov[bad] = -cov[bad]
    out = run(vjf, name, hi=k, after=(whole.mean[k], cov))
    for f in ("mean", "var", "cov"):
        same_bits(getattr(out, f)[:, others], getattr(whole, f)[:k, others], f"indefinite after_cov: {f} of the other trials")
        assert bool(torch.isnan(getattr(out, f)[:, bad]).all())
    mean = whole.mean[k].clone()
    mean[bad, 0] = float("nan")
    out = run(vjf, name, hi=k, after=(mean, whole.cov[k]))
    same_bits(out.mean[:, others], whole.mean[:k, others], "NaN in after_mean: the other trials")
    assert bool(torch.isnan(out.mean[:, bad]).all()) and bool(torch.isnan(out.var[:, bad]).all())


# ------------------------------------------------------------------ 6
def test_refusals_and_no_side_effects(vjf):
    from vjf_amd import _native as N
    L = N.lib()
    name = "control"
    model = model_of(vjf, name)
    xdim, udim, n, ydim, B, T = sc.CASES[name]
    t = dev(name)
    model._ensure_ctx(B)
    state = model.get_state()
    before = model._blob.clone()
    counters = (model.transition.n_sample, model.likelihood.n_sample)
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    with pytest.raises(TypeError):
        model.smooth((t["mu"], t["lv"]))
    with pytest.raises(AssertionError):
        model.smooth((t["mu"], t["lv"]), t["u"][:-1])
    for sv in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            model.smooth((t["mu"], t["lv"]), t["u"], state_var=sv)
    vel = model.transition.velocity
    new = lambda *s: torch.empty(*s, device="cuda", dtype=torch.float32)      # noqa: E731
    mean, var, cov0 = new(T, B, xdim), new(T, B, xdim), new(B, xdim, xdim)
    p = N.ptr

    def call(mu=t["mu"], u=t["u"], am=None, ac=None, T=T, B=B, n=n, d=xdim + udim, dout=xdim, sv=sc.Q):
        return L.vjf_smooth(p(mu), p(t["lv"]), p(u), p(vel.feature.centroid), p(vel.feature.logwidth), p(vel.w_mean), p(am), p(ac), p(mean),
                            p(var), None, p(cov0), T, B, n, d, dout, sv, None)
    for rc, kw in ((-1, dict(mu=None)), (-20, dict(T=0)), (-20, dict(sv=0.0)), (-20, dict(sv=float("nan"))), (-20, dict(B=0)),
                   (-20, dict(am=mean[0])), (-20, dict(ac=cov0)), (-21, dict(u=None)), (-11, dict(n=9, d=33, dout=33, u=None)),
                   (-11, dict(n=1000, d=64, dout=64, u=None)), (-11, dict(n=3000, d=3, dout=3, u=None))):
        assert call(**kw) == rc, kw                      # (every refusal comes before the first launch: nothing is read or written)
        assert b"vjf_smooth" in L.vjf_last_error()
    lds = ctypes.c_int64()
    assert L.vjf_smooth_plan(9, 33, 33, ctypes.byref(lds)) == -11
    assert L.vjf_smooth_plan(256, 32, 24, ctypes.byref(lds)) == 0 and lds.value <= 159 * 1024
    assert call() == 0
    torch.cuda.synchronize()
    whole = full(vjf, name)
    same_bits(mean, whole.mean, "raw call: mean")
    same_bits(var, whole.var, "raw call: var")
    same_bits(cov0, whole.cov[0], "raw call: cov0")
    assert torch.equal(before.view(torch.int32), model._blob.view(torch.int32))
    after = model.get_state()
    assert after.keys() == state.keys() and all(np.array_equal(np.asarray(v), np.asarray(after[k])) for k, v in state.items())
    assert (model.transition.n_sample, model.likelihood.n_sample) == counters
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(gpu_rng, torch.cuda.get_rng_state())
    assert model.status() == 0
