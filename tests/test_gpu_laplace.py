"""`laplace_filter` (vjf_laplace_filter): the filter of the learned generative model with count observations and the Laplace evidence in
one native call.

  1. parity of mean, var, cov, loglik and grad_norm against the fp64 reference (tests/laplace_cases.py: the cases, the regimes, the
     rule), with and without the gap pattern;
  2. exact properties: symmetry, the diagonal, the head, return_cov = False;
  3. rows that are not observed: loglik and grad_norm exactly 0, a NaN in their y changes no bit; with every row unobserved mean, var
     and cov are bitwise those of `ekf` on a Gaussian twin of the model;
  4. C = 0: loglik is the Poisson log-pmf at exp(b), summed, P = P^- and m = m^-;
  5. bitwise invariances: the row index and a repeat, the stream, the batch size, the tile-mates, every form of the kernel, chunks
     chained with `before`;
  6. n_iter = 1 and n_iter = 64, one row, ydim in {1, 16, 17, 65};
  7. poisoning;
  8. refusals through the real library and no side effects.

All tests need a real MI355X:  pytest -m gpu."""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import ekf_cases as ec
from tests import laplace_cases as lc
from tests import laplace_ref as lr
from tests.margins import check_close

pytestmark = pytest.mark.gpu
NAMES = list(lc.CASES)
REGIMES = list(lc.REGIMES)
F = lc.F
EPS32 = lc.EPS32


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_MODEL, _IN, _OUT, _OBS = {}, {}, {}, {}


def model_of(vjf, name, regime="typical"):
    if (name, regime) not in _MODEL:
        _MODEL[(name, regime)] = lc.make_model(vjf, name, regime)
    return _MODEL[(name, regime)]


def dev(name, regime="typical"):
    """{y, u, x0, lv0} of the case as device tensors, and the float q: once per module."""
    if (name, regime) not in _IN:
        _IN[(name, regime)] = {k: (torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in lc.inputs(name, regime).items()}
    return _IN[(name, regime)]


def obs_of(name):
    if name not in _OBS:
        _OBS[name] = torch.as_tensor(lc.observed(name)).cuda()
    return _OBS[name]


def run(vjf, name, regime="typical", gaps=False, rows=None, lo=0, hi=None, y=None, model=None, **kw):
    """`laplace_filter` on the trials `rows` and the time rows [lo, hi) of the case, from the case's prior unless `before` / `x0` is
    given."""
    t = dev(name, regime)
    y = t["y"] if y is None else y
    u, obs = t["u"], obs_of(name) if gaps else None
    hi = y.shape[0] if hi is None else hi
    y, u, obs = y[lo:hi], None if u is None else u[lo:hi], None if obs is None else obs[lo:hi]
    x0, lv0 = t["x0"], t["lv0"]
    if rows is not None:
        y, u, obs = y[:, rows], None if u is None else u[:, rows], None if obs is None else obs[:, rows]
        x0, lv0 = x0[rows], lv0[rows]
    if "before" not in kw and "x0" not in kw:
        kw["x0"] = vjf.Gaussian(x0.contiguous(), lv0.contiguous())
    kw = {"state_var": t["q"], "return_cov": True, "observed": obs, **kw}
    m = model_of(vjf, name, regime) if model is None else model
    return m.laplace_filter(y.contiguous(), None if u is None else u.contiguous(), **kw)


def full(vjf, name, regime="typical", gaps=False):
    """The undivided call of the case with the covariances: once per module."""
    key = (name, regime, bool(gaps))
    if key not in _OUT:
        _OUT[key] = run(vjf, name, regime, gaps)
        torch.cuda.synchronize()
    return _OUT[key]


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def same_bits(a, b, what=""):
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} against {tuple(b.shape)}"
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f"{what}: differs"


def same_result(a, b, what, rows=None, lo=0, hi=None):
    """a against b's trials `rows` and time rows [lo, hi), bit for bit: every tensor, and a's head against its last row."""
    for k in lc.TENSORS:
        want = getattr(b, k)[lo:hi]
        same_bits(getattr(a, k), want if rows is None else want[:, rows], f"{what}: {k}")
    same_bits(a.head[0], a.mean[-1], f"{what}: head mean")
    same_bits(a.head[1], a.cov[-1], f"{what}: head cov")


def by_rule(what, tensor, got, ref64, other, name, regime):
    """max|got - ref64| <= F max(E, 8 eps scale), E = max|other - ref64|; prints the achieved ratio before it asserts."""
    b = lc.bound(tensor, ref64, other, name, regime)
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    err = float(np.abs(g - ref64).max())
    print(f"laplace margin: {what}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    check_close(g, np.asarray(ref64, np.float64), rtol=0, atol=F * b, what=f"{what} [ratio = used * {F}]")


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("gaps", [False, True], ids=["all", "gaps"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", NAMES)
def test_parity_against_the_fp64_reference(vjf, name, regime, gaps):
    xdim, udim, n, ydim, B, T = lc.CASES[name]
    out = full(vjf, name, regime, gaps)
    assert out.mean.shape == (T, B, xdim) and out.var.shape == (T, B, xdim) and out.cov.shape == (T, B, xdim, xdim)
    assert out.loglik.shape == (T, B) and out.grad_norm.shape == (T, B) and out.head[1].shape == (B, xdim, xdim)
    ref = lc.references(name, regime, gaps)
    for what in lc.TENSORS:
        by_rule(f"{name} {regime} {'gaps' if gaps else 'all'} {what}", what, getattr(out, what), *ref[what], name, regime)
    ev64 = ref["loglik"][0].sum(axis=0)
    np.testing.assert_allclose(host(out.log_likelihood()), ev64, rtol=0, atol=T * F * lc.bound("loglik", *ref["loglik"]))


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("gaps", [False, True], ids=["all", "gaps"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", NAMES)
def test_exact_properties(vjf, name, regime, gaps):
    out = full(vjf, name, regime, gaps)
    same_bits(out.cov, out.cov.transpose(-1, -2), "cov against its transpose")
    same_bits(torch.diagonal(out.cov, dim1=-2, dim2=-1), out.var, "the diagonal of cov against var")
    same_bits(out.head[0], out.mean[-1], "head mean")
    same_bits(out.head[1], out.cov[-1], "head cov")
    assert bool((out.var > 0).all()) and bool(torch.isfinite(out.cov).all()) and bool(torch.isfinite(out.loglik).all())
    assert bool((out.grad_norm >= 0).all())
    no = run(vjf, name, regime, gaps, return_cov=False)
    assert no.cov is None
    for k in ("mean", "var", "loglik", "grad_norm"):
        same_bits(getattr(no, k), getattr(out, k), f"{k} without cov")
    same_bits(no.head[1], out.cov[-1], "head cov without cov")


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", NAMES)
def test_rows_that_are_not_observed(vjf, name):
    out = full(vjf, name, "typical", True)
    obs = obs_of(name).bool()
    assert bool((out.loglik[~obs] == 0).all()) and bool((out.loglik[obs] != 0).all()) and bool((out.grad_norm[~obs] == 0).all())
    y = dev(name)["y"].clone()
    y[~obs] = float("nan")
    same_result(run(vjf, name, gaps=True, y=y), out, "NaN in the rows that are not observed")


@pytest.mark.parametrize("name", NAMES)
def test_nothing_observed_is_the_ekf_of_a_gaussian_twin(vjf, name):
    """With every row unobserved both filters are the prediction: mean, var and cov agree bit for bit."""
    xdim, udim, n, ydim, B, T = lc.CASES[name]
    t = dev(name)
    none = torch.zeros(T, B, dtype=torch.bool)
    out = run(vjf, name, observed=none)
    twin = ec.make_model(vjf, name)
    x0 = vjf.Gaussian(t["x0"], t["lv0"])
    ref = twin.ekf(torch.zeros_like(t["y"]), t["u"], x0=x0, state_var=t["q"], obs_var=1.0, observed=none, return_cov=True)
    for k in ("mean", "var", "cov"):
        same_bits(getattr(out, k), getattr(ref, k), f"nothing observed: {k} against ekf")
    assert bool((out.loglik == 0).all()) and bool((out.grad_norm == 0).all())


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("name", ["control", "wide"])
def test_a_zero_decoder(vjf, name):
    """C = 0: the counts say nothing of x.  loglik is the Poisson log-pmf at exp(b), summed; P = P^- and m = m^-, the rows of a run
    with nothing observed."""
    xdim, udim, n, ydim, B, T = lc.CASES[name]
    t = dev(name)
    m = lc.make_model(vjf, name, "typical")
    m.decoder.decode.weight.zero_()
    b = m.decoder.decode.bias.detach().cpu().numpy().astype(np.float64)
    out = run(vjf, name, model=m)
    pred = run(vjf, name, model=m, observed=torch.zeros(T, B, dtype=torch.bool))
    for k in ("mean", "var", "cov"):
        same_bits(getattr(out, k), getattr(pred, k), f"C = 0: {k} against the prediction")
    y = lc.inputs(name)["y"].astype(np.float64)
    lg = np.vectorize(math.lgamma)(y + 1.0)
    pmf = (y * b - np.exp(b) - lg).sum(axis=2)
    err = float(np.abs(host(out.loglik) - pmf).max())
    bound = 8 * EPS32 * float((np.abs(y * b) + np.exp(b) + lg).sum(axis=2).max())       # the terms that are added up
    print(f"laplace margin: {name} C = 0 loglik against the log-pmf: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f} (F = {F})")
    assert err <= F * bound


# ------------------------------------------------------------------ 5
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
    whole = full(vjf, name, "busy", True)
    B = lc.CASES[name][4]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).cuda()
    same_result(run(vjf, name, "busy", True, rows=perm), whole, "permuted trials", perm)
    same_result(run(vjf, name, "busy", True), whole, "a repeat")
    torch.cuda.synchronize()
    with own_stream() as side:
        with torch.cuda.stream(side):
            out = run(vjf, name, "busy", True)
        side.synchronize()
    same_result(out, whole, "side stream")


@pytest.mark.parametrize("B", [1, 15, 16, 17, 37])
def test_bits_batch_size(vjf, B):
    """The first B trials of ragged3 (37 trials) and B trials from its middle: a trial's rows do not depend on the batch."""
    whole = full(vjf, "ragged3", "typical", True)
    for lo in (0, 37 - B):
        rows = torch.arange(lo, lo + B).cuda()
        same_result(run(vjf, "ragged3", gaps=True, rows=rows), whole, f"trials [{lo}:{lo + B}]", rows)


@pytest.mark.parametrize("name", ["ragged3", "control"])
def test_bits_do_not_depend_on_the_tile_mates(vjf, name):
    """Four trials beside tile-mates whose records are others' (shifted by 3), negative or NaN."""
    whole = full(vjf, name)
    y = dev(name)["y"]
    keep = torch.tensor([1, 6, 17, y.shape[1] - 1]).cuda()
    for mates in (y + 3.0, torch.full_like(y, -1.0), torch.full_like(y, float("nan"))):
        mixed = mates.clone()
        mixed[:, keep] = y[:, keep]
        out = run(vjf, name, y=mixed)
        for k in lc.TENSORS:
            same_bits(getattr(out, k)[:, keep], getattr(whole, k)[:, keep], f"{k} beside other tile-mates")


@pytest.mark.parametrize("name", NAMES)
def test_bits_the_forms_of_the_kernel_agree(vjf, name, monkeypatch):
    """The forms for shapes beyond the LDS budget (centroids and w_mean, and the decoder, read from global memory), forced at the
    test shapes through the planner's overrides."""
    whole = full(vjf, name, "busy", True)
    for env in ({"VJF_FC_CENTROID_LDS": "0"}, {"VJF_LAPLACE_DECODER_LDS": "0"}, {"VJF_FC_CENTROID_LDS": "0", "VJF_LAPLACE_DECODER_LDS": "0"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            same_result(run(vjf, name, "busy", True), whole, str(env))


@pytest.mark.parametrize("name", ["control", "x24", "ragged3"])
def test_bits_chunked_with_before(vjf, name):
    whole = full(vjf, name, "typical", True)
    T = lc.CASES[name][5]
    for k in (T // 2, 1, T - 1):
        front = run(vjf, name, gaps=True, hi=k)
        back = run(vjf, name, gaps=True, lo=k, before=front.head)
        same_result(front, whole, f"rows [:{k}]", hi=k)
        same_result(back, whole, f"rows [{k}:] with before", lo=k)
        back = run(vjf, name, gaps=True, lo=k, before=run(vjf, name, gaps=True, hi=k, return_cov=False).head)
        same_result(back, whole, f"rows [{k}:] before a head without cov", lo=k)
    head = None
    for t in range(min(T, 4)):                      # a row at a time
        r = run(vjf, name, gaps=True, lo=t, hi=t + 1, **({} if head is None else {"before": head}))
        same_result(r, whole, f"row {t} alone", lo=t, hi=t + 1)
        head = r.head
    junk = whole.cov[1] + torch.triu(torch.full_like(whole.cov[1], float("nan")), 1)
    same_result(run(vjf, name, gaps=True, lo=2, before=(whole.mean[1], junk)), whole, "junk above the diagonal", lo=2)


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("n_iter", [1, 64])
def test_one_and_sixty_four_iterations(vjf, n_iter):
    """n_iter = 1 against the reference at n_iter = 1 (the step control's first decision); n_iter = 64 against the converged
    reference: the iterations behind convergence change nothing beyond the rule."""
    name, regime = "control", "busy"
    out = run(vjf, name, regime, n_iter=n_iter)
    r64 = lc.run_reference(name, regime, False, np.float64, n_iter=n_iter)
    r32 = lc.run_reference(name, regime, False, np.float32, n_iter=n_iter)
    for i, what in enumerate(lc.TENSORS):
        by_rule(f"{name} {regime} n_iter = {n_iter} {what}", what, getattr(out, what), r64[i], r32[i], name, regime)


@pytest.mark.parametrize("name", ["control", "x24"])
def test_one_row(vjf, name):
    whole = full(vjf, name)
    one = run(vjf, name, hi=1)
    assert one.mean.shape[0] == 1 and one.loglik.shape[0] == 1
    same_result(one, whole, "T = 1", hi=1)


@pytest.mark.parametrize("ydim", [1, 16, 17, 65])
def test_the_number_of_outputs(vjf, ydim):
    """One y row, a full tile, a tile and a row, and a second round of tiles: a model of its own against the reference."""
    xdim, udim, n, B, T = 5, 1, 23, 19, 5
    torch.manual_seed(11)
    m = vjf.VJF.make_model(ydim, xdim, udim, n, [4], likelihood="poisson")
    g = torch.Generator().manual_seed(100 + ydim)
    m.transition.velocity.w_mean.copy_((0.5 * torch.randn(n, xdim, generator=g)).cuda())
    m.decoder.decode.weight.copy_((0.4 * torch.randn(ydim, xdim, generator=g)).cuda())
    m.decoder.decode.bias.copy_((0.5 + 0.3 * torch.randn(ydim, generator=g)).cuda())
    x0 = torch.randn(B, xdim, generator=g)
    lv0 = torch.full((B, xdim), math.log(0.05))
    u = torch.randn(T, B, udim, generator=g)
    y = torch.poisson(torch.full((T, B, ydim), 2.0), generator=g)
    obs = torch.ones(T, B, dtype=torch.uint8)
    obs[1, ::3] = 0
    out = m.laplace_filter(y.cuda(), u.cuda(), x0=vjf.Gaussian(x0.cuda(), lv0.cuda()), state_var=0.01, observed=obs, return_cov=True)
    refs = []
    for dt in (np.float64, np.float32):
        s, C, b = lc.state_of(m)
        c = lambda v: v.numpy().astype(dt)          # noqa: E731
        refs.append(lr.laplace_filter(s.cast(dt) if dt == np.float32 else s, C.astype(dt), b.astype(dt), c(y), c(u), 0.01, c(x0),
                                      prior_logvar=c(lv0), observed=obs.numpy()))
    for i, what in enumerate(lc.TENSORS):
        ref64, ref32 = refs[0][i], refs[1][i]
        scale = max(1.0, float(np.abs(y.numpy().astype(np.float64) @ C).max())) if what == "grad_norm" else \
            (max(1.0, float(np.abs(ref64).max())) if what == "mean" else float(np.abs(ref64).max()))
        E = float(np.abs(ref32.astype(np.float64) - ref64).max())
        assert E <= 1e-3 * scale
        bound = max(E, 8 * EPS32 * scale)
        err = float(np.abs(host(getattr(out, what)).astype(np.float64) - ref64).max())
        print(f"laplace margin: ydim = {ydim} {what}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f} (F = {F})")
        assert err <= F * bound, what


# ------------------------------------------------------------------ 7
def test_poisoning(vjf):
    """Runs to completion: the values are data, not a fault.  A NaN, an infinity or a negative count in an observed y, a NaN in u:
    the trial is NaN from that row on, its rows before and every other trial keep their bits."""
    name = "control"
    whole = full(vjf, name)
    B, T = lc.CASES[name][4], lc.CASES[name][5]
    bad, t0 = 5, T // 2
    others = torch.tensor([r for r in range(B) if r != bad]).cuda()
    for field, value in (("y", float("nan")), ("y", float("inf")), ("y", -1.0), ("u", float("nan"))):
        t = dev(name)
        y, u = t["y"].clone(), t["u"].clone()
        (y if field == "y" else u)[t0, bad, 1] = value
        out = model_of(vjf, name).laplace_filter(y, u, x0=vjf.Gaussian(t["x0"], t["lv0"]), state_var=t["q"], return_cov=True)
        torch.cuda.synchronize()
        for k in lc.TENSORS:
            got, want = getattr(out, k), getattr(whole, k)
            same_bits(got[:, others], want[:, others], f"{value} in {field}: {k} of the other trials")
            same_bits(got[:t0, bad], want[:t0, bad], f"{value} in {field}: {k} before the row")
            assert bool(torch.isnan(got[t0:, bad]).all()), f"{value} in {field}: {k} from the row on"
        assert bool(torch.isnan(out.head[1][bad]).all())


def test_poisoning_by_the_prior_and_by_an_overflowing_rate(vjf):
    name = "control"
    whole = full(vjf, name)
    k, bad = 7, 5
    others = torch.tensor([r for r in range(lc.CASES[name][4]) if r != bad]).cuda()
    cov = whole.cov[k - 1].clone()
    cov[bad] = -cov[bad]
    out = run(vjf, name, lo=k, before=(whole.mean[k - 1], cov))
    for f in lc.TENSORS:
        same_bits(getattr(out, f)[:, others], getattr(whole, f)[k:, others], f"indefinite before: {f} of the other trials")
        assert bool(torch.isnan(getattr(out, f)[:, bad]).all())
    # a prior mean so far out that exp(eta) overflows at z = 0: phi is not finite there
    mean = whole.mean[k - 1].clone()
    mean[bad] = 1e6
    out = run(vjf, name, lo=k, before=(mean, whole.cov[k - 1]))
    same_bits(out.mean[:, others], whole.mean[k:, others], "an overflowing rate: the other trials")
    assert bool(torch.isnan(out.mean[:, bad]).all()) and bool(torch.isnan(out.loglik[:, bad]).all())


# ------------------------------------------------------------------ 8
def test_refusals_and_no_side_effects(vjf):
    from vjf_amd import _native as N
    L = N.lib()
    name = "control"
    model = model_of(vjf, name)
    xdim, udim, n, ydim, B, T = lc.CASES[name]
    t = dev(name)
    model._ensure_ctx(B)
    twin = ec.make_model(vjf, name)                  # (seeds torch's generator: before its state is recorded)
    state = model.get_state()
    before = model._blob.clone()
    counters = model.transition.n_sample
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    x0 = vjf.Gaussian(t["x0"], t["lv0"])
    with pytest.raises(TypeError):
        model.laplace_filter(t["y"], x0=x0)
    with pytest.raises(AssertionError):
        model.laplace_filter(t["y"], t["u"][:-1], x0=x0)
    with pytest.raises(ValueError):
        model.laplace_filter(t["y"], t["u"], x0=x0, before=(t["x0"], torch.diag_embed(t["lv0"].exp())))
    for kw in (dict(state_var=0.0), dict(state_var=float("nan")), dict(n_iter=0), dict(n_iter=65)):
        with pytest.raises(ValueError):
            model.laplace_filter(t["y"], t["u"], x0=x0, **kw)
    with pytest.raises(NotImplementedError, match="ekf"):
        twin.laplace_filter(t["y"], t["u"], x0=x0)
    with pytest.raises(NotImplementedError, match="Poisson"):
        model.ekf(t["y"], t["u"], x0=x0)
    vel, dec = model.transition.velocity, model.decoder.decode
    new = lambda *s: torch.full(s, 7.0, device="cuda", dtype=torch.float32)      # noqa: E731
    mean, var, ll, gn, last = new(T, B, xdim), new(T, B, xdim), new(T, B), new(T, B), new(B, xdim, xdim)
    p = N.ptr

    def call(y=t["y"], u=t["u"], plv=t["lv0"], pc=None, T=T, B=B, n=n, d=xdim + udim, dout=xdim, dy=ydim, it=lc.N_ITER, sv=t["q"]):
        return L.vjf_laplace_filter(p(y), p(u), None, p(vel.feature.centroid), p(vel.feature.logwidth), p(vel.w_mean), p(dec.weight),
                                    p(dec.bias), p(t["x0"]), p(plv), p(pc), p(mean), p(var), None, p(ll), p(gn), p(last), T, B, n, d,
                                    dout, dy, it, sv, None)
    for rc, kw in ((-1, dict(y=None)), (-20, dict(T=0)), (-20, dict(sv=0.0)), (-20, dict(B=0)), (-20, dict(dy=0)), (-20, dict(it=0)),
                   (-20, dict(it=65)), (-20, dict(pc=last)), (-20, dict(plv=None)), (-21, dict(u=None)),
                   (-11, dict(n=9, d=25, dout=25, u=None)), (-11, dict(n=3000, d=3, dout=3, u=None))):
        assert call(**kw) == rc, kw                      # (every refusal comes before the first launch: nothing is read or written)
        assert b"vjf_laplace_filter" in L.vjf_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in (mean, var, ll, gn, last))
    assert call() == 0
    torch.cuda.synchronize()
    whole = full(vjf, name)
    same_bits(mean, whole.mean, "raw call: mean")
    same_bits(var, whole.var, "raw call: var")
    same_bits(ll, whole.loglik, "raw call: loglik")
    same_bits(gn, whole.grad_norm, "raw call: grad_norm")
    same_bits(last, whole.cov[-1], "raw call: cov_last")
    assert torch.equal(before.view(torch.int32), model._blob.view(torch.int32))
    after = model.get_state()
    assert after.keys() == state.keys() and all(np.array_equal(np.asarray(v), np.asarray(after[k])) for k, v in state.items())
    assert model.transition.n_sample == counters
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(gpu_rng, torch.cuda.get_rng_state())
    assert model.status() == 0
