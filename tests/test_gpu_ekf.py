"""`ekf` (vjf_ekf): the extended Kalman filter of the learned generative model and the model evidence in one native call.

  1. parity of mean, var, cov and loglik against the fp64 reference (tests/ekf_cases.py: the cases, the regimes, the rule), with and
     without the gap pattern;
  2. exact properties: symmetry, the diagonal, the head, return_cov = False, eigenvalues, positivity;
  3. rows that are not observed: loglik exactly 0, a NaN in their y changes no bit, a trial never observed follows forecast_sequence;
  4. bitwise invariances: the row index, the batch size, the tile-mates, the stream, VJF_FC_CENTROID_LDS, the decoder's placement,
     chunks chained with `before`;
  5. limits: a huge observation noise, T = 1, B = 1 and 17, a diagonal prior against the same prior as (mean, diag cov);
  6. poisoning: a NaN in an observed y and an indefinite `before` covariance;
  7. refusals through the real library and no side effects.

All tests need a real MI355X:  pytest -m gpu."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import ekf_cases as ec
from tests.margins import check_close

pytestmark = pytest.mark.gpu
NAMES = list(ec.CASES)
REGIMES = list(ec.REGIMES)
F = ec.F
EPS32 = ec.EPS32


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_MODEL, _IN, _OUT, _OBS = {}, {}, {}, {}


def model_of(vjf, name):
    if name not in _MODEL:
        _MODEL[name] = ec.make_model(vjf, name)
    return _MODEL[name]


def dev(name, regime="typical"):
    """{y, u, x0, lv0} of the case as device tensors, and the floats r, q: once per module."""
    if (name, regime) not in _IN:
        _IN[(name, regime)] = {k: (torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in ec.inputs(name, regime).items()}
    return _IN[(name, regime)]


def obs_of(name):
    if name not in _OBS:
        _OBS[name] = torch.as_tensor(ec.observed(name)).cuda()
    return _OBS[name]


def run(vjf, name, regime="typical", gaps=False, rows=None, lo=0, hi=None, y=None, **kw):
    """`ekf` on the trials `rows` and the time rows [lo, hi) of the case, from the case's prior unless `before` / `x0` is given."""
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
    kw = {"state_var": t["q"], "obs_var": t["r"], "return_cov": True, "observed": obs, **kw}
    return model_of(vjf, name).ekf(y.contiguous(), None if u is None else u.contiguous(), **kw)


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
    """a against b's trials `rows` and time rows [lo, hi), bit for bit: mean, var, cov, loglik, and a's head against its last row."""
    for k in ec.TENSORS:
        want = getattr(b, k)[lo:hi]
        same_bits(getattr(a, k), want if rows is None else want[:, rows], f"{what}: {k}")
    same_bits(a.head[0], a.mean[-1], f"{what}: head mean")
    same_bits(a.head[1], a.cov[-1], f"{what}: head cov")


def by_rule(what, tensor, got, ref64, other):
    """max|got - ref64| <= F max(E, 8 eps scale), E = max|other - ref64|; prints the achieved ratio before it asserts."""
    b = ec.bound(tensor, ref64, other)
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    err = float(np.abs(g - ref64).max())
    print(f"ekf margin: {what}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    check_close(g, np.asarray(ref64, np.float64), rtol=0, atol=F * b, what=f"{what} [ratio = used * {F}]")


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("gaps", [False, True], ids=["all", "gaps"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", NAMES)
def test_parity_against_the_fp64_reference(vjf, name, regime, gaps):
    xdim, udim, n, ydim, B, T = ec.CASES[name]
    out = full(vjf, name, regime, gaps)
    assert out.mean.shape == (T, B, xdim) and out.var.shape == (T, B, xdim) and out.cov.shape == (T, B, xdim, xdim)
    assert out.loglik.shape == (T, B) and out.head[1].shape == (B, xdim, xdim)
    ref = ec.references(name, regime, gaps)
    for what in ec.TENSORS:
        by_rule(f"{name} {regime} {'gaps' if gaps else 'all'} {what}", what, getattr(out, what), *ref[what])
    ev64 = ref["loglik"][0].sum(axis=0)
    np.testing.assert_allclose(host(out.log_likelihood()), ev64, rtol=0, atol=T * F * ec.bound("loglik", *ref["loglik"]))


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
    ev = np.linalg.eigvalsh(host(out.cov).astype(np.float64))
    worst = float((ev[..., 0] / ev[..., -1]).min())
    print(f"{name} {regime}: smallest eigenvalue over the largest, worst {worst:.3e}")
    assert (ev[..., 0] >= -8 * EPS32 * ev[..., -1]).all()
    no = run(vjf, name, regime, gaps, return_cov=False)
    assert no.cov is None
    same_bits(no.mean, out.mean, "mean without cov")
    same_bits(no.var, out.var, "var without cov")
    same_bits(no.loglik, out.loglik, "loglik without cov")
    same_bits(no.head[1], out.cov[-1], "head cov without cov")


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", NAMES)
def test_rows_that_are_not_observed(vjf, name):
    out = full(vjf, name, "typical", True)
    obs = obs_of(name).bool()
    assert bool((out.loglik[~obs] == 0).all()) and bool((out.loglik[obs] != 0).all())
    y = dev(name)["y"].clone()
    y[~obs] = float("nan")
    same_result(run(vjf, name, gaps=True, y=y), out, "NaN in the rows that are not observed")
    # the trial that is never observed: the mean is the mean map's roll-out from the prior mean
    xdim, udim, n, ydim, B, T = ec.CASES[name]
    t = dev(name)
    m = model_of(vjf, name)
    zw, zs = torch.zeros(T, n, xdim), torch.zeros(T, B, xdim)
    xf = m.forecast_sequence(t["x0"], t["u"], T, w_noise=zw, state_noise=zs)[0]
    b = ec.bound("mean", *ec.references(name, "typical", True)["mean"])
    err = float((out.mean[:, 1] - xf[1:, 1]).abs().max())
    print(f"ekf margin: {name} never observed: mean against forecast_sequence: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    assert err <= F * b


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
    whole = full(vjf, name, "sharp", True)
    B = ec.CASES[name][4]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).cuda()
    same_result(run(vjf, name, "sharp", True, rows=perm), whole, "permuted trials", perm)
    same_result(run(vjf, name, "sharp", True), whole, "a repeat")
    torch.cuda.synchronize()
    with own_stream() as side:
        with torch.cuda.stream(side):
            out = run(vjf, name, "sharp", True)
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
    """Four trials beside tile-mates whose records are others' (shifted by 3) or NaN."""
    whole = full(vjf, name)
    y = dev(name)["y"]
    keep = torch.tensor([1, 6, 17, y.shape[1] - 1]).cuda()
    for mates in (y + 3.0, torch.full_like(y, float("nan"))):
        mixed = mates.clone()
        mixed[:, keep] = y[:, keep]
        out = run(vjf, name, y=mixed)
        for k in ec.TENSORS:
            same_bits(getattr(out, k)[:, keep], getattr(whole, k)[:, keep], f"{k} beside other tile-mates")


@pytest.mark.parametrize("name", NAMES)
def test_bits_the_forms_of_the_kernel_agree(vjf, name, monkeypatch):
    """The forms for shapes beyond the LDS budget (centroids and w_mean, and the decoder, read from global memory), forced at the
    test shapes through the planner's overrides."""
    whole = full(vjf, name, "sharp", True)
    for env in ({"VJF_FC_CENTROID_LDS": "0"}, {"VJF_EKF_DECODER_LDS": "0"}, {"VJF_FC_CENTROID_LDS": "0", "VJF_EKF_DECODER_LDS": "0"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            same_result(run(vjf, name, "sharp", True), whole, str(env))


@pytest.mark.parametrize("name", ["control", "x24", "ragged3"])
def test_bits_chunked_with_before(vjf, name):
    whole = full(vjf, name, "typical", True)
    T = ec.CASES[name][5]
    for k in (T // 2, 1, T - 1):
        front = run(vjf, name, gaps=True, hi=k)
        back = run(vjf, name, gaps=True, lo=k, before=front.head)
        same_result(front, whole, f"rows [:{k}]", hi=k)
        same_result(back, whole, f"rows [{k}:] with before", lo=k)
        # the head of a call without the covariances, and `before` as (mean[k - 1], cov[k - 1]) of the undivided call
        back = run(vjf, name, gaps=True, lo=k, before=run(vjf, name, gaps=True, hi=k, return_cov=False).head)
        same_result(back, whole, f"rows [{k}:] before a head without cov", lo=k)
        same_result(run(vjf, name, gaps=True, lo=k, before=(whole.mean[k - 1], whole.cov[k - 1])), whole, f"rows [{k}:] before (mean, cov)", lo=k)
    # a row at a time
    head = None
    for t in range(min(T, 8)):
        r = run(vjf, name, gaps=True, lo=t, hi=t + 1, **({} if head is None else {"before": head}))
        same_result(r, whole, f"row {t} alone", lo=t, hi=t + 1)
        head = r.head
    # only the lower triangle of the `before` covariance is read
    junk = whole.cov[1] + torch.triu(torch.full_like(whole.cov[1], float("nan")), 1)
    same_result(run(vjf, name, gaps=True, lo=2, before=(whole.mean[1], junk)), whole, "junk above the diagonal", lo=2)


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("name", ["control", "wide", "scalar"])
def test_a_huge_observation_noise_returns_the_prediction(vjf, name):
    """vague with r = 1e12: the filter is the prediction, the mean within the rule of the run with nothing observed."""
    xdim, udim, n, ydim, B, T = ec.CASES[name]
    out = run(vjf, name, "vague", obs_var=1e12)
    pred = run(vjf, name, "vague", observed=torch.zeros(T, B, dtype=torch.bool))
    ref = ec.references(name, "vague")
    assert bool(torch.isfinite(out.loglik).all()) and bool((out.loglik < 0).all())
    b = F * ec.bound("mean", *ref["mean"])
    err = float((out.mean - pred.mean).abs().max())
    print(f"ekf margin: {name} obs_var = 1e12 mean against the prediction: err {err:.3e} bound {b / F:.3e} ratio {err * F / b:.3f} (F = {F})")
    assert err <= b
    errv = float((out.cov - pred.cov).abs().max())
    bv = F * 8 * EPS32 * float(pred.cov.abs().max())
    print(f"ekf margin: {name} obs_var = 1e12 cov against the prediction: err {errv:.3e} bound {bv / F:.3e} ratio {errv * F / bv:.3f} (F = {F})")
    assert errv <= bv


@pytest.mark.parametrize("name", ["control", "x24"])
def test_one_row(vjf, name):
    whole = full(vjf, name)
    one = run(vjf, name, hi=1)
    assert one.mean.shape[0] == 1 and one.loglik.shape[0] == 1
    same_result(one, whole, "T = 1", hi=1)


@pytest.mark.parametrize("B", [1, 17])
def test_one_trial_and_seventeen(vjf, B):
    name = "control"
    whole = full(vjf, name)
    rows = torch.arange(B).cuda()
    same_result(run(vjf, name, rows=rows), whole, f"B = {B}", rows)
    if B == 1:                                     # given without its batch axis
        t = dev(name)
        one = model_of(vjf, name).ekf(t["y"][:, 0], t["u"][:, 0], x0=vjf.Gaussian(t["x0"][:1], t["lv0"][:1]), state_var=t["q"],
                                      obs_var=t["r"], return_cov=True)
        same_result(one, whole, "(T, ydim)", rows)


@pytest.mark.parametrize("name", ["control", "x24"])
def test_a_diagonal_prior_against_the_same_prior_as_a_covariance(vjf, name):
    """exp(logvar) is formed on the device in one case and by torch in the other: the two agree within the rule of the case."""
    t = dev(name)
    whole = full(vjf, name)
    out = run(vjf, name, before=(t["x0"], torch.diag_embed(t["lv0"].exp())))
    ref = ec.references(name)
    for k in ec.TENSORS:
        b = F * ec.bound(k, *ref[k])
        err = float((getattr(out, k) - getattr(whole, k)).abs().max())
        print(f"ekf margin: {name} diagonal prior as a covariance {k}: err {err:.3e} bound {b / F:.3e} ratio {err * F / b:.3f} (F = {F})")
        assert err <= b


# ------------------------------------------------------------------ 6
def test_poisoning_by_a_nan_in_an_observed_row(vjf):
    """Runs to completion: the NaN is data, not a fault."""
    name = "control"
    whole = full(vjf, name)
    B, T = ec.CASES[name][4], ec.CASES[name][5]
    bad, t0 = 5, T // 2
    others = torch.tensor([r for r in range(B) if r != bad]).cuda()
    for field, value in (("y", float("nan")), ("y", float("inf")), ("u", float("nan"))):
        t = dev(name)
        y, u = t["y"].clone(), t["u"].clone()
        (y if field == "y" else u)[t0, bad, 1] = value
        out = model_of(vjf, name).ekf(y, u, x0=vjf.Gaussian(t["x0"], t["lv0"]), state_var=t["q"], obs_var=t["r"], return_cov=True)
        torch.cuda.synchronize()
        for k in ec.TENSORS:
            got, want = getattr(out, k), getattr(whole, k)
            same_bits(got[:, others], want[:, others], f"{value} in {field}: {k} of the other trials")
            same_bits(got[:t0, bad], want[:t0, bad], f"{value} in {field}: {k} before the row")
            assert bool(torch.isnan(got[t0:, bad]).all()), f"{value} in {field}: {k} from the row on"
        assert bool(torch.isnan(out.head[1][bad]).all())


def test_poisoning_by_an_indefinite_before_covariance(vjf):
    name = "control"
    whole = full(vjf, name)
    k, bad = 7, 5
    others = torch.tensor([r for r in range(ec.CASES[name][4]) if r != bad]).cuda()
    cov = whole.cov[k - 1].clone()
    cov[bad] = -cov[bad]
    out = run(vjf, name, lo=k, before=(whole.mean[k - 1], cov))
    for f in ec.TENSORS:
        same_bits(getattr(out, f)[:, others], getattr(whole, f)[k:, others], f"indefinite before: {f} of the other trials")
        assert bool(torch.isnan(getattr(out, f)[:, bad]).all())
    mean = whole.mean[k - 1].clone()
    mean[bad, 0] = float("nan")
    out = run(vjf, name, lo=k, before=(mean, whole.cov[k - 1]))
    same_bits(out.mean[:, others], whole.mean[k:, others], "NaN in the before mean: the other trials")
    assert bool(torch.isnan(out.mean[:, bad]).all()) and bool(torch.isnan(out.loglik[:, bad]).all())


# ------------------------------------------------------------------ 7
def test_refusals_and_no_side_effects(vjf):
    from vjf_amd import _native as N
    L = N.lib()
    name = "control"
    model = model_of(vjf, name)
    xdim, udim, n, ydim, B, T = ec.CASES[name]
    t = dev(name)
    model._ensure_ctx(B)
    state = model.get_state()
    before = model._blob.clone()
    counters = (model.transition.n_sample, model.likelihood.n_sample)
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    x0 = vjf.Gaussian(t["x0"], t["lv0"])
    with pytest.raises(TypeError):
        model.ekf(t["y"], x0=x0)
    with pytest.raises(AssertionError):
        model.ekf(t["y"], t["u"][:-1], x0=x0)
    with pytest.raises(ValueError):
        model.ekf(t["y"], t["u"], x0=x0, before=(t["x0"], torch.diag_embed(t["lv0"].exp())))
    for kw in ("state_var", "obs_var"):
        for v in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError):
                model.ekf(t["y"], t["u"], x0=x0, **{kw: v})
    vel, dec = model.transition.velocity, model.decoder.decode
    new = lambda *s: torch.full(s, 7.0, device="cuda", dtype=torch.float32)      # noqa: E731
    mean, var, ll, last = new(T, B, xdim), new(T, B, xdim), new(T, B), new(B, xdim, xdim)
    p = N.ptr

    def call(y=t["y"], u=t["u"], plv=t["lv0"], pc=None, T=T, B=B, n=n, d=xdim + udim, dout=xdim, dy=ydim, sv=t["q"], ov=t["r"]):
        return L.vjf_ekf(p(y), p(u), None, p(vel.feature.centroid), p(vel.feature.logwidth), p(vel.w_mean), p(dec.weight), p(dec.bias),
                         p(t["x0"]), p(plv), p(pc), p(mean), p(var), None, p(ll), p(last), T, B, n, d, dout, dy, sv, ov, None)
    for rc, kw in ((-1, dict(y=None)), (-20, dict(T=0)), (-20, dict(sv=0.0)), (-20, dict(ov=float("nan"))), (-20, dict(B=0)), (-20, dict(dy=0)),
                   (-20, dict(pc=last)), (-20, dict(plv=None)), (-21, dict(u=None)), (-11, dict(n=9, d=33, dout=33, u=None)),
                   (-11, dict(n=9, d=32, dout=32, u=None)), (-11, dict(n=1000, d=64, dout=64, u=None)), (-11, dict(n=3000, d=3, dout=3, u=None))):
        assert call(**kw) == rc, kw                      # (every refusal comes before the first launch: nothing is read or written)
        assert b"vjf_ekf" in L.vjf_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in (mean, var, ll, last))
    lds = ctypes.c_int64()
    assert L.vjf_ekf_plan(9, 33, 33, ydim, ctypes.byref(lds)) == -11
    assert L.vjf_ekf_plan(256, 24, 16, 1 << 20, ctypes.byref(lds)) == 0 and lds.value <= 159 * 1024
    assert call() == 0
    torch.cuda.synchronize()
    whole = full(vjf, name)
    same_bits(mean, whole.mean, "raw call: mean")
    same_bits(var, whole.var, "raw call: var")
    same_bits(ll, whole.loglik, "raw call: loglik")
    same_bits(last, whole.cov[-1], "raw call: cov_last")
    assert torch.equal(before.view(torch.int32), model._blob.view(torch.int32))
    after = model.get_state()
    assert after.keys() == state.keys() and all(np.array_equal(np.asarray(v), np.asarray(after[k])) for k, v in state.items())
    assert (model.transition.n_sample, model.likelihood.n_sample) == counters
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(gpu_rng, torch.cuda.get_rng_state())
    assert model.status() == 0
