"""`score_forecast` (vjf_kstep_score): the k-step-ahead prediction error over a filtered record in one native call.

  1. parity of every output against the fp64 reference (tests/kstep_cases.py: the cases, the records, the rule);
  2. exact, no tolerance: `pred` is `forecast_sequence` from every origin with zero weight noise, bit for bit; sse_x and base_x are
     the stated fold (fp32 in start order per tile, fp64 in tile order) recomputed in numpy from the returned pred and mu, bit for
     bit; row 0 of sse_x and the horizons beyond a short record are exactly 0;
  3. bitwise invariances: VJF_KS_CHUNK, VJF_FC_CENTROID_LDS, VJF_FC_LOOKAHEAD, a repeat, a side stream, return_pred;
  4. additivity over a split of the trials, a planted NaN, a poisoned output buffer, refusals without side effects.

A NaN planted in mu[t0, b0] reaches `pred` only through the roll-outs that START at or pass through that row of that trial, which is
the start (t0, b0) alone (a start's prediction depends on that start's inputs alone; targets enter the sums, not pred): exactly its
rows turn NaN, every other bit of pred stays.

All tests need a real MI355X:  pytest -m gpu."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import kstep_cases as kc
from tests import kstep_ref as kr
from tests.margins import check_close

pytestmark = pytest.mark.gpu
NAMES = list(kc.CASES)
K, F = kc.K, kc.F
SUMS = ("sse_x", "base_x", "sse_y", "base_y")


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_MODEL, _IN, _OUT = {}, {}, {}


def model_of(vjf, name):
    if name not in _MODEL:
        _MODEL[name] = kc.make_model(vjf, name)
    return _MODEL[name]


def dev(name):
    if name not in _IN:
        _IN[name] = {k: None if v is None else torch.as_tensor(v).cuda() for k, v in kc.record(name).items()}
    return _IN[name]


def run(vjf, name, rows=None, mu=None, return_pred=True, n_step=K):
    t = dev(name)
    mu = t["mu"] if mu is None else mu
    y, u = t["y"], t["u"]
    if rows is not None:
        mu, y, u = mu[:, rows].contiguous(), y[:, rows].contiguous(), None if u is None else u[:, rows].contiguous()
    return model_of(vjf, name).score_forecast(mu, y, u, n_step, return_pred=return_pred)


def full(vjf, name):
    """The call of the whole case with pred: once per module."""
    if name not in _OUT:
        _OUT[name] = run(vjf, name)
        torch.cuda.synchronize()
    return _OUT[name]


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same_bits(a, b, what=""):
    for f in SUMS + ("pred", "sst_x", "sst_y"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f"{what}: {f}"
        if x is not None:
            assert x.shape == y.shape and torch.equal(bits(x), bits(y)), f"{what}: {f} differs"


def by_rule(name, key, got, n):
    r64, r32 = kc.references(name)
    u = kc.unit(name, key, n)
    ref, b = r64[key] / u, kc.bound(r64[key] / u, r32[key] / u)
    g = got.detach().cpu().numpy().astype(np.float64) / u
    err = float(np.abs(g - ref).max())
    print(f"kstep margin: {name} {key}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    check_close(g, ref, rtol=0, atol=F * b, what=f"{name} {key} [ratio = used * {F}]")


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", NAMES)
def test_parity_against_the_fp64_reference(vjf, name):
    xdim, udim, n, ydim, B, T = kc.CASES[name]
    out = full(vjf, name)
    r64, _ = kc.references(name)
    assert type(out).__name__ == "ForecastScore" and out.kind == ("poisson" if kc.is_poisson(name) else "gaussian")
    assert out.n.tolist() == r64["n"].tolist() == [max(T - h, 0) * B for h in range(K + 1)]
    assert out.sse_x.shape == out.base_x.shape == out.sst_x.shape == (K + 1, xdim) and out.sse_x.dtype == torch.float64
    assert out.sse_y.shape == out.base_y.shape == (K + 1, ydim) and out.pred.shape == (K, T, B, xdim) and out.pred.dtype == torch.float32
    for key in SUMS:
        by_rule(name, key, getattr(out, key), r64["n"])
    # pred against the fp64 reference under the same rule (NaN exactly where the horizon is beyond the record)
    p64, p32 = kc.references(name)[0]["pred"], kc.references(name)[1]["pred"]
    got = out.pred.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(p64))
    ok = ~np.isnan(p64)
    if ok.any():
        b = kc.bound(p64[ok], p32[ok])
        err = float(np.abs(got[ok].astype(np.float64) - p64[ok]).max())
        print(f"kstep margin: {name} pred: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
        check_close(got[ok], p64[ok], rtol=0, atol=F * b, what=f"{name} pred [ratio = used * {F}]")
    # sst is the host's: numpy's variance of the valid target rows times their count
    mu = kc.record(name)["mu"].astype(np.float64)
    for h in range(K + 1):
        want = mu[h:].reshape(-1, xdim).var(0) * max(T - h, 0) * B if h < T else np.zeros(xdim)
        np.testing.assert_allclose(out.sst_x[h].cpu().numpy(), want, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", NAMES)
def test_pred_is_forecast_sequence_from_every_origin_bit_for_bit(vjf, name):
    xdim, udim, n, ydim, B, T = kc.CASES[name]
    out, t, m = full(vjf, name), dev(name), model_of(vjf, name)
    zeros = torch.zeros(K, n, xdim, device="cuda")
    for o in range(T):
        steps = min(K, T - 1 - o)
        assert torch.isnan(out.pred[steps:, o]).all(), f"origin {o}: NaN beyond the record"
        if steps == 0:
            continue
        u = None if t["u"] is None else t["u"][o + 1:o + 1 + steps].contiguous()
        x = m.transition.forecast_sequence(t["mu"][o], u, steps, w_noise=zeros[:steps])
        assert torch.equal(out.pred[:steps, o].contiguous().view(torch.int32), x[1:].contiguous().view(torch.int32)), f"origin {o}"


@pytest.mark.parametrize("name", NAMES)
def test_sums_are_the_stated_fold_of_pred_bit_for_bit(vjf, name):
    xdim, udim, n, ydim, B, T = kc.CASES[name]
    out = full(vjf, name)
    sse, base = kr.sums_from_pred(out.pred.cpu().numpy(), kc.record(name)["mu"], ordered=True)
    assert np.array_equal(out.sse_x.cpu().numpy().view(np.int64), sse.view(np.int64))
    assert np.array_equal(out.base_x.cpu().numpy().view(np.int64), base.view(np.int64))
    assert (out.sse_x[0] == 0).all(), "row 0 of sse_x is exactly 0"
    for h in range(T, K + 1):                               # (only `short` has such horizons)
        for key in SUMS:
            assert (getattr(out, key)[h] == 0).all(), f"{key}[{h}] beyond the record"
        assert out.n[h] == 0 and torch.isnan(out.pred[h - 1]).all()
    if name == "short":
        assert T == 5 and out.n.tolist()[5:] == [0, 0, 0, 0]


@contextlib.contextmanager
def own_stream():
    """A stream of the test's own, destroyed behind it (tests/test_gpu_fixed_point.py says why: a stream from torch's pool lives for
    the rest of the process and holds a share of the runtime's few hardware queues)."""
    with open("/proc/self/maps") as f:
        path = sorted({line.split()[-1] for line in f if "libamdhip64" in line})[0]
    hip, s = ctypes.CDLL(path), ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        yield torch.cuda.ExternalStream(s.value)
    finally:
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(s) == 0


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", ["control", "wide", "beyond256", "poisson"])
def test_bitwise_invariances(vjf, name, monkeypatch):
    ref = full(vjf, name)
    for env, val in (("VJF_KS_CHUNK", "1"), ("VJF_KS_CHUNK", "3"), ("VJF_FC_CENTROID_LDS", "0"), ("VJF_FC_LOOKAHEAD", "0")):
        monkeypatch.setenv(env, val)
        same_bits(run(vjf, name), ref, f"{env}={val}")
        monkeypatch.delenv(env)
    same_bits(run(vjf, name), ref, "a repeated call")
    torch.cuda.synchronize()
    with own_stream() as side:
        with torch.cuda.stream(side):
            other = run(vjf, name)
        side.synchronize()
    same_bits(other, ref, "a side stream")
    off = run(vjf, name, return_pred=False)
    assert off.pred is None
    for key in SUMS:
        assert torch.equal(bits(getattr(off, key)), bits(getattr(ref, key))), f"return_pred off: {key}"


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("name", ["ragged3", "control", "poisson"])
def test_additivity_over_a_split_of_the_trials(vjf, name):
    xdim, udim, n, ydim, B, T = kc.CASES[name]
    whole = full(vjf, name)
    cut = 21
    a, b = run(vjf, name, rows=slice(0, cut)), run(vjf, name, rows=slice(cut, B))
    assert (a.n + b.n).tolist() == whole.n.tolist()
    for key in SUMS:
        by_rule(name, key, getattr(a, key) + getattr(b, key), kc.references(name)[0]["n"])
    # a part's predictions are the whole's: a start's prediction depends on that start's inputs alone
    assert torch.equal(bits(a.pred), bits(whole.pred[:, :, :cut])) and torch.equal(bits(b.pred), bits(whole.pred[:, :, cut:]))


def test_a_planted_nan_stays_in_its_own_start(vjf):
    name = "control"
    xdim, udim, n, ydim, B, T = kc.CASES[name]
    whole = full(vjf, name)
    t0, b0 = 4, 17
    mu = dev(name)["mu"].clone()
    mu[t0, b0, 1] = float("nan")
    out = run(vjf, name, mu=mu)
    hit = torch.zeros(K, T, B, dtype=torch.bool, device="cuda")
    hit[:min(K, T - 1 - t0), t0, b0] = True
    was_nan = torch.isnan(whole.pred).all(-1)
    assert torch.equal(torch.isnan(out.pred).all(-1), hit | was_nan) and torch.equal(torch.isnan(out.pred).any(-1), hit | was_nan)
    keep = ~(hit | was_nan)
    assert torch.equal(out.pred[keep].view(torch.int32), whole.pred[keep].view(torch.int32))
    # the sums that a term with this row enters are NaN in that column at least; row 0 of sse_x has NaN - NaN in column 1 only
    assert torch.isnan(out.sse_x[0, 1]) and (out.sse_x[0, [0, 2, 3, 4]] == 0).all()
    assert torch.isnan(out.base_x[1:T - t0, 1]).all()           # (as a start: horizons 1 .. T - 1 - t0)


def test_a_poisoned_output_buffer_is_fully_overwritten_and_refusals_touch_nothing(vjf):
    name = "ragged3"
    xdim, udim, n, ydim, B, T = kc.CASES[name]
    ref, t, m = full(vjf, name), dev(name), model_of(vjf, name)
    vel, dec = m.transition.velocity, m.decoder.decode
    from vjf_amd import _native as N
    L = N.lib()
    size = ctypes.c_int64()
    assert L.vjf_kstep_score_scratch_size(T, B, K, xdim, ydim, ctypes.byref(size)) == 0
    scratch = torch.full((size.value,), 0xff, dtype=torch.uint8, device="cuda")
    nan64 = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")     # noqa: E731
    outs = [nan64(K + 1, xdim), nan64(K + 1, xdim), nan64(K + 1, ydim), nan64(K + 1, ydim)]
    pred = torch.full((K, T, B, xdim), 7.0, device="cuda")

    def call(mu=t["mu"], y=t["y"], dec_W=dec.weight, T_=T, K_=K, n_=n, d_=xdim):
        return L.vjf_kstep_score(N.ptr(mu), N.ptr(y), None, N.ptr(vel.feature.centroid), N.ptr(vel.feature.logwidth), N.ptr(vel.w_mean),
                                 N.ptr(dec_W), N.ptr(dec.bias), *(N.ptr(o) for o in outs), N.ptr(pred), N.ptr(scratch), T_, B, K_, n_, d_,
                                 xdim, ydim, 0, None)
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if isinstance(v, torch.Tensor)}
    for rc, kw in ((-1, dict(mu=None)), (-20, dict(T_=0)), (-20, dict(K_=0)), (-20, dict(dec_W=None)), (-21, dict(d_=xdim + 2)),
                   (-11, dict(n_=3000))):
        assert call(**kw) == rc, kw
        assert b"vjf_kstep_score" in L.vjf_last_error()
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs) and (pred == 7.0).all(), "a refusal writes nothing"
    assert (scratch == 0xff).all()
    assert call() == 0
    torch.cuda.synchronize()
    for o, key in zip(outs, SUMS):
        assert torch.equal(bits(o), bits(getattr(ref, key))), key
    assert torch.equal(bits(pred), bits(ref.pred))
    after = m.state_dict()
    assert all(torch.equal(v, after[k]) for k, v in before.items())
