"""`forecast_ensemble` (vjf_forecast_ens): S sampled roll-outs of a whole horizon and their per-step mean and variance in one native
call.

  1. parity of the four moment tensors against the fp64 oracle (tests/ensemble_cases.py: the shapes, the draws and the rule);
  2. the members are `forecast_sequence`, bit for bit; one member is the roll-out itself with variances of exactly 0;
  3. a seeded drop-in for S successive `forecast_sequence` calls: same draws, same order, the generator left in the same state;
  4. bitwise invariances of all four moment tensors: permuted trials, sub-batches, both chunkings, a side stream, the forms of the
     kernels, a split horizon, a member prefix;
  5. the scratch bound, and a long horizon with many members on it;
  6. no side effects on the model;
  7. edges and refusals.

All tests need a real MI355X:  pytest -m gpu."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ensemble_cases as ec
from tests import forecast_cases as fc
from tests.margins import check_close

pytestmark = pytest.mark.gpu

MOMENTS = ec.TENSORS


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_CACHE = {}


def case(vjf, name):
    """(model, inputs and draws as device tensors): built once per module."""
    if name not in _CACHE:
        m = fc.make_model(vjf, name)
        a = dict(fc.inputs(name))
        del a["w_noise"], a["state_noise"]
        a.update(ec.noises(name))
        _CACHE[name] = (m, {k: None if v is None else torch.as_tensor(v).cuda() for k, v in a.items()})
    return _CACHE[name]


def same_bits(a, b, what=""):
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} against {tuple(b.shape)}"
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), \
        f"{what}: differs by {float((a.double() - b.double()).abs().max()):.3e}"


def same_moments(a, b, what, rows=slice(None), steps=slice(None)):
    for k in MOMENTS:
        same_bits(getattr(a, k), getattr(b, k)[steps][:, rows], f"{what}: {k}")


def by_rule(what, got, ref64, other, F=ec.F):
    """max|got - ref64| <= F max(E, 8 eps max|ref64|), E = max|other - ref64|; prints the achieved ratio before it asserts."""
    b = fc.bound(ref64, other)
    g = got.detach().cpu().numpy().astype(np.float64)
    err = float(np.abs(g - ref64).max())
    print(f"ensemble margin: {what}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    check_close(g, np.asarray(ref64, np.float64), rtol=0, atol=F * b, what=f"{what} [ratio = used * {F}]")   # (asserts, and records)


def ens(m, t, S=ec.S_MAX, mode="noisy", T=None, t0=0, rows=None, x0=None, members=False):
    """forecast_ensemble on the case's inputs: the first S members, steps t0 .. t0 + T - 1, trials `rows` (an index tensor), every
    draw given.  mode: ec.MODES; x0 overrides the start (a plain tensor)."""
    T = t["w_noise"].shape[1] - t0 if T is None else T
    pick = (lambda a, ax: a) if rows is None else (lambda a, ax: a.index_select(ax, rows).contiguous())
    u = None if t["u"] is None else pick(t["u"][t0:t0 + T], 1)
    sn = pick(t["state_noise"][:S, t0:t0 + T], 2) if mode == "noisy" else None
    z = None
    if x0 is not None:
        start = pick(x0, x0.ndim - 2)
    elif mode == "gaussian":
        from vjf_amd import Gaussian
        mean = pick(t["x0"], 0)
        start, z = Gaussian(mean, torch.full_like(mean, ec.LOGVAR0)), pick(t["x0_noise"][:S], 1)
    else:
        start = pick(t["x0"], 0)
    return m.forecast_ensemble(start, u, T, S, w_noise=t["w_noise"][:S, t0:t0 + T], state_noise=sn, x0_noise=z, return_members=members)


# ------------------------------------------------------------------ 1
PARITY = [(name, 8, mode) for name in ec.CASES for mode in ("quiet", "noisy")] + \
         [("ragged3", 8, "gaussian"), ("control", 8, "gaussian"), ("wide", 3, "quiet"), ("wide", 3, "noisy")]


@pytest.mark.parametrize("name,S,mode", PARITY)
def test_parity_against_the_fp64_oracle(vjf, name, S, mode):
    m, t = case(vjf, name)
    refs = ec.references(m, name, S, mode)
    r = ens(m, t, S, mode)
    assert r.x is None
    for k in MOMENTS:
        r64, r32 = refs[k]
        assert getattr(r, k).shape == r64.shape
        by_rule(f"{name} S={S} {mode} {k}", getattr(r, k), r64, r32)


# ------------------------------------------------------------------ 2
BITWISE = ["ragged3", "wide"]


@pytest.mark.parametrize("name", BITWISE)
def test_members_are_forecast_sequence(vjf, name):
    m, t = case(vjf, name)
    T, S = fc.CASES[name][5], ec.S_MAX
    r = ens(m, t, members=True)
    assert r.x.shape == (S, T + 1) + tuple(t["x0"].shape)
    for s in range(S):
        x = m.transition.forecast_sequence(t["x0"], t["u"], T, w_noise=t["w_noise"][s], state_noise=t["state_noise"][s])
        same_bits(r.x[s], x, f"member {s}")


@pytest.mark.parametrize("name", BITWISE)
def test_one_member_is_the_rollout(vjf, name):
    m, t = case(vjf, name)
    T = fc.CASES[name][5]
    r = ens(m, t, S=1, members=True)
    x, y = m.forecast_sequence(t["x0"], t["u"], T, w_noise=t["w_noise"][0], state_noise=t["state_noise"][0])
    same_bits(r.x_mean, x, "x_mean")
    same_bits(r.x[0], x, "the member")
    assert not r.x_var.any() and not r.y_var.any()                   # exactly 0
    a = fc.inputs(name)
    z = ec.noises(name)
    (_, y64), (_, y32) = fc.oracles(m, a["x0"], a["u"], z["w_noise"][0], z["state_noise"][0])
    by_rule(f"{name} S=1 y_mean", r.y_mean, y64, y32)
    by_rule(f"{name} S=1 forecast_sequence's y", y, y64, y32)
    b = fc.bound(y64, y32)
    assert float((r.y_mean.double() - y.double()).abs().max()) <= ec.F * b


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "quiet"])
@pytest.mark.parametrize("updated", [True, False], ids=["after_rls", "fresh"])
def test_seeded_drop_in_for_successive_forecast_sequences(vjf, updated, noise):
    xdim, udim, n, ydim, B, T, S = 5, 2, 37, 21, 37, 12, 3
    torch.manual_seed(17)
    m = vjf.VJF.make_model(ydim, xdim, udim, n, fc.HIDDEN, likelihood="gaussian")
    g = torch.Generator().manual_seed(18)
    x0, u = torch.randn(B, xdim, generator=g), torch.randn(T, B, udim, generator=g)
    if updated:
        m.filter(torch.randn(B, ydim, generator=g), torch.randn(B, udim, generator=g), update=True)
        assert m.check_status() == 0 and m.transition.velocity._w_colmajor
    torch.manual_seed(99)
    seq = [m.forecast_sequence(x0, u, T, noise=noise) for _ in range(S)]
    state = torch.get_rng_state()
    torch.manual_seed(99)
    r = m.forecast_ensemble(x0, u, T, S, noise=noise, return_members=True)
    assert torch.equal(torch.get_rng_state(), state)
    for s in range(S):
        same_bits(r.x[s], seq[s][0], f"member {s}")
    xs, ys = torch.stack([a for a, _ in seq]).double(), torch.stack([b for _, b in seq]).double()
    scale = max(float(xs.abs().max()), float(ys.abs().max()), 1.)
    for k, ref in (("x_mean", xs.mean(0)), ("x_var", xs.var(0, unbiased=False)), ("y_mean", ys.mean(0)), ("y_var", ys.var(0, unbiased=False))):
        # (the members are the same bits, so the moments differ from the members' fp64 moments by the fp32 fold and the fp32 decoding)
        check_close(getattr(r, k).double().cpu().numpy(), ref.cpu().numpy(), rtol=0, atol=64 * fc.EPS32 * scale ** (2 if "var" in k else 1))


# ------------------------------------------------------------------ 4
@pytest.fixture(scope="module")
def full(vjf):
    return {name: ens(*case(vjf, name), members=True) for name in BITWISE}


@pytest.mark.parametrize("name", BITWISE)
def test_bits_permuted_trials(vjf, full, name):
    m, t = case(vjf, name)
    perm = torch.randperm(t["x0"].shape[0], generator=torch.Generator().manual_seed(3)).cuda()
    same_moments(ens(m, t, rows=perm), full[name], "permuted trials", rows=perm)


@pytest.mark.parametrize("name", BITWISE)
def test_bits_sub_batches(vjf, full, name):
    """A whole first tile, the ragged last tile ([32:37] of 37 trials; [16:18] of 18) and a single trial."""
    m, t = case(vjf, name)
    B = t["x0"].shape[0]
    for lo, hi in ((0, 16), (B - B % 16, B), (B - 2, B - 1)):
        same_moments(ens(m, t, rows=torch.arange(lo, hi).cuda()), full[name], f"trials [{lo}:{hi}]", rows=slice(lo, hi))


@pytest.mark.parametrize("env", [dict(VJF_FC_CHUNK="7"), dict(VJF_FE_MEMBERS="3"), dict(VJF_FC_CHUNK="7", VJF_FE_MEMBERS="3"),
                                 dict(VJF_FC_LOOKAHEAD="0"), dict(VJF_FC_CENTROID_LDS="0")], ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
@pytest.mark.parametrize("name", BITWISE)
def test_bits_chunking_and_the_forms_of_the_kernels(vjf, full, name, env, monkeypatch):
    """Chunks of 7 steps; chunks of 3 members (8 = 3 + 3 + 2: a ragged last chunk, the running moments crossing the output arrays
    twice); both; the roll-out without look-ahead (and the moments staging one member per barrier); centroids and decoder from global
    memory."""
    m, t = case(vjf, name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = ens(m, t, members=True)
    same_moments(r, full[name], str(env))
    same_bits(r.x, full[name].x, f"{env}: members")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_other_stream(vjf, full, name):
    m, t = case(vjf, name)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r = ens(m, t)
    side.synchronize()
    same_moments(r, full[name], "side stream")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_split_horizon(vjf, full, name):
    """T steps in one call = k steps, then T - k from the members' x[:, k] as an (S, B, xdim) start with the noise slices."""
    m, t = case(vjf, name)
    T = t["w_noise"].shape[1]
    k = 25 if T > 25 else 13
    head = ens(m, t, T=k, members=True)
    same_moments(head, full[name], "head", steps=slice(0, k + 1))
    tail = ens(m, t, t0=k, x0=head.x[:, k].clone(), members=True)
    same_moments(tail, full[name], "tail", steps=slice(k, None))
    same_bits(tail.x, full[name].x[:, k:], "tail members")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_member_prefix(vjf, full, name):
    m, t = case(vjf, name)
    same_bits(ens(m, t, S=3, members=True).x, full[name].x[:3], "the first 3 members")


# ------------------------------------------------------------------ 5
def test_scratch_bound_and_a_long_horizon_of_many_members(vjf, monkeypatch):
    from vjf_amd import _native as N
    nbytes = ctypes.c_int64()
    assert N.lib().vjf_forecast_ens_scratch_size(10 ** 9, 10 ** 6, 4096, 200, 10, ctypes.byref(nbytes)) == 0
    assert 0 < nbytes.value <= (8 << 20) + (32 << 20) + 4096        # the documented cap (include/vjf_hip.h)
    m, _ = case(vjf, "ragged3")
    xdim, udim, n, ydim, _, _ = fc.CASES["ragged3"]
    T, S, B = 300, 40, 3
    g = torch.Generator().manual_seed(7)
    x0, wn = torch.randn(B, xdim, generator=g).cuda(), torch.randn(S, T, n, xdim, generator=g).cuda()
    a = m.forecast_ensemble(x0, None, T, S, w_noise=wn)
    monkeypatch.setenv("VJF_FC_CHUNK", "64")
    monkeypatch.setenv("VJF_FE_MEMBERS", "7")
    b = m.forecast_ensemble(x0, None, T, S, w_noise=wn)
    for k in MOMENTS:
        assert torch.isfinite(getattr(a, k)).all(), k
    same_moments(a, b, "T = 300, S = 40")


def moments_equal(a, b, what):
    for k in MOMENTS:
        assert torch.isfinite(getattr(a, k)).all(), f"{what}: {k}"
    same_moments(a, b, what)


@pytest.mark.parametrize("name,S", [("configB", 2000), ("ragged3", 40000)])
def test_one_step_of_many_members(vjf, name, S, monkeypatch):
    """n_step = 1 (the default) with many members and B = 3.  configB's model, S = 2000: one step's weight samples of all members are
    16 MB, more than the 8 MiB cap, so the default chunking splits the members.  ragged3's model, S = 40000: more members than a
    chunk may hold (4096).  Bitwise against chunks of 7 members."""
    from vjf_amd import _native as N
    m, _ = case(vjf, name)
    xdim, udim, n, ydim, _, _ = fc.CASES[name]
    T, B = 1, 3
    sc, tc = ctypes.c_int32(), ctypes.c_int32()
    assert N.lib().vjf_forecast_ens_chunks(T, S, B, n, xdim, ctypes.byref(sc), ctypes.byref(tc)) == 0
    assert tc.value == 1 and sc.value < S and sc.value * n * xdim * 4 <= 8 << 20 < S * n * xdim * 4
    g = torch.Generator().manual_seed(11)
    x0, wn = torch.randn(B, xdim, generator=g).cuda(), torch.randn(S, T, n, xdim, generator=g).cuda()
    a = m.forecast_ensemble(x0, None, T, S, w_noise=wn)
    monkeypatch.setenv("VJF_FE_MEMBERS", "7")
    moments_equal(a, m.forecast_ensemble(x0, None, T, S, w_noise=wn), f"T = 1, S = {S}")


@pytest.mark.parametrize("T,S", [(1, 128), (24, 16)], ids=["one_step_128_members", "24_steps_16_members"])
def test_the_state_cap_drives_the_default_chunking(vjf, T, S, monkeypatch):
    """configB's model with 4096 trials: one member-step is 160 KB of states.  T = 1, S = 128 needs 2 x 128 rows = 42 MB, and T = 24,
    S = 16 needs 16 x 25 rows = 66 MB, both more than the 32 MiB cap: the default chunking splits the members (and keeps all 24
    steps).  Bitwise against short chunks of both kinds, with state noise and the members kept in the second call only."""
    from vjf_amd import _native as N
    m, _ = case(vjf, "configB")
    xdim, udim, n, ydim, _, _ = fc.CASES["configB"]
    B = 4096
    sc, tc = ctypes.c_int32(), ctypes.c_int32()
    assert N.lib().vjf_forecast_ens_chunks(T, S, B, n, xdim, ctypes.byref(sc), ctypes.byref(tc)) == 0
    assert sc.value < S and tc.value == T and sc.value * (tc.value + 1) * B * xdim * 4 <= 32 << 20
    g = torch.Generator().manual_seed(12)
    x0, wn = torch.randn(B, xdim, generator=g).cuda(), torch.randn(S, T, n, xdim, generator=g).cuda()
    sn = torch.randn(S, T, B, xdim, generator=g).cuda()
    a = m.forecast_ensemble(x0, None, T, S, w_noise=wn, state_noise=sn)
    monkeypatch.setenv("VJF_FE_MEMBERS", "7")
    monkeypatch.setenv("VJF_FC_CHUNK", "5")
    b = m.forecast_ensemble(x0, None, T, S, w_noise=wn, state_noise=sn, return_members=True)
    moments_equal(a, b, f"T = {T}, S = {S}, B = 4096")
    same_bits(b.x[S - 1], m.transition.forecast_sequence(x0, None, T, w_noise=wn[S - 1], state_noise=sn[S - 1]), "the last member")


# ------------------------------------------------------------------ 6
def test_no_side_effects(vjf):
    m, t = case(vjf, "control")
    m._ensure_ctx(t["x0"].shape[0])
    before = m._blob.clone()
    counters = (m.transition.n_sample, m.likelihood.n_sample)
    m.forecast_ensemble(t["x0"], t["u"], fc.CASES["control"][5], 4, noise=True)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), m._blob.view(torch.int32))
    assert (m.transition.n_sample, m.likelihood.n_sample) == counters
    assert m.status() == 0


# ------------------------------------------------------------------ 7
def test_edges(vjf):
    m, t = case(vjf, "control")
    xdim, udim, n, ydim, B, T = fc.CASES["control"]
    S = 4
    # n_step = 0: the start, its variance across the members (exactly 0 for a shared start), the decoded start
    r = m.forecast_ensemble(t["x0"], t["u"][:0], 0, S, return_members=True)
    assert r.x_mean.shape == (1, B, xdim) and r.y_mean.shape == (1, B, ydim) and r.x.shape == (S, 1, B, xdim)
    same_bits(r.x_mean[0], t["x0"], "n_step = 0")
    assert not r.x_var.any() and not r.y_var.any()
    y0 = m.forecast_sequence(t["x0"], t["u"][:0], 0)[1]
    check_close(r.y_mean.cpu().numpy(), y0.cpu().numpy(), rtol=0, atol=8 * fc.EPS32 * float(y0.abs().max()))
    starts = t["x0"] + 0.2 * t["x0_noise"][:S]
    r = m.forecast_ensemble(starts, t["u"][:0], 0, S, return_members=True)
    same_bits(r.x[:, 0], starts, "the starts")
    check_close(r.x_mean[0].cpu().numpy(), starts.double().mean(0).cpu().numpy(), rtol=0, atol=4 * fc.EPS32 * float(starts.abs().max()))
    check_close(r.x_var[0].cpu().numpy(), starts.double().var(0, unbiased=False).cpu().numpy(), rtol=0, atol=1e-6)
    # B = 1, given as one row and as a 1-D x0 (u and the state noise without their batch axis): the rows of the full batch
    full = ens(m, t, S=S)
    one = m.forecast_ensemble(t["x0"][4:5], t["u"][:, 4:5], T, S, w_noise=t["w_noise"][:S], state_noise=t["state_noise"][:S, :, 4:5])
    flat = m.forecast_ensemble(t["x0"][4], t["u"][:, 4], T, S, w_noise=t["w_noise"][:S], state_noise=t["state_noise"][:S, :, 4])
    assert one.x_mean.shape == flat.x_mean.shape == (T + 1, 1, xdim)
    same_moments(one, full, "B = 1", rows=slice(4, 5))
    same_moments(flat, one, "1-D x0")
    # RBFDS.forecast_ensemble: no decoder there
    tr = m.transition.forecast_ensemble(t["x0"], t["u"], T, S, w_noise=t["w_noise"][:S], state_noise=t["state_noise"][:S], return_members=True)
    assert len(tr) == 3
    same_bits(tr[0], full.x_mean, "RBFDS x_mean")
    same_bits(tr[1], full.x_var, "RBFDS x_var")
    assert tr[2].shape == (S, T + 1, B, xdim)
    with pytest.raises(ValueError):
        m.forecast_ensemble(t["x0"], t["u"], T, 0)
    with pytest.raises(TypeError):
        m.forecast_ensemble(t["x0"], None, T, S)
    with pytest.raises(AssertionError):
        m.forecast_ensemble(t["x0"], t["u"], T, S, w_noise=t["w_noise"][:S, :, :-1])
    with pytest.raises(AssertionError):
        m.forecast_ensemble(t["x0"], t["u"], T, S, w_noise=t["w_noise"][:S - 1])
    with pytest.raises(AssertionError):
        m.forecast_ensemble(t["x0"], t["u"], T, S, state_noise=t["state_noise"][:S, :-1])
    with pytest.raises(AssertionError):
        from vjf_amd import Gaussian
        m.forecast_ensemble(Gaussian(t["x0"], torch.zeros_like(t["x0"])), t["u"], T, S, x0_noise=t["x0_noise"][:S, :-1])
    with pytest.raises(AssertionError):
        m.forecast_ensemble(t["x0"], t["u"][:-1], T, S)


def test_raw_abi_refusals(vjf):
    from vjf_amd import _native as N
    L = N.lib()
    m, t = case(vjf, "control")
    xdim, udim, n, ydim, B, T = fc.CASES["control"]
    S = 4
    vel, dec = m.transition.velocity, m.decoder.decode
    new = lambda *s: torch.empty(*s, device="cuda")          # noqa: E731
    xm, xv, ym, yv = new(T + 1, B, xdim), new(T + 1, B, xdim), new(T + 1, B, ydim), new(T + 1, B, ydim)
    nbytes = ctypes.c_int64()
    assert L.vjf_forecast_ens_scratch_size(T, 0, B, n, xdim, ctypes.byref(nbytes)) == -20
    assert b"vjf_forecast_ens_scratch_size" in L.vjf_last_error()
    assert L.vjf_forecast_ens_scratch_size(T, S, B, n, xdim, ctypes.byref(nbytes)) == 0
    assert S * T * n * xdim * 4 + S * (T + 1) * B * xdim * 4 <= nbytes.value <= 1 << 20
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    p = N.ptr
    wn, sn = t["w_noise"][:S].contiguous(), t["state_noise"][:S].contiguous()

    def call(x0=t["x0"], stride=0, T=T, S=S, B=B, n=n, d=xdim + udim, dout=xdim, u=t["u"]):
        return L.vjf_forecast_ens(p(x0), stride, p(u), p(wn), p(sn), p(vel.feature.centroid),
                                  p(vel.feature.logwidth), p(vel.w_mean), p(vel.w_chol), p(m.transition.logvar), p(dec.weight), p(dec.bias),
                                  p(xm), p(xv), p(ym), p(yv), None, p(scratch), T, S, B, n, d, dout, ydim, None)
    for rc, kw in ((-1, dict(x0=None)), (-20, dict(T=-1)), (-20, dict(S=0)), (-20, dict(B=0)), (-20, dict(d=xdim - 1)), (-20, dict(stride=7)),
                   (-21, dict(u=None)), (-11, dict(n=3000))):
        assert call(**kw) == rc, kw                     # (every refusal comes before the first launch: nothing is read or written)
        assert b"vjf_forecast_ens" in L.vjf_last_error()
    assert call() == 0
    torch.cuda.synchronize()
    r = ens(m, t, S=S)
    for k, got in zip(MOMENTS, (xm, xv, ym, yv)):
        same_bits(got, getattr(r, k), f"raw call: {k}")
