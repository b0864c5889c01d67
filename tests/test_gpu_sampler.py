"""`sample_posterior` (vjf_smooth_sample): joint draws from the smoothed posterior by backward sampling in one native call.

  1. parity of the draws against the fp64 reference (tests/sampler_cases.py: the cases, the kinds, the noise, the rule);
  2. zero noise is `smooth`'s mean, bit for bit;
  3. edge sizes: T = 1, T = 2, S = 1;
  4. bitwise invariances: the member's index, S, the members per workgroup, VJF_FC_CENTROID_LDS, the batch size, the trial's row, the
     tile-mates, a repeat, the stream;
  5. chunks with `after`;
  6. poisoning: a NaN row of a trial, NaN noise of a member;
  7. refusals through the real library and no side effects.

All tests need a real MI355X:  pytest -m gpu."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import sampler_cases as pc
from tests import sampler_ref as pr
from tests.margins import check_close

pytestmark = pytest.mark.gpu
NAMES = list(pc.CASES)
KINDS = list(pc.KINDS)
F = pc.F


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_MODEL, _IN, _OUT = {}, {}, {}


def model_of(vjf, name):
    if name not in _MODEL:
        _MODEL[name] = pc.make_model(vjf, name)
    return _MODEL[name]


def dev(name, kind="typical"):
    """{mu, lv, u, z} of the case as device tensors: once per module."""
    if (name, kind) not in _IN:
        t = {k: None if v is None else torch.as_tensor(v).cuda() for k, v in pc.inputs(name, kind).items()}
        t["z"] = torch.as_tensor(pc.noise(name)).cuda()
        _IN[(name, kind)] = t
    return _IN[(name, kind)]


def run(vjf, name, kind="typical", rows=None, lo=0, hi=None, mu=None, z=None, members=None, after=None, **kw):
    """`sample_posterior` on the trials `rows`, the time rows [lo, hi) and the members `members` of the case (u cut to match, one
    more row with `after`)."""
    t = dev(name, kind)
    mu = t["mu"] if mu is None else mu
    z = t["z"] if z is None else z
    lv, u = t["lv"], t["u"]
    hi = mu.shape[0] if hi is None else hi
    hu = hi + (after is not None)
    mu, lv, u, z = mu[lo:hi], lv[lo:hi], None if u is None else u[lo:hu], z[:, lo:hi]
    if rows is not None:
        mu, lv, u, z = mu[:, rows], lv[:, rows], None if u is None else u[:, rows], z[:, :, rows]
        after = None if after is None else after[:, rows]
    if members is not None:
        z = z[members]
        after = None if after is None else after[members]
    kw = {"state_var": pc.Q, **kw}
    return model_of(vjf, name).transition.sample_posterior((mu.contiguous(), lv.contiguous()), None if u is None else u.contiguous(),
                                                           z.shape[0], noise=z.contiguous(), after=after, **kw)


def full(vjf, name, kind="typical"):
    """The undivided call of the case: once per module."""
    if (name, kind) not in _OUT:
        _OUT[(name, kind)] = run(vjf, name, kind)
        torch.cuda.synchronize()
    return _OUT[(name, kind)]


def same_bits(a, b, what=""):
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} against {tuple(b.shape)}"
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f"{what}: differs"


def by_rule(what, got, ref64, other):
    """max|got - ref64| <= F max(E, 8 eps scale), E = max|other - ref64|; prints the achieved ratio before it asserts."""
    b = pc.bound(ref64, other)
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    err = float(np.abs(g - ref64).max())
    print(f"sampler margin: {what}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    check_close(g, np.asarray(ref64, np.float64), rtol=0, atol=F * b, what=f"{what} [ratio = used * {F}]")


def reference_of(name, kind, lo=0, hi=None, members=None):
    """(ref64, ref32) of the rows [lo, hi) drawn on their own (the last row of the cut is the record's last) for `members`."""
    a, z = pc.inputs(name, kind), pc.noise(name)
    z = z if members is None else z[members]
    s64 = pc.state(name)
    out = []
    for s, dt in ((s64, np.float64), (s64.cast(np.float32), np.float32)):
        c = lambda v: None if v is None else np.asarray(v, dt)[lo:hi]          # noqa: E731
        out.append(pr.sample(s, c(a["mu"]), c(a["lv"]), c(a["u"]), dt(pc.Q), np.asarray(z, dt)[:, lo:hi]))
    return out


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_parity_against_the_fp64_reference(vjf, name, kind):
    xdim, udim, n, ydim, B, T = pc.CASES[name]
    out = full(vjf, name, kind)
    assert type(out).__name__ == "PosteriorSamples" and out.x.shape == (pc.MEMBERS[name], T, B, xdim) and out.x.dtype == torch.float32
    same_bits(out.head, out.x[:, 0], "head")
    by_rule(f"{name} {kind} x", out.x, *pc.references(name, kind))


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("kind", ["typical", "mixed"])
@pytest.mark.parametrize("name", ["ragged3", "control", "wide", "x24"])
def test_zero_noise_is_the_smoothed_mean_bit_for_bit(vjf, name, kind):
    t = dev(name, kind)
    sm = model_of(vjf, name).smooth((t["mu"], t["lv"]), t["u"], state_var=pc.Q)
    out = run(vjf, name, kind, z=torch.zeros_like(t["z"][:3]))
    for s in range(3):
        same_bits(out.x[s], sm.mean, f"member {s} with zero noise against smooth's mean")


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", ["control", "x24", "scalar"])
def test_edge_sizes(vjf, name):
    T = pc.CASES[name][5]
    a, z = pc.inputs(name), pc.noise(name)
    one = run(vjf, name, lo=T - 1)                                                       # T = 1: x = mu + sd z
    mu, lv = a["mu"][-1], a["lv"][-1]
    by_rule(f"{name} T = 1", one.x[:, 0], mu.astype(np.float64) + np.exp(0.5 * lv.astype(np.float64)) * z[:, -1].astype(np.float64),
            mu + np.exp(np.float32(0.5) * lv) * z[:, -1])
    same_bits(one.x, full(vjf, name).x[:, T - 1:], "T = 1 against the last row of the whole call")
    by_rule(f"{name} T = 2", run(vjf, name, lo=T - 2).x, *reference_of(name, "typical", lo=T - 2))
    by_rule(f"{name} S = 1", run(vjf, name, members=[0]).x, *reference_of(name, "typical", members=[0]))


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


@pytest.mark.parametrize("name", ["ragged3", "x24"])
def test_bits_members_permuted_and_alone(vjf, name):
    whole = full(vjf, name, "mixed")
    S = pc.MEMBERS[name]
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(4)).tolist()
    same_bits(run(vjf, name, "mixed", members=perm).x, whole.x[perm], "permuted members")
    for s in (0, S // 2, S - 1):
        same_bits(run(vjf, name, "mixed", members=[s]).x, whole.x[[s]], f"member {s} alone")


@pytest.mark.parametrize("name", ["ragged3", "configB", "x24"])
def test_bits_members_per_workgroup(vjf, name, monkeypatch):
    """VJF_SMS_MEMBERS forces the chunk of members a workgroup carries; S itself is the planner's own choice where it fits."""
    whole = full(vjf, name, "mixed")
    S = pc.MEMBERS[name]
    for sc_ in (1, 3, 16, S):
        monkeypatch.setenv("VJF_SMS_MEMBERS", str(sc_))
        same_bits(run(vjf, name, "mixed").x, whole.x, f"VJF_SMS_MEMBERS={sc_}")


@pytest.mark.parametrize("name", NAMES)
def test_bits_the_forms_of_the_kernel_agree(vjf, name, monkeypatch):
    """The form for shapes beyond the LDS budget (centroids and w_mean read from global memory), forced at the test shapes."""
    whole = full(vjf, name, "mixed")
    monkeypatch.setenv("VJF_FC_CENTROID_LDS", "0")
    same_bits(run(vjf, name, "mixed").x, whole.x, "VJF_FC_CENTROID_LDS=0")


@pytest.mark.parametrize("B", [1, 15, 16, 17, 37])
def test_bits_batch_size(vjf, B):
    """The first B trials of ragged3 (37 trials) and B trials from its middle: a trial's draws do not depend on the batch."""
    whole = full(vjf, "ragged3")
    for lo in (0, 37 - B):
        rows = torch.arange(lo, lo + B).cuda()
        same_bits(run(vjf, "ragged3", rows=rows).x, whole.x[:, :, rows], f"trials [{lo}:{lo + B}]")


@pytest.mark.parametrize("name", ["ragged3", "control"])
def test_bits_row_index_tile_mates_repeat_and_stream(vjf, name):
    whole = full(vjf, name, "mixed")
    B = pc.CASES[name][4]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).cuda()
    same_bits(run(vjf, name, "mixed", rows=perm).x, whole.x[:, :, perm], "permuted trials")
    same_bits(run(vjf, name, "mixed").x, whole.x, "a repeat")
    # four trials beside tile-mates whose means are others' (shifted by 3) or NaN
    mu = dev(name, "mixed")["mu"]
    keep = torch.tensor([1, 6, 17, B - 1]).cuda()
    for mates in (mu + 3.0, torch.full_like(mu, float("nan"))):
        mixed = mates.clone()
        mixed[:, keep] = mu[:, keep]
        same_bits(run(vjf, name, "mixed", mu=mixed).x[:, :, keep], whole.x[:, :, keep], "beside other tile-mates")
    torch.cuda.synchronize()
    with own_stream() as side:
        with torch.cuda.stream(side):
            out = run(vjf, name, "mixed")
        side.synchronize()
    same_bits(out.x, whole.x, "side stream")


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("name", ["control", "x24", "ragged3"])
def test_bits_chunked_with_after(vjf, name):
    whole = full(vjf, name)
    T = pc.CASES[name][5]
    for k in (T // 2, 1, T - 1):
        back = run(vjf, name, lo=k)
        front = run(vjf, name, hi=k, after=back.head)
        same_bits(back.x, whole.x[:, k:], f"rows [{k}:]")
        same_bits(front.x, whole.x[:, :k], f"rows [:{k}] with after")
        same_bits(run(vjf, name, hi=k, after=whole.x[:, k].contiguous()).x, whole.x[:, :k], f"rows [:{k}] after x[:, {k}]")
    head = None
    for t in range(T - 1, max(T - 7, -1), -1):                   # a row at a time
        r = run(vjf, name, lo=t, hi=t + 1, after=head)
        same_bits(r.x, whole.x[:, t:t + 1], f"row {t} alone")
        head = r.head


# ------------------------------------------------------------------ 6
def test_poisoning_by_a_nan_row(vjf):
    name = "control"
    whole = full(vjf, name)
    (xdim, udim, n, ydim, B, T), bad = pc.CASES[name], 5
    t0 = T // 2
    others = torch.tensor([r for r in range(B) if r != bad]).cuda()
    for field in ("mu", "lv", "u"):
        t = {k: (None if v is None else v.clone()) for k, v in dev(name).items()}
        t[field][t0 + (field == "u"), bad, 1] = float("nan")          # (u[t0 + 1] drives the step out of row t0)
        out = model_of(vjf, name).sample_posterior((t["mu"], t["lv"]), t["u"], t["z"].shape[0], state_var=pc.Q, noise=t["z"])
        same_bits(out.x[:, :, others], whole.x[:, :, others], f"NaN in {field}: the other trials")
        same_bits(out.x[:, t0 + 1:, bad], whole.x[:, t0 + 1:, bad], f"NaN in {field}: behind the row")
        assert bool(torch.isnan(out.x[:, :t0 + 1, bad]).all()), f"NaN in {field}: every member from the row back"
    # the last row itself
    t = {k: (None if v is None else v.clone()) for k, v in dev(name).items()}
    t["lv"][T - 1, bad, 0] = float("inf")
    out = model_of(vjf, name).sample_posterior((t["mu"], t["lv"]), t["u"], t["z"].shape[0], state_var=pc.Q, noise=t["z"])
    assert bool(torch.isnan(out.x[:, :, bad]).all())
    same_bits(out.x[:, :, others], whole.x[:, :, others], "inf in the last lv: the other trials")


def test_poisoning_by_nan_noise_of_one_member(vjf):
    """NaN noise of member 3, trial 5 at a middle row, component c: by propagation, components 0 .. c of that row (those the
    back-substitution L^T w = z reaches) and every component of the rows before it; nothing else moves."""
    name = "control"
    whole = full(vjf, name)
    (xdim, udim, n, ydim, B, T), bad, s = pc.CASES[name], 5, 3
    t0 = T // 2
    for c in (xdim - 1, 1):
        z = dev(name)["z"].clone()
        z[s, t0, bad, c] = float("nan")
        out = run(vjf, name, z=z)
        want = whole.x.clone()
        want[s, :t0, bad] = float("nan")
        want[s, t0, bad, :c + 1] = float("nan")
        assert bool((torch.isnan(out.x) == torch.isnan(want)).all()), f"component {c}: the NaN region"
        keep = ~torch.isnan(want)
        assert torch.equal(out.x[keep].view(torch.int32), whole.x[keep].view(torch.int32)), f"component {c}: everything else keeps its bits"
    # a non-finite after-row of one member
    k = 7
    after = whole.x[:, k].clone()
    after[s, bad, 0] = float("nan")
    out = run(vjf, name, hi=k, after=after)
    want = whole.x[:, :k].clone()
    want[s, :, bad] = float("nan")
    assert bool((torch.isnan(out.x) == torch.isnan(want)).all())
    keep = ~torch.isnan(want)
    assert torch.equal(out.x[keep].view(torch.int32), whole.x[:, :k][keep].view(torch.int32))


# ------------------------------------------------------------------ 7
def test_refusals_and_no_side_effects(vjf):
    from vjf_amd import _native as N
    L = N.lib()
    name = "control"
    model = model_of(vjf, name)
    xdim, udim, n, ydim, B, T = pc.CASES[name]
    S = pc.MEMBERS[name]
    t = dev(name)
    model._ensure_ctx(B)
    state = model.get_state()
    before = model._blob.clone()
    counters = (model.transition.n_sample, model.likelihood.n_sample)
    big = vjf.VJF.make_model(5, 32, 0, 9, [4], likelihood="gaussian")      # (its initialisation draws: before the generators are read)
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    q = (t["mu"], t["lv"])
    with pytest.raises(TypeError):
        model.sample_posterior(q, n_sample=S, noise=t["z"])
    with pytest.raises(AssertionError):
        model.sample_posterior(q, t["u"][:-1], S, noise=t["z"])
    with pytest.raises(AssertionError, match="noise"):
        model.sample_posterior(q, t["u"], S + 1, noise=t["z"])
    for sv in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            model.sample_posterior(q, t["u"], S, state_var=sv, noise=t["z"])
    with pytest.raises(NotImplementedError):
        big.sample_posterior((torch.zeros(3, 2, 32), torch.zeros(3, 2, 32)), n_sample=2, noise=torch.zeros(2, 3, 2, 32))
    vel = model.transition.velocity
    x = torch.full((S, T, B, xdim), 7.0, device="cuda")
    p = N.ptr

    def call(mu=t["mu"], u=t["u"], z=t["z"], after=None, out=x, T=T, S=S, B=B, n=n, d=xdim + udim, dout=xdim, sv=pc.Q):
        return L.vjf_smooth_sample(p(mu), p(t["lv"]), p(u), p(vel.feature.centroid), p(vel.feature.logwidth), p(vel.w_mean), p(z), p(after),
                                   p(out), T, S, B, n, d, dout, sv, None)
    for rc, kw in ((-1, dict(mu=None)), (-1, dict(z=None)), (-1, dict(out=None)), (-20, dict(T=0)), (-20, dict(S=0)), (-20, dict(sv=0.0)),
                   (-20, dict(sv=float("nan"))), (-20, dict(B=0)), (-21, dict(u=None)), (-11, dict(n=9, d=33, dout=33, u=None)),
                   (-11, dict(n=9, d=32, dout=32, u=None)), (-11, dict(n=1000, d=64, dout=64, u=None)),
                   (-11, dict(n=3000, d=3, dout=3, u=None))):
        assert call(**kw) == rc, kw                      # (every refusal comes before the first launch: nothing is read or written)
        assert b"vjf_smooth_sample" in L.vjf_last_error()
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()), "a refused call wrote x"
    sc_, lds = ctypes.c_int32(), ctypes.c_int64()
    assert L.vjf_smooth_sample_plan(9, 33, 33, 4, ctypes.byref(sc_), ctypes.byref(lds)) == -11
    assert L.vjf_smooth_sample_plan(256, 32, 24, 16, ctypes.byref(sc_), ctypes.byref(lds)) == 0 and 1 <= sc_.value <= 16 and lds.value <= 159 * 1024
    assert call() == 0
    torch.cuda.synchronize()
    same_bits(x, full(vjf, name).x, "raw call")
    assert torch.equal(before.view(torch.int32), model._blob.view(torch.int32))
    after = model.get_state()
    assert after.keys() == state.keys() and all(np.array_equal(np.asarray(v), np.asarray(after[k])) for k, v in state.items())
    assert (model.transition.n_sample, model.likelihood.n_sample) == counters
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(gpu_rng, torch.cuda.get_rng_state())
    assert model.status() == 0
