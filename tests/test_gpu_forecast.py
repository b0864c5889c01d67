"""`forecast_sequence` (vjf_forecast_seq): the sampled roll-out of a whole horizon in one native call.

  1. parity against the fp64 oracle on synthetic seeded states (tests/forecast_cases.py: the shapes, the inputs and the rule);
  2. the reference's own recorded roll-out (g8_fit);
  3. a seeded drop-in for `forecast`: same draws in the same order, the generator left in the same state;
  4. bitwise properties: permuted rows, sub-batches, chunking, a split horizon, another stream, the two forms of the kernel;
  5. no side effects on the model;
  6. edges and refusals.

All tests need a real MI355X:  pytest -m gpu."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import vjf_oracle as orc
from tests import forecast_cases as fc
from tests import goldenio as gio
from tests.helpers import load_fixture_state, load_oracle_state
from tests.margins import check_close

pytestmark = pytest.mark.gpu


def close(a, b, **kw):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    check_close(np.asarray(a, np.float64), np.asarray(b, np.float64), **kw)      # (asserts, and records the achieved margin)


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


_CACHE = {}


def case(vjf, name):
    """(model, inputs as device tensors, ((x64, y64), (x32, y32)) with state noise, the same without): built once per module."""
    if name not in _CACHE:
        m = fc.make_model(vjf, name)
        a = fc.inputs(name)
        with_noise = fc.oracles(m, a["x0"], a["u"], a["w_noise"], a["state_noise"])
        without = fc.oracles(m, a["x0"], a["u"], a["w_noise"], None)
        t = {k: None if v is None else torch.as_tensor(v).cuda() for k, v in a.items()}
        _CACHE[name] = (m, t, with_noise, without)
    return _CACHE[name]


def same_bits(a, b, what=""):
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} against {tuple(b.shape)}"
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), \
        f"{what}: differs by {float((a.double() - b.double()).abs().max()):.3e}"


def by_rule(what, got, ref64, other, F=fc.F):
    """max|got - ref64| <= F max(E, 8 eps max|ref64|), E = max|other - ref64|; prints the achieved ratio before it asserts."""
    b = fc.bound(ref64, other)
    g = got.detach().cpu().numpy().astype(np.float64)
    err = float(np.abs(g - ref64).max())
    print(f"forecast margin: {what}: err {err:.3e} bound {b:.3e} ratio {err / b:.3f} (F = {F})")
    close(g, ref64, rtol=0, atol=F * b, what=f"{what} [ratio = used * {F}]")


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("state_noise", [False, True], ids=["quiet", "noisy"])
@pytest.mark.parametrize("name", list(fc.CASES))
def test_parity_against_the_fp64_oracle(vjf, name, state_noise):
    m, t, noisy, quiet = case(vjf, name)
    (x64, y64), (x32, y32) = noisy if state_noise else quiet
    x, y = m.forecast_sequence(t["x0"], t["u"], fc.CASES[name][5], w_noise=t["w_noise"],
                               state_noise=t["state_noise"] if state_noise else None)
    assert x.shape == x64.shape and y.shape == y64.shape
    same_bits(x[0], t["x0"], "x[0]")
    by_rule(f"{name} x", x, x64, x32, fc.factor(name, state_noise))
    by_rule(f"{name} y", y, y64, y32, fc.factor(name, state_noise))


# ------------------------------------------------------------------ 2
def test_the_references_recorded_rollout(vjf):
    """g8_fit: the state fit() of the reference ended with (`sT.*`), its recorded weight noise, its x and y."""
    z = gio.load("g8_fit")
    T, B, dy, dz, du, n = [int(v) for v in z["meta"][:6]]
    hid = [int(v) for v in z["meta"][6:]]
    m = vjf.VJF.make_model(dy, dz, du, n, hid, likelihood="gaussian")
    load_fixture_state(m, z, "sT")
    wn = z["fc_wnoise"]
    x, y = m.forecast_sequence(torch.tensor(z["fc_x0"]), None, wn.shape[0], w_noise=torch.tensor(wn))
    s32 = gio.state_from(z, "sT", ydim=dy, xdim=dz, udim=du, n_rbf=n, hidden=hid, likelihood=orc.GAUSSIAN).cast(np.float32)
    x32, y32 = orc.forecast(s32, z["fc_x0"].astype(np.float32), None, wn.shape[0], wn.astype(np.float32))
    by_rule("g8 x", x, z["fc_x"].reshape(x.shape), x32)
    by_rule("g8 y", y, z["fc_y"].reshape(y.shape), y32)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("noise", [True, False], ids=["noise", "quiet"])
@pytest.mark.parametrize("updated", [True, False], ids=["after_rls", "fresh"])
def test_seeded_drop_in_for_forecast(vjf, updated, noise):
    """`forecast` and `forecast_sequence` under the same seed: the same draws (so both are the oracle's roll-out on those draws, the
    sequence call within F times what the per-step path itself is off by), and the generator left in the same state.  After an RLS
    update the weight draw is the strided one (`_w_colmajor`)."""
    xdim, udim, n, ydim, B, T = 5, 2, 37, 21, 37, 12
    torch.manual_seed(17)
    m = vjf.VJF.make_model(ydim, xdim, udim, n, fc.HIDDEN, likelihood="gaussian")
    g = torch.Generator().manual_seed(18)
    x0, u = torch.randn(B, xdim, generator=g), torch.randn(T, B, udim, generator=g)
    if updated:
        m.filter(torch.randn(B, ydim, generator=g), torch.randn(B, udim, generator=g), update=True)
        assert m.check_status() == 0 and m.transition.velocity._w_colmajor
    torch.manual_seed(99)
    xa, ya = m.forecast(x0, u, T, noise=noise)
    state_a = torch.get_rng_state()
    torch.manual_seed(99)
    xb, yb = m.forecast_sequence(x0, u, T, noise=noise)
    state_b = torch.get_rng_state()
    assert torch.equal(state_a, state_b)
    torch.manual_seed(99)                                    # the draws themselves, for the oracle
    ws, ss = [], []
    for _ in range(T):
        ws.append(m.transition.velocity._draw_weight_noise().numpy())
        if noise:
            ss.append(torch.randn(B, xdim).numpy())
    assert torch.equal(torch.get_rng_state(), state_a)
    s64 = load_oracle_state(m, np.float64)
    x64, y64 = orc.forecast(s64, x0.numpy().astype(np.float64), u.numpy().astype(np.float64), T, np.stack(ws).astype(np.float64),
                            np.stack(ss).astype(np.float64) if noise else None)
    assert xa.shape == xb.shape and ya.shape == yb.shape
    by_rule("drop-in x", xb, x64, xa.cpu().numpy())
    by_rule("drop-in y", yb, y64, ya.cpu().numpy())


# ------------------------------------------------------------------ 4
BITWISE = ["ragged3", "wide"]


def run(m, t, T=None, rows=None, x0=None, t0=0, state_noise=True):
    """x of forecast_sequence on the case's inputs: steps t0 .. t0 + T - 1, trials `rows` (an index tensor), explicit noise."""
    T = t["w_noise"].shape[0] - t0 if T is None else T
    pick = (lambda a: a) if rows is None else (lambda a: a[:, rows].contiguous())
    u = None if t["u"] is None else pick(t["u"][t0:t0 + T])
    sn = pick(t["state_noise"][t0:t0 + T]) if state_noise else None
    x0 = t["x0"] if x0 is None else x0
    x0 = x0 if rows is None else x0[rows].contiguous()
    return m.transition.forecast_sequence(x0, u, T, w_noise=t["w_noise"][t0:t0 + T], state_noise=sn)


@pytest.fixture(scope="module")
def full(vjf):
    return {name: run(*case(vjf, name)[:2]) for name in BITWISE}


@pytest.mark.parametrize("name", BITWISE)
def test_bits_permuted_rows(vjf, full, name):
    m, t = case(vjf, name)[:2]
    perm = torch.randperm(t["x0"].shape[0], generator=torch.Generator().manual_seed(3)).cuda()
    same_bits(run(m, t, rows=perm), full[name][:, perm], "permuted rows")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_sub_batches(vjf, full, name):
    """A whole first tile, the ragged last tile ([32:37] of 37 trials; [16:18] of 18) and a single trial."""
    m, t = case(vjf, name)[:2]
    B = t["x0"].shape[0]
    for lo, hi in ((0, 16), (B - B % 16, B), (B - 2, B - 1)):
        rows = torch.arange(lo, hi).cuda()
        same_bits(run(m, t, rows=rows), full[name][:, lo:hi], f"trials [{lo}:{hi}]")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_chunking(vjf, full, name, monkeypatch):
    m, t = case(vjf, name)[:2]
    monkeypatch.setenv("VJF_FC_CHUNK", "7")
    same_bits(run(m, t), full[name], "VJF_FC_CHUNK=7")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_split_horizon(vjf, full, name):
    """T steps in one call = k steps, then T - k from x[k] with the noise slices; k = 25 where the horizon is longer than that (T =
    40), 13 for T = 24."""
    m, t = case(vjf, name)[:2]
    T = t["w_noise"].shape[0]
    k = 25 if T > 25 else 13
    head = run(m, t, T=k)
    tail = run(m, t, x0=head[k].clone(), t0=k)
    same_bits(head, full[name][:k + 1], "head")
    same_bits(tail, full[name][k:], "tail")


@pytest.mark.parametrize("name", BITWISE)
def test_bits_other_stream(vjf, full, name):
    m, t = case(vjf, name)[:2]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = run(m, t)
    side.synchronize()
    same_bits(x, full[name], "side stream")


@pytest.mark.parametrize("env", ["VJF_FC_LOOKAHEAD", "VJF_FC_CENTROID_LDS"])
@pytest.mark.parametrize("name", list(fc.CASES))
def test_bits_the_forms_of_the_kernel_agree(vjf, name, env, monkeypatch):
    """The form for shapes beyond the register / LDS budgets (W[t] read when used; centroids from global memory), forced at the
    test shapes: the same MFMA steps on the same operands in the same order, so the same bits -- and so the parity above holds for it."""
    m, t = case(vjf, name)[:2]
    want = run(m, t)
    monkeypatch.setenv(env, "0")
    same_bits(run(m, t), want, f"{env}=0")


def test_bits_horizon_beyond_one_default_chunk(vjf, monkeypatch):
    """4100 steps (the default chunk is at most 4096) against chunks of 1000, on a bounded scratch."""
    m, t = case(vjf, "ragged3")[:2]
    xdim, udim, n, ydim, B, _ = fc.CASES["ragged3"]
    T, B = 4100, 3
    g = torch.Generator().manual_seed(7)
    x0, wn = torch.randn(B, xdim, generator=g).cuda(), torch.randn(T, n, xdim, generator=g).cuda()
    nbytes = ctypes.c_int64()
    from vjf_amd import _native as N
    assert N.lib().vjf_forecast_scratch_size(10 ** 9, 200, 10, ctypes.byref(nbytes)) == 0 and nbytes.value <= (8 << 20) + 4096
    a = m.transition.forecast_sequence(x0, None, T, w_noise=wn)
    monkeypatch.setenv("VJF_FC_CHUNK", "1000")
    b = m.transition.forecast_sequence(x0, None, T, w_noise=wn)
    assert torch.isfinite(a).all()
    same_bits(a, b, "4100 steps")


# ------------------------------------------------------------------ 5
def test_no_side_effects(vjf):
    m, t = case(vjf, "control")[:2]
    m._ensure_ctx(t["x0"].shape[0])
    before = m._blob.clone()
    counters = (m.transition.n_sample, m.likelihood.n_sample)
    m.forecast_sequence(t["x0"], t["u"], fc.CASES["control"][5], noise=True)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), m._blob.view(torch.int32))
    assert (m.transition.n_sample, m.likelihood.n_sample) == counters
    assert m.status() == 0


# ------------------------------------------------------------------ 6
def test_edges(vjf):
    m, t, noisy, quiet = case(vjf, "control")
    xdim, udim, n, ydim, B, T = fc.CASES["control"]
    x, y = m.forecast_sequence(t["x0"], t["u"][:0], 0)
    assert x.shape == (1, B, xdim) and y.shape == (1, B, ydim)
    same_bits(x[0], t["x0"], "n_step = 0")
    close(y[0], quiet[0][1][0], rtol=0, atol=fc.F * fc.bound(quiet[0][1][0], quiet[1][1][0]))
    # B = 1, given as one row and as a 1-D x0 (u without its batch axis): the rows of the full batch
    full = run(m, t, state_noise=False)
    one = m.transition.forecast_sequence(t["x0"][4:5], t["u"][:, 4:5], T, w_noise=t["w_noise"])
    flat = m.transition.forecast_sequence(t["x0"][4], t["u"][:, 4], T, w_noise=t["w_noise"])
    assert one.shape == flat.shape == (T + 1, 1, xdim)
    same_bits(one, full[:, 4:5], "B = 1")
    same_bits(flat, one, "1-D x0")
    with pytest.raises(TypeError):
        m.forecast_sequence(t["x0"], None, T)
    with pytest.raises(AssertionError):
        m.forecast_sequence(t["x0"], t["u"], T, w_noise=t["w_noise"][:, :-1])
    with pytest.raises(AssertionError):
        m.forecast_sequence(t["x0"], t["u"], T, state_noise=t["state_noise"][:-1])
    with pytest.raises(AssertionError):
        m.forecast_sequence(t["x0"], t["u"][:-1], T)


def test_raw_abi_refusals(vjf):
    from vjf_amd import _native as N
    L = N.lib()
    m, t = case(vjf, "control")[:2]
    xdim, udim, n, ydim, B, T = fc.CASES["control"]
    vel = m.transition.velocity
    x = torch.empty(T + 1, B, xdim, device="cuda")
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    p = N.ptr

    def call(x0=t["x0"], T=T, B=B, n=n, d=xdim + udim, dout=xdim, u=t["u"]):
        return L.vjf_forecast_seq(p(x0), p(u), p(t["w_noise"]), None, p(vel.feature.centroid), p(vel.feature.logwidth), p(vel.w_mean),
                                  p(vel.w_chol), p(m.transition.logvar), p(x), p(scratch), T, B, n, d, dout, None)
    for rc, kw in ((-1, dict(x0=None)), (-20, dict(T=0)), (-20, dict(B=0)), (-20, dict(d=xdim - 1)), (-21, dict(u=None)),
                   (-11, dict(n=3000))):
        assert call(**kw) == rc, kw                     # (every refusal comes before the first launch: nothing is read or written)
        assert b"vjf_forecast_seq" in L.vjf_last_error()
    nbytes = ctypes.c_int64()
    assert L.vjf_forecast_scratch_size(0, n, xdim, ctypes.byref(nbytes)) == -20
    assert L.vjf_forecast_scratch_size(T, n, xdim, ctypes.byref(nbytes)) == 0 and T * n * xdim * 4 <= nbytes.value <= 1 << 20
    assert call() == 0
    torch.cuda.synchronize()
    same_bits(x, run(m, t, state_noise=False), "raw call")
