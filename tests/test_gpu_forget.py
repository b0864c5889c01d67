"""The forgetting factor of the fused RLS update (`transition.shrink`, VJF_SC_SHRINK) on every filter route:
g = shrink P W + Phi'T / v,  P <- shrink P + Phi'Phi / v  in every step that runs the update, nothing else anywhere.

  1  every plan family through the nine-call script of tests/lifetime.py with shrink = 0.9, against the oracle with its `rls` pinned;
  2  the trajectory captured from the reference (tests/golden/make_golden_forget.py), step by step and as one sequence;
  3  shrink = 1 is the code without the factor: bitwise, whether 1 was written or the slot holds the 0 of an older blob;
  4  steps without an RLS update do not see the factor: bitwise;
  5  the factor changed between calls of one context;
  6  a failed factorisation takes the scaled update back;
  7  the sharded route on one rank: bitwise the plain path;
  8  a state saved mid-run carries the factor.

All tests need a real MI355X:  pytest -m gpu."""
import warnings

import numpy as np
import pytest
import torch

from oracle import vjf_oracle as orc
from tests import forget_cases as fc
from tests import goldenio as gio
from tests import lifetime as life
from tests.helpers import load_fixture_state, load_oracle_state, state_close
from tests.margins import check_close

pytestmark = pytest.mark.gpu

POST = dict(rtol=1e-6, atol=1e-6)      # test_filter_trajectory_golden's


def close(a, b, **kw):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    check_close(np.asarray(a, np.float64), np.asarray(b, np.float64), **kw)      # (asserts, and records the achieved margin)


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


def _same_bits(what, k, ma, mb, a, b):
    for name, x, y in zip(("mean", "logvar", "losses"), a, b):
        assert torch.equal(x, y), f"{what}: call {k}: {name} differs by {float((x.double() - y.double()).abs().max()):.3e}"
    assert torch.equal(ma._blob, mb._blob), f"{what}: state after call {k}: {life.blob_diff(ma, mb)}"


def _blob_without_factor(m):
    from vjf_amd import _native as N
    b = m._blob.clone()
    b[m._scalars.storage_offset() + N.SC_SHRINK] = 0.0
    return b


# ------------------------------------------------------------------ 1
LIFE = [(fam, "default") for fam in life.FAMILIES] + [(fam, False) for fam in life.FAMILIES] + [("mega", 3), ("rlsb", 3)]


@pytest.mark.parametrize("fam,overlap", LIFE, ids=[f"{f}-{o}" for f, o in LIFE])
def test_life_with_forgetting(vjf, monkeypatch, fam, overlap):
    """Outputs of every call at lifetime.POST / LOSS against the fp64 oracle, a clean status word; after the last call the whole
    state by lifetime.compare_state (non-RLS tensors at STATE; the four RLS tensors at the fixed RLS tolerance or, noted, within 3 x
    the fp32 oracle's own distance from fp64).  Such a note is accepted for "rlsb" and "wide" only: on the torch-seeded models of
    lifetime.make_model the fp32 oracle alone uses 2.88 and 1.02 of the RLS tolerance there over this script, at most 0.53 ("serial")
    on the other four, and at most 0.14 of POST anywhere; no factorisation fails (forget_cases.reference asserts it).
    Without the feature `shrink` is an attribute nobody reads and the run is the shrink = 1 one: w_precision is 40-73 x the RLS
    tolerance away from this oracle after three updates."""
    m = life.make_model(vjf, fam)
    tr = fc.reference(fam, m, monkeypatch)
    m.transition.shrink = fc.LAM
    if overlap != "default":
        m.set_overlap(overlap)
    tag = f"forget[{fam},{overlap}]"
    for step, ref in zip(life.drive(fam, m), tr.refs64):
        life.compare_outputs(tag, step, ref)
        assert m.check_status() == 0, f"call {step.k}"
    notes = life.compare_state(tag, m, tr.s64, tr.s32)
    for n in notes:
        print("note:", n)
    assert not notes or fam in ("rlsb", "wide"), notes
    assert m.transition.shrink == float(np.float32(fc.LAM))


# ------------------------------------------------------------------ 2
def _fixture_model(vjf, z, info):
    m = vjf.VJF.make_model(info["dy"], info["dz"], info["du"], info["n"], info["hidden"], likelihood=info["lik"], lr=1e-4,
                           shrink=float(z["shrink"]))
    load_fixture_state(m, z, "s0")
    return m


def test_reference_fixture_step_by_step(vjf):
    """test_filter_trajectory_golden on the g10_forget0.9 trajectory, at its tolerances."""
    z, info, _ = gio.traj_case(fc.FIXTURES["f32"])
    model = _fixture_model(vjf, z, info)
    u, q = z["u"], None
    for t in range(info["T"]):
        q, loss, *comp = model.filter(torch.tensor(z["y"][t]), torch.tensor(u[t]), q, sgd=True, update=True, verbose=True,
                                      warm_up=info["warm_up"], eps=(torch.tensor(z["eps"][t, 0]), torch.tensor(z["eps"][t, 1])))
        close(q.mean, z["out.mu"][t], **POST)
        close(q.logvar, z["out.lv"][t], **POST)
        close(torch.stack([loss, *comp]), z["out.loss"][t], rtol=1e-6, atol=1e-6)
        close(model.transition.logvar, z["out.sigma"][t], rtol=0, atol=1e-6)
        close(model.likelihood.logvar, z["out.rho"][t], rtol=0, atol=1e-6)
        assert model.likelihood.n_sample == int(z["out.n_lik"][t])
        assert model.transition.n_sample == int(z["out.n_tr"][t])
        if f"s{t + 1}.w_mean" in z.files:
            state_close(model, z, prefix=f"s{t + 1}", rtol=5e-6, atol=1e-6, rls_rtol=5e-5, rls_atol=1e-6)
    state_close(model, z, prefix="sT", rtol=5e-6, atol=1e-6, rls_rtol=5e-4, rls_atol=5e-6)
    assert model.status() == 0


def test_reference_fixture_as_one_sequence(vjf):
    z, info, _ = gio.traj_case(fc.FIXTURES["f32"])
    model = _fixture_model(vjf, z, info)
    mu, lv, loss = model.filter_sequence(torch.tensor(z["y"]), torch.tensor(z["u"]), None, eps=torch.tensor(z["eps"]),
                                         sgd=True, update=True, warm_up=info["warm_up"])
    close(mu, z["out.mu"], **POST)
    close(lv, z["out.lv"], **POST)
    close(loss, z["out.loss"], rtol=1e-6, atol=1e-6)
    close(model.transition.logvar, z["out.sigma"][-1], rtol=0, atol=1e-6)
    close(model.likelihood.logvar, z["out.rho"][-1], rtol=0, atol=1e-6)
    assert model.transition.n_sample == int(z["out.n_tr"][-1])
    state_close(model, z, prefix="sT", rtol=5e-6, atol=1e-6, rls_rtol=5e-4, rls_atol=5e-6)
    assert model.status() == 0


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("fam", ["mega", "rlsb", "serial"])
def test_factor_one_is_the_code_without_it(vjf, fam):
    """Three models through the whole script: one never touched, one with 1.0 assigned, one whose slot holds 0 (every blob written
    before the slot had a meaning, every direct caller of the C ABI).  Outputs of every call bitwise equal; blobs bitwise equal --
    for the third, everywhere but the slot itself."""
    from vjf_amd import _native as N
    plain, one, zero = (life.make_model(vjf, fam) for _ in range(3))
    one.transition.shrink = 1.0
    zero._scalars[N.SC_SHRINK] = 0.0
    for a, b, c in zip(life.drive(fam, plain), life.drive(fam, one), life.drive(fam, zero)):
        _same_bits(f"one[{fam}]", a.k, plain, one, a.out, b.out)
        for name, x, y in zip(("mean", "logvar", "losses"), a.out, c.out):
            assert torch.equal(x, y), f"zero[{fam}]: call {a.k}: {name}"
        # (the round trip before call 7 reads the 0 as 1 and writes that; until then nobody writes the slot)
        assert float(zero._scalars[N.SC_SHRINK]) == (0.0 if a.k < 7 else 1.0), f"call {a.k}"
        assert torch.equal(_blob_without_factor(plain), _blob_without_factor(zero)), f"zero[{fam}]: call {a.k}: {life.blob_diff(plain, zero)}"
        assert plain.check_status() == 0 and one.check_status() == 0 and zero.check_status() == 0


# ------------------------------------------------------------------ 4
NO_RLS = {"warm_up": life.WARM, "no_update": life.SGD_ONLY, "infer": life.INFER}


@pytest.mark.parametrize("fam", ["mega", "rlsb"])
@pytest.mark.parametrize("flags", list(NO_RLS))
def test_no_update_no_effect(vjf, fam, flags):
    """A sequence and a single step without an RLS update at shrink = 0.5: the outputs and the blob (the factor's own slot aside)
    are bitwise those of shrink = 1 -- in particular P is not touched at all."""
    f = life.FAMILIES[fam]
    a, b = life.make_model(vjf, fam), life.make_model(vjf, fam)
    b.transition.shrink = 0.5
    p0 = a.transition.velocity.w_precision.clone()
    y, u, eps = life.inputs(fam)[0]                                          # 3 steps, 64 trials
    for m in (a, b):
        m.filter_sequence(y, u, None, eps=eps, **NO_RLS[flags])
        m.filter(y[0], None if u is None else u[0], None, eps=(eps[0, 0], eps[0, 1]), **NO_RLS[flags])
    oa = a.filter_sequence(y, u, None, eps=eps, **NO_RLS[flags])
    ob = b.filter_sequence(y, u, None, eps=eps, **NO_RLS[flags])
    for name, x, yv in zip(("mean", "logvar", "losses"), oa, ob):
        assert torch.equal(x, yv), f"{fam} {flags}: {name}"
    assert torch.equal(_blob_without_factor(a), _blob_without_factor(b)), life.blob_diff(a, b)
    assert torch.equal(b.transition.velocity.w_precision, p0)
    assert b.transition.shrink == 0.5 and a.check_status() == 0 and b.check_status() == 0
    assert f["n"] == p0.shape[0]


# ------------------------------------------------------------------ 5
def test_factor_changed_between_calls(vjf, monkeypatch):
    """One context on the one-launch route, three sequences with shrink = 1, 0.9, 1: the context handle stays, the write is ordered
    like the learning rates' (no synchronisation here), and every call matches the oracle driven the same way."""
    fam = "mega"
    m = life.make_model(vjf, fam)
    p = fc.pin(monkeypatch, 1.0)
    s64, s32 = load_oracle_state(m, np.float64), load_oracle_state(m, np.float32)
    ins = [life.inputs(fam)[i] for i in (1, 5, 7)]                            # three times 2 steps on 64 trials
    ctx = None
    for k, (lam, (y, u, eps)) in enumerate(zip((1.0, fc.LAM, 1.0), ins), 1):
        m.transition.shrink = lam
        p.lam = lam
        out = m.filter_sequence(y, u, None, eps=eps, **life.TR)
        assert m.route() == "one-launch"
        ctx = ctx or m._ctx.value
        assert m._ctx.value == ctx, f"call {k}: the context was re-created"
        refs = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for s in (s64, s32):
                refs.append(orc.filter_sequence(s, y.numpy(), u.numpy(), eps.numpy(), **life.TR))
        life.compare_outputs("between calls", life.Step(k, None, 64, out, refs), refs[0])
        assert m.check_status() == 0
    assert p.failed == 0
    notes = life.compare_state("between calls", m, s64, s32)
    assert not notes, notes


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("n_rbf,bad_from", fc.FAIL_SHAPES)
def test_failed_factorisation_takes_the_scaled_update_back(vjf, n_rbf, bad_from):
    """test_rls_failure_is_flagged_and_leaves_rls_state at shrink = 0.9: the status bit, W / w_chol / w_pchol bitwise kept, and P
    restored as (P' - G / v) / shrink -- within that test's tolerances divided by the factor (the same rounding errors carried
    through one division, whose own half-ulp the relative part covers)."""
    lam = fc.LAM
    torch.manual_seed(4)
    model = vjf.VJF.make_model(10, 3, 0, n_rbf, [8], likelihood="gaussian", shrink=lam)
    g = torch.Generator().manual_seed(5)
    T, B = 3, 64
    y, eps = torch.randn(T, B, 10, generator=g), torch.randn(T, 2, B, 3, generator=g)
    lr = model.transition.velocity
    with torch.no_grad():
        P = lr.w_precision.clone()
        P[bad_from:, bad_from:] -= 1e6 * torch.eye(n_rbf - bad_from, device=P.device)
        lr.w_precision.copy_(P)
    keep = {k: getattr(lr, k).clone() for k in ("w_mean", "w_chol", "w_pchol", "w_precision")}
    sig0 = model.transition.logvar.clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.filter(y[0], eps=(eps[0, 0], eps[0, 1]))
        assert model.status() & 8                                # VJF_STATUS_RLS_FAILED
        for k in ("w_mean", "w_chol", "w_pchol"):
            assert torch.equal(getattr(lr, k), keep[k]), k
        close(lr.w_precision, keep["w_precision"], rtol=1e-6 / lam, atol=1e-4 / lam)
        assert not torch.equal(model.transition.logvar, sig0)    # the state-noise estimate still moves (model.py:373-377)
        model.filter_sequence(y, eps=eps)
        assert model.status() & 8
        for k in ("w_mean", "w_chol", "w_pchol"):
            assert torch.equal(getattr(lr, k), keep[k]), k
        close(lr.w_precision, keep["w_precision"], rtol=1e-6 / lam, atol=5e-4 / lam)
        assert torch.isfinite(model.transition.logvar).all()


# ------------------------------------------------------------------ 7
def test_sharded_path_one_rank_with_forgetting(vjf, monkeypatch):
    """test_sharded_path_one_rank_nccl at shrink = 0.9: the local half, the all-reduce over RCCL and the global half run the same
    kernels and read the same scalar -- bitwise the plain path."""
    import os
    import torch.distributed as dist
    z, info, _ = gio.traj_case("g5_medium_gaussian_f32")

    def model():
        m = vjf.VJF.make_model(info["dy"], info["dz"], info["du"], info["n"], info["hidden"], likelihood=info["lik"], shrink=fc.LAM)
        load_fixture_state(m, z, "s0")
        return m
    m0, m1, m2 = model(), model(), model()
    m0.transition.shrink = 1.0
    y, eps = torch.tensor(z["y"][:4]), torch.tensor(z["eps"][:4])
    for m in (m0, m1):
        m.set_overlap(False)
    m0.filter_sequence(y, None, None, eps=eps)
    o1 = m1.filter_sequence(y, None, None, eps=eps)
    assert not torch.equal(m0.transition.velocity.w_precision, m1.transition.velocity.w_precision)    # (the factor acts)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29547")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    os.environ["VJF_FORCE_DIST"] = "1"
    try:
        o2 = m2.filter_sequence(y, None, None, eps=eps)
        q, loss = m2.filter(torch.tensor(z["y"][4]), eps=(torch.tensor(z["eps"][4, 0]), torch.tensor(z["eps"][4, 1])))
        torch.cuda.synchronize()
    finally:
        os.environ.pop("VJF_FORCE_DIST", None)
        dist.destroy_process_group()
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    q1, loss1 = m1.filter(torch.tensor(z["y"][4]), eps=(torch.tensor(z["eps"][4, 0]), torch.tensor(z["eps"][4, 1])))
    assert torch.equal(q.mean, q1.mean) and torch.equal(loss, loss1)
    assert torch.equal(m1._blob, m2._blob), life.blob_diff(m1, m2)


# ------------------------------------------------------------------ 8
def test_state_saved_mid_run_carries_the_factor(vjf, tmp_path):
    """A run at shrink = 0.9 saved after its first sequence and loaded into a fresh model (built without the argument): the factor
    arrives with the state and the second sequence is bitwise the uninterrupted run's."""
    fam = "mega"
    (y1, u1, e1), (y2, u2, e2) = life.inputs(fam)[1], life.inputs(fam)[5]
    a = life.make_model(vjf, fam)
    a.transition.shrink = fc.LAM
    a.filter_sequence(y1, u1, None, eps=e1, **life.TR)
    path = str(tmp_path / "mid.npz")
    a.save_state(path)
    b = life.make_model(vjf, fam)
    assert b.transition.shrink == 1.0
    b.load_state(path)
    assert b.transition.shrink == a.transition.shrink
    oa = a.filter_sequence(y2, u2, None, eps=e2, **life.TR)
    ob = b.filter_sequence(y2, u2, None, eps=e2, **life.TR)
    _same_bits("state i/o", 2, a, b, oa, ob)
    assert a.check_status() == 0 and b.check_status() == 0
    # (and the factor was in force in the second sequence: a twin that drops it after loading ends elsewhere)
    c = life.make_model(vjf, fam)
    c.load_state(path)
    c.transition.shrink = 1.0
    c.filter_sequence(y2, u2, None, eps=e2, **life.TR)
    assert not torch.equal(c.transition.velocity.w_precision, a.transition.velocity.w_precision)
