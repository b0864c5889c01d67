"""CPU side of the forgetting-factor tests (tests/forget_cases.py): the oracle with its `rls` pinned to 0.9 against the two
trajectories captured from the reference (tests/golden/make_golden_forget.py), and what the host mirror owns of the factor on the
oracle-backed stand-in for the C ABI (tests/fake_backend.py): the scalar's slot in the blob, its life across context growth and
the state round trips, its validation, and the operator-by-operator `RBFDS.update`."""
import numpy as np
import pytest
import torch

from oracle import vjf_oracle as orc
from tests import fake_backend
from tests import forget_cases as fc
from tests import goldenio as gio
from tests import lifetime as life
from vjf_amd import _native as N

cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="the stand-in backend works on CPU tensors")


def close(a, b, **kw):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), **kw)


@pytest.fixture
def fake():
    undo = fake_backend.install()
    yield N._lib
    undo()


# ------------------------------------------------------------------ the oracle against the reference
def test_fixtures_are_the_g5_shape_and_really_forget():
    """The pair has the shapes of g5_gaussian_du2_wu0_* and starts from the same state (same seed); its final precision matrix is
    NOT the one of the run without forgetting -- a fixture that equalled the g5 one would pin nothing."""
    for tag, name in fc.FIXTURES.items():
        z, info, _ = gio.traj_case(name)
        z5, info5, _ = gio.traj_case(f"g5_gaussian_du2_wu0_{tag}")
        assert info == info5
        assert float(z["shrink"]) == fc.LAM
        close(z["s0.w_precision"], z5["s0.w_precision"], rtol=0, atol=0)
        close(z["y"], z5["y"], rtol=0, atol=0)
        assert np.abs(z["sT.w_precision"] - z5["sT.w_precision"]).max() > 0.1 * np.abs(z5["sT.w_precision"]).max()


def test_forget_trajectory_f64(monkeypatch):
    """test_g5_trajectory_f64's comparisons and tolerances."""
    fc.pin(monkeypatch)
    z, info, s, outs = fc.run_traj(fc.FIXTURES["f64"])
    for t, o in enumerate(outs):
        close(o.mu_t, z["out.mu"][t], rtol=1e-8, atol=1e-10)
        close(o.lv_t, z["out.lv"][t], rtol=1e-8, atol=1e-10)
        close([o.loss, o.recon, o.dyn, o.entropy], z["out.loss"][t], rtol=1e-9, atol=1e-10)
        close(o.rho, z["out.rho"][t], rtol=1e-9, atol=1e-10)
        close(o.sigma, z["out.sigma"][t], rtol=1e-8, atol=1e-10)
        assert o.n_lik == int(z["out.n_lik"][t]) and o.n_tr == int(z["out.n_tr"][t])
        if hasattr(o, "state"):
            for k, v in gio.state_arrays(o.state).items():
                close(v, z[f"s{t + 1}.{k}"], rtol=1e-7, atol=1e-10)
    for k, v in gio.state_arrays(s).items():
        close(v, z[f"sT.{k}"], rtol=1e-6, atol=1e-9)


def test_forget_trajectory_f32(monkeypatch):
    """test_g5_trajectory_f32's comparisons and tolerances."""
    fc.pin(monkeypatch)
    z, info, s, outs = fc.run_traj(fc.FIXTURES["f32"])
    assert s.dtype == np.float32
    for t, o in enumerate(outs):
        close(o.mu_t, z["out.mu"][t], rtol=2e-5, atol=2e-5)
        close(o.lv_t, z["out.lv"][t], rtol=2e-5, atol=2e-5)
        close([o.loss, o.recon, o.dyn, o.entropy], z["out.loss"][t], rtol=2e-5, atol=2e-5)
        close(o.sigma, z["out.sigma"][t], rtol=0, atol=2e-5)
        close(o.rho, z["out.rho"][t], rtol=0, atol=2e-5)
    close(s.w_mean, z["sT.w_mean"], rtol=1e-3, atol=2e-5)
    close(s.w_precision, z["sT.w_precision"], rtol=1e-4, atol=1e-4)
    close(s.w_chol, z["sT.w_chol"], rtol=1e-3, atol=2e-5)
    for k in ("mean_W", "lv_W", "lv_b", "dec_W", "dec_b", "rec_W0", "rec_b0"):
        close(gio.state_arrays(s)[k], z[f"sT.{k}"], rtol=1e-4, atol=1e-5)


def test_unpinned_oracle_misses_the_fixture():
    """The other direction: the oracle as it stands (factor 1) is far from the fixture, so the two tests above test the factor."""
    z, info, s, outs = fc.run_traj(fc.FIXTURES["f64"])
    assert np.abs(s.w_precision - z["sT.w_precision"]).max() > 0.1 * np.abs(z["sT.w_precision"]).max()


# ------------------------------------------------------------------ the host mirror
def _slot9(m):
    n, off, size = N.state_layout(m._config(1))
    return m._blob[off[N.SLOT_SCALARS] + 9]


@cpu_only
def test_scalar_lands_in_slot_9(fake):
    import vjf_amd
    assert N.SC_SHRINK == 9 and N.N_SCALARS == 16
    m = life.make_model(vjf_amd, "mega")
    assert m.transition.shrink == 1.0 and float(_slot9(m)) == 1.0            # the default, written at adoption
    m.transition.shrink = 0.9
    assert float(_slot9(m)) == float(np.float32(0.9)) and m.transition.shrink == float(np.float32(0.9))
    others = m._scalars.clone()
    m.transition.shrink = 0.98
    changed = (m._scalars != others).nonzero().flatten().tolist()
    assert changed == [N.SC_SHRINK]
    # a blob from before the slot had a meaning holds 0 there: it reads as 1
    m._scalars[N.SC_SHRINK] = 0.0
    assert m.transition.shrink == 1.0


@cpu_only
def test_constructor_arguments_reach_the_blob(fake):
    """`RBFDS(..., shrink=)` set before adoption is carried into the blob; `VJF(..., shrink=)` / `make_model(..., shrink=)` set it
    on the transition; without the argument the transition keeps its own."""
    import vjf_amd
    from vjf_amd.likelihood import GaussianLikelihood
    from vjf_amd.model import RBFDS, VJF
    from vjf_amd.recognition import Recognition
    tr = RBFDS(16, 3, 0, shrink=0.95)
    assert tr.shrink == 0.95                                                # no owner yet: a plain attribute
    m = VJF(10, 3, GaussianLikelihood(), tr, Recognition(10, 3, 0, [8]))
    assert float(_slot9(m)) == float(np.float32(0.95)) and tr.shrink == float(np.float32(0.95))
    m = vjf_amd.VJF.make_model(10, 3, 0, 16, [8], likelihood="gaussian", shrink=0.9)
    assert float(_slot9(m)) == float(np.float32(0.9))
    m = VJF(10, 3, GaussianLikelihood(), RBFDS(16, 3, 0, shrink=0.95), Recognition(10, 3, 0, [8]), shrink=0.5)
    assert float(_slot9(m)) == 0.5
    m = vjf_amd.VJF.make_model(10, 3, 0, 16, [8], likelihood="gaussian")
    assert float(_slot9(m)) == 1.0


@cpu_only
def test_scalar_survives_growth_and_the_state_round_trip(fake):
    """Setting the factor re-creates nothing; growth re-creates the context on the same blob and the factor is still there;
    `set_state(get_state())` changes nothing but the two words it clears."""
    import vjf_amd
    m = life.make_model(vjf_amd, "mega")
    (y1, u1, e1), _, _, _, (y5, u5, e5) = life.inputs("mega")[:5]
    m.filter_sequence(y1, u1, None, eps=e1, **life.TR)
    ctx = fake.ctxs[m._ctx.value]                                           # (the object: the stand-in's handles are ids)
    m.transition.shrink = 0.9
    m.filter_sequence(y1, u1, None, eps=e1, **life.TR)
    assert fake.ctxs[m._ctx.value] is ctx and m._ctx_batch == 64            # the context is not re-created
    m.filter_sequence(y5, u5, None, eps=e5, **life.TR)
    assert m._ctx_batch == 150 and fake.ctxs[m._ctx.value] is not ctx       # grown
    assert float(_slot9(m)) == float(np.float32(0.9))
    before = m._blob.clone()
    m.set_state(m.get_state())
    base = (m._scalars.data_ptr() - m._blob.data_ptr()) // 4
    changed = (m._blob != before).nonzero().flatten().tolist()
    assert set(changed) <= {base + N.SC_STATUS, base + N.SC_TRI_CLEAN}, changed
    assert float(_slot9(m)) == float(np.float32(0.9))


@cpu_only
def test_save_and_load_into_a_new_model(fake, tmp_path):
    import vjf_amd
    a = life.make_model(vjf_amd, "mega")
    a.transition.shrink = 0.9
    st = a.get_state()
    assert st["transition.shrink"].dtype == np.float64 and float(st["transition.shrink"]) == float(np.float32(0.9))
    path = str(tmp_path / "state.npz")
    a.save_state(path)
    b = life.make_model(vjf_amd, "mega")
    assert b.transition.shrink == 1.0
    b.load_state(path)
    assert b.transition.shrink == a.transition.shrink and torch.equal(_slot9(b), _slot9(a))
    with np.load(path) as z:
        assert "transition.shrink" in z.files


@cpu_only
def test_state_from_before_the_key_loads_as_one(fake):
    """A state dict without the key: what every state saved before the factor existed is, and what `get_state` still writes at
    shrink = 1 (the key is left out there, so such a state keeps the old format)."""
    import vjf_amd
    a = life.make_model(vjf_amd, "mega")
    old = a.get_state()
    assert "transition.shrink" not in old
    b = life.make_model(vjf_amd, "mega")
    b.transition.shrink = 0.9
    b.set_state(old)
    assert b.transition.shrink == 1.0 and float(_slot9(b)) == 1.0


@cpu_only
@pytest.mark.parametrize("bad", [0.0, -0.1, 1.0001, 2.0, float("nan"), float("inf")])
def test_bad_values_raise(fake, bad):
    import vjf_amd
    from vjf_amd.model import RBFDS
    with pytest.raises(ValueError, match="shrink"):
        RBFDS(16, 3, 0, shrink=bad)
    tr = RBFDS(16, 3, 0)
    with pytest.raises(ValueError, match="shrink"):
        tr.shrink = bad
    assert tr.shrink == 1.0
    with pytest.raises(ValueError, match="shrink"):
        vjf_amd.VJF.make_model(10, 3, 0, 16, [8], likelihood="gaussian", shrink=bad)
    m = vjf_amd.VJF.make_model(10, 3, 0, 16, [8], likelihood="gaussian", shrink=0.9)
    with pytest.raises(ValueError, match="shrink"):
        m.transition.shrink = bad
    assert float(_slot9(m)) == float(np.float32(0.9))                       # a refused value leaves the blob alone
    st = m.get_state()
    st["transition.shrink"] = np.float64(bad)
    with pytest.raises(ValueError, match="shrink"):
        m.set_state(st)


@cpu_only
@pytest.mark.parametrize("owned", [False, True])
def test_update_passes_the_factor_to_rls(fake, owned):
    """`RBFDS.update` (operator by operator) with shrink = 0.9 against the oracle's `rls(..., 0.9)` on the same statistics, alone
    and as a model's transition (where the factor is read back from the blob).  The stand-in's `vjf_blr_rls` honours the argument it
    is given, so a factor dropped on the way would give the shrink = 1 result, which is checked to be far away."""
    import vjf_amd
    from vjf_amd.model import RBFDS
    n, dz, du, B = 16, 3, 2, 40
    torch.manual_seed(3)
    if owned:
        m = vjf_amd.VJF.make_model(10, dz, du, n, [8], likelihood="gaussian", shrink=fc.LAM)
        tr = m.transition
    else:
        tr = RBFDS(n, dz, du, shrink=fc.LAM)
    g = torch.Generator().manual_seed(4)
    xs, xt, ut = torch.randn(B, dz, generator=g), torch.randn(B, dz, generator=g), torch.randn(B, du, generator=g)
    vel = tr.velocity
    with torch.no_grad():
        vel.w_precision.copy_(torch.eye(n) * 3.0)                            # (a P that the factor visibly scales)
        vel.w_mean.copy_(torch.randn(n, dz, generator=g) * 0.1)

    def oracle(lam):
        s = orc.OracleState(1, dz, du, n, (1,), orc.GAUSSIAN)
        s.centroid, s.logwidth = vel.feature.centroid.numpy().astype(np.float64), vel.feature.logwidth.numpy().astype(np.float64)
        s.w_mean, s.w_precision = vel.w_mean.numpy().astype(np.float64), vel.w_precision.numpy().astype(np.float64)
        feat = orc.rbf(np.concatenate([xs.numpy(), ut.numpy()], 1).astype(np.float64), s.centroid, np.exp(s.logwidth))
        assert orc.rls(s, feat, (xt - xs).numpy().astype(np.float64), float(np.exp(np.float32(tr.logvar.item()))), lam) == 0
        return s
    want, plain = oracle(float(np.float32(fc.LAM))), oracle(1.0)
    tr.update(xt, xs, ut)
    for k in ("w_precision", "w_pchol", "w_mean", "w_chol"):
        close(getattr(vel, k).numpy(), getattr(want, k), rtol=2e-6, atol=1e-6, err_msg=k)
    assert np.abs(vel.w_precision.numpy() - plain.w_precision).max() > 0.25
