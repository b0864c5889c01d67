"""CPU side of the `score_forecast` tests: the host logic of vjf_amd/model.py (shapes and dtypes of the result, a Gaussian, a pair or
a tensor as q, a one-trial record, sst against numpy.var, the methods, the refusals) through a stand-in for vjf_kstep_score built on
tests/kstep_ref.py in fp64, and the planner, the scratch size and the return codes of the real library (host-only code: no GPU is
touched before a refusal)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fake_backend
from tests import kstep_ref as kr
from tests.fake_backend import _arr
from tests.test_smoother_host import SMALL, cpu_only, inputs, small_model
from vjf_amd import _native as N


def _arr64(p, n):
    return np.ctypeslib.as_array((C.c_double * int(n)).from_address(p.value))


class KstepLib(fake_backend.FakeLib):
    """FakeLib + vjf_kstep_score: kstep_ref.score in fp64 on the fp32 values it is handed, behind the entry point's own argument
    checks; the plan and the scratch size are the real library's.  Records every call's arguments in `calls`."""
    def __init__(self):
        super().__init__()
        self.calls = []

    def vjf_last_error(self):
        return self.err or self.real.vjf_last_error()

    def vjf_kstep_score_scratch_size(self, *a):
        return self.real.vjf_kstep_score_scratch_size(*a)

    def vjf_kstep_score_plan(self, *a):
        self.err = b""
        return self.real.vjf_kstep_score_plan(*a)

    def vjf_kstep_score(self, mu, y, u, cen, lw, w_mean, dec_W, dec_b, sse_x, base_x, sse_y, base_y, pred, scratch, T, B, K, n, d, dout,
                        dy, poisson, stream):
        null = lambda p: p is None or not p.value                                                 # noqa: E731
        if any(null(p) for p in (mu, cen, lw, w_mean, sse_x, base_x, scratch)) or (not null(y) and (null(sse_y) or null(base_y))):
            self.err = b"vjf_kstep_score: null tensor"
            return -1
        if (not null(y) and (null(dec_W) or null(dec_b))) or T < 1 or B < 1 or K < 1 or n < 1 or dout < 1 or d < dout:
            self.err = b"vjf_kstep_score: bad shape"
            return -20
        du = d - dout
        if du > 0 and null(u):
            self.err = b"vjf_kstep_score: u is required when d > dout"
            return -21
        f = lambda p, *shape: _arr(p, int(np.prod(shape))).reshape(shape).astype(np.float64)      # noqa: E731
        st = {"centroid": f(cen, n, d), "logwidth": f(lw, n), "w_mean": f(w_mean, n, dout)}
        Y = None
        if not null(y):
            st["dec_W"], st["dec_b"], Y = f(dec_W, dy, dout), f(dec_b, dy), f(y, T, B, dy)
        U = f(u, T, B, du) if du > 0 else None
        self.calls.append(dict(T=T, B=B, K=K, n=n, d=d, dout=dout, dy=dy if Y is not None else 0, poisson=poisson, mu=f(mu, T, B, dout), y=Y, u=U,
                               pred=not null(pred)))
        r = kr.score(st, f(mu, T, B, dout), Y, U, K, poisson=bool(poisson))
        _arr64(sse_x, (K + 1) * dout)[...] = r["sse_x"].ravel()
        _arr64(base_x, (K + 1) * dout)[...] = r["base_x"].ravel()
        if Y is not None:
            _arr64(sse_y, (K + 1) * dy)[...] = r["sse_y"].ravel()
            _arr64(base_y, (K + 1) * dy)[...] = r["base_y"].ravel()
        if not null(pred):
            _arr(pred, K * T * B * dout)[...] = r["pred"].ravel()
        return 0


@pytest.fixture
def fake():
    old = N._lib
    N._lib = KstepLib()
    yield N._lib
    N._lib = old


def obs(seed=4, T=SMALL["T"], B=SMALL["B"]):
    return torch.randn(T, B, SMALL["ydim"], generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------- the host logic
@cpu_only
def test_shapes_dtypes_methods_and_sst(fake):
    import vjf_amd
    c = SMALL
    T, B, d, dy, K = c["T"], c["B"], c["xdim"], c["ydim"], 4
    m = small_model()
    mu, lv, u = inputs()
    y = obs()
    out = m.score_forecast((mu, lv), y, u, K, return_pred=True)
    assert isinstance(out, vjf_amd.model.ForecastScore)
    assert out._fields == ("n", "sse_x", "base_x", "sse_y", "base_y", "sst_x", "sst_y", "pred", "kind") and out.kind == "gaussian"
    assert out.n.tolist() == [(T - h) * B for h in range(K + 1)] and out.n.dtype == torch.int64
    for t, dim in ((out.sse_x, d), (out.base_x, d), (out.sst_x, d), (out.sse_y, dy), (out.base_y, dy), (out.sst_y, dy)):
        assert t.shape == (K + 1, dim) and t.dtype == torch.float64
    assert out.pred.shape == (K, T, B, d) and out.pred.dtype == torch.float32
    call, = fake.calls
    assert (call["T"], call["B"], call["K"], call["n"], call["d"], call["dout"], call["dy"], call["poisson"]) == (T, B, K, c["n"], d + c["udim"], d, dy, 0)
    np.testing.assert_array_equal(call["mu"], mu.double().numpy())
    np.testing.assert_array_equal(call["u"], u.double().numpy())
    np.testing.assert_array_equal(call["y"], y.double().numpy())
    assert (out.sse_x[0] == 0).all() and torch.isnan(out.pred[K - 1, T - K:]).all() and not torch.isnan(out.pred[K - 1, :T - K]).any()
    # sst: numpy's variance of the valid target rows times their count
    for h in range(K + 1):
        np.testing.assert_allclose(out.sst_x[h].numpy(), mu[h:].double().numpy().reshape(-1, d).var(0) * (T - h) * B, rtol=1e-10)
        np.testing.assert_allclose(out.sst_y[h].numpy(), y[h:].double().numpy().reshape(-1, dy).var(0) * (T - h) * B, rtol=1e-10)
    # the methods
    np.testing.assert_allclose(out.r2_x().numpy(), 1 - out.sse_x.sum(1).numpy() / out.sst_x.sum(1).numpy())
    np.testing.assert_allclose(out.r2_y().numpy(), 1 - out.sse_y.sum(1).numpy() / out.sst_y.sum(1).numpy())
    np.testing.assert_allclose(out.skill_x()[1:].numpy(), 1 - out.sse_x.sum(1)[1:].numpy() / out.base_x.sum(1)[1:].numpy())
    np.testing.assert_allclose(out.skill_y().numpy(), 1 - out.sse_y.sum(1).numpy() / out.base_y.sum(1).numpy())
    np.testing.assert_allclose(out.mse_x().numpy(), out.sse_x.sum(1).numpy() / (out.n.numpy() * d))
    np.testing.assert_allclose(out.mse_y().numpy(), out.sse_y.sum(1).numpy() / (out.n.numpy() * dy))
    assert out.r2_x()[0] == 1 and out.r2_x().shape == (K + 1,)
    # defaults: n_step 8, no pred; the transition's own method scores x alone
    out = m.score_forecast((mu, lv), y, u)
    assert fake.calls[-1]["K"] == 8 and out.pred is None and not fake.calls[-1]["pred"]
    assert out.n.tolist()[T:] == [0] * (9 - T) and (out.sse_x[T:] == 0).all() and torch.isnan(out.mse_x()[T:]).all()
    tr = m.transition.score_forecast(mu, u, K)
    assert tr.sse_y is None and tr.base_y is None and tr.sst_y is None and tr.kind is None and fake.calls[-1]["dy"] == 0
    with pytest.raises(ValueError, match="y"):
        tr.skill_y()
    with pytest.raises(ValueError):
        tr.r2_y()
    assert torch.equal(tr.sse_x, m.score_forecast(mu, None, u, K).sse_x)


@cpu_only
def test_the_forms_of_q_and_a_one_trial_record(fake):
    import vjf_amd
    c = SMALL
    m = small_model()
    mu, lv, u = inputs()
    y = obs()
    a = m.score_forecast(vjf_amd.Gaussian(mu, lv), y, u, 3)
    b = m.score_forecast((mu, lv), y, u, 3)
    t = m.score_forecast(mu.double(), y.double(), u.double(), 3)
    for k in ("sse_x", "base_x", "sse_y", "base_y", "sst_x", "sst_y"):
        assert torch.equal(getattr(a, k), getattr(b, k)) and torch.equal(getattr(a, k), getattr(t, k))
    one = m.score_forecast(mu[:, 2], y[:, 2], u[:, 2], 3, return_pred=True)
    assert fake.calls[-1]["B"] == 1 and one.pred.shape == (3, c["T"], 1, c["xdim"]) and one.n.tolist() == [6, 5, 4, 3]
    whole = m.score_forecast(mu, y, u, 3, return_pred=True)
    np.testing.assert_array_equal(one.pred[:, :, 0].numpy(), whole.pred[:, :, 2].numpy())      # (NaN in the same places)
    m0 = small_model(udim=0)
    assert m0.score_forecast(mu, y, n_step=2).sse_x.shape == (3, c["xdim"]) and fake.calls[-1]["u"] is None


@cpu_only
def test_poisson_kind(fake):
    import vjf_amd
    c = SMALL
    torch.manual_seed(1)
    m = vjf_amd.VJF.make_model(c["ydim"], c["xdim"], 0, c["n"], [4], likelihood="poisson")
    mu, lv, _ = inputs(udim=0)
    y = torch.poisson(torch.full((c["T"], c["B"], c["ydim"]), 2.0), generator=torch.Generator().manual_seed(2))
    out = m.score_forecast((mu, lv), y, n_step=3)
    assert out.kind == "poisson" and fake.calls[-1]["poisson"] == 1 and out.sst_y is None and out.sse_y.shape == (4, c["ydim"])
    with pytest.raises(ValueError, match="Poisson"):
        out.r2_y()
    assert out.skill_y().shape == (4,) and out.mse_y().shape == (4,)


@cpu_only
def test_assertions_and_refusals_of_the_python_surface(fake):
    import vjf_amd
    m = small_model()
    mu, lv, u = inputs()
    y = obs()
    for K in (0, -2):
        with pytest.raises(ValueError, match="n_step"):
            m.score_forecast(mu, y, u, K)
    with pytest.raises(TypeError):
        m.score_forecast(mu, y)                            # u missing with udim > 0
    with pytest.raises(AssertionError, match="rows"):
        m.score_forecast(mu, y, u[:-1])
    with pytest.raises(AssertionError, match="y is"):
        m.score_forecast(mu, y[:-1], u)
    with pytest.raises(AssertionError, match="columns"):
        m.score_forecast(mu[..., :-1], y, u)
    assert fake.calls == []
    big = vjf_amd.VJF.make_model(5, 3, 0, 3000, [4], likelihood="gaussian")      # beyond one workgroup's LDS: the real plan refuses
    with pytest.raises(NotImplementedError, match="LDS"):
        big.score_forecast(torch.zeros(4, 2, 3), n_step=2)
    assert fake.calls == []
    fake.vjf_kstep_score = lambda *a: (setattr(fake, "err", b"vjf_kstep_score: refused") or -20)
    with pytest.raises(N.VjfError, match="vjf_kstep_score: refused"):
        m.score_forecast(mu, y, u, 2)


@cpu_only
def test_no_write_to_the_model_or_the_inputs(fake):
    m = small_model()
    mu, lv, u = inputs()
    y = obs()
    before = {k: v.detach().clone() for k, v in m.state_dict().items() if isinstance(v, torch.Tensor)}
    rng = torch.get_rng_state()
    muc, yc, uc = mu.clone(), y.clone(), u.clone()
    m.score_forecast((mu, lv), y, u, 3, return_pred=True)
    after = m.state_dict()
    assert all(torch.equal(v, after[k]) for k, v in before.items()) and torch.equal(rng, torch.get_rng_state())
    assert torch.equal(mu, muc) and torch.equal(y, yc) and torch.equal(u, uc)


# ---------------------------------------------------------------------------------------------------- the real library's host code
def test_return_codes_of_the_entry_point():
    """Every refusal comes before the first launch, so the real entry point can be asked without a GPU: it reads no tensor."""
    L = N.lib()
    buf = np.zeros(64, np.float64)
    p = C.c_void_p(buf.ctypes.data)

    def call(mu=p, y=p, u=p, cen=p, dec_W=p, dec_b=p, sse_x=p, sse_y=p, scratch=p, T=4, B=2, K=3, n=9, d=5, dout=3, dy=4):
        return L.vjf_kstep_score(mu, y, u, cen, p, p, dec_W, dec_b, sse_x, p, sse_y, p, None, scratch, T, B, K, n, d, dout, dy, 0, None)
    for rc, kw in ((-1, dict(mu=None)), (-1, dict(cen=None)), (-1, dict(sse_x=None)), (-1, dict(sse_y=None)), (-1, dict(scratch=None)),
                   (-20, dict(T=0)), (-20, dict(K=0)), (-20, dict(B=0)), (-20, dict(n=0)), (-20, dict(d=2)), (-20, dict(dout=0)),
                   (-20, dict(dy=0)), (-20, dict(dec_W=None)), (-20, dict(dec_b=None)), (-21, dict(u=None)),
                   (-11, dict(n=3000, d=3, dout=3)), (-11, dict(n=2000, d=64, dout=64, dy=200))):
        assert call(**kw) == rc, kw
        assert b"vjf_kstep_score" in L.vjf_last_error()
    assert call(n=3000, d=3, dout=3) == -11 and b"LDS" in L.vjf_last_error() and b"162816" in L.vjf_last_error()


def plan(T, B, K, n, d, dout, dy):
    lds, tiles, per, forms = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1), C.c_int32(-1)
    rc = N.lib().vjf_kstep_score_plan(T, B, K, n, d, dout, dy, C.byref(lds), C.byref(tiles), C.byref(per), C.byref(forms))
    return rc, lds.value, tiles.value, per.value, forms.value


def scratch(T, B, K, dout, dy):
    b = C.c_int64(-1)
    assert N.lib().vjf_kstep_score_scratch_size(T, B, K, dout, dy, C.byref(b)) == 0
    return b.value


GRID = [(12, 37, 8, 20, 3, 3, 7), (10, 33, 8, 200, 10, 10, 50), (10, 18, 8, 300, 5, 5, 7), (200, 4096, 16, 200, 10, 10, 50),
        (10000, 1, 32, 20, 3, 3, 10), (40, 1, 8, 20, 3, 3, 0), (5, 37, 8, 37, 7, 5, 21), (3000, 4096, 64, 256, 32, 24, 300), (1, 1, 1, 1, 1, 1, 0)]
CAP = 32 << 20


def test_the_plan_and_the_scratch_size(monkeypatch):
    for v in ("VJF_KS_CHUNK", "VJF_FC_CENTROID_LDS", "VJF_FC_LOOKAHEAD"):
        monkeypatch.delenv(v, raising=False)
    for T, B, K, n, d, dout, dy in GRID:
        rc, lds, tiles, per, forms = plan(T, B, K, n, d, dout, dy)
        elems = (K + 1) * (2 * dout + 2 * dy)
        assert rc == 0 and tiles == -(-T * B // 16) and 1 <= per <= tiles and 0 < lds <= 159 * 1024, (T, B, K, n, d, dout, dy)
        assert per * elems * 4 <= CAP or per == 1, "the partials of a chunk stay within the cap"
        assert per == tiles or (per + 1) * elems * 4 > CAP, "and a chunk is as large as the cap allows"
        chunks = [(t0, min(per, tiles - t0)) for t0 in range(0, tiles, per)]
        assert sum(c for _, c in chunks) == tiles and all(a + c == b for (a, c), (b, _) in zip(chunks, chunks[1:])), "every tile exactly once"
        need = scratch(T, B, K, dout, dy)
        assert need >= elems * 8 + per * elems * 4 and need <= elems * 8 + 256 + max(CAP, elems * 4) + 256
        # LDS: the x step's buffers, xh_0, two y-hat blocks and, by the forms, the centroids and the decoder
        doutp, dyp = -(-dout // 16) * 16, -(-dy // 16) * 16
        floats = 17 * (n + d + 4 * doutp) + n + 17 * dout + 2 * 17 * dyp + (n * d if forms & 1 else 0) + (dout * (-(-dy // 32) * 32 + 16) if forms & 4 else 0)
        assert lds == 4 * floats, (T, B, K, n, d, dout, dy, forms)
        assert not (forms & 2) or (forms & 1 and n <= 256 and dout <= 32)
        assert not (forms & 4) or dy > 0
    assert plan(10, 33, 8, 200, 10, 10, 50)[4] == 7 and plan(10, 18, 8, 300, 5, 5, 7)[4] == 5
    # the override: monotone, never above what the cap allows, 0 is "not set"
    free = plan(200, 4096, 16, 200, 10, 10, 50)[3]
    last = 0
    for forced in (1, 3, 100, free - 1, free, free + 1, 10 ** 6):
        monkeypatch.setenv("VJF_KS_CHUNK", str(forced))
        per = plan(200, 4096, 16, 200, 10, 10, 50)[3]
        assert per == min(forced, free) and per >= last
        last = per
        assert scratch(200, 4096, 16, 10, 50) >= 17 * 120 * 8 + free * 17 * 120 * 4, "the scratch size does not shrink with the override"
    monkeypatch.setenv("VJF_KS_CHUNK", "0")
    assert plan(200, 4096, 16, 200, 10, 10, 50)[3] == free
    monkeypatch.delenv("VJF_KS_CHUNK")
    monkeypatch.setenv("VJF_FC_CENTROID_LDS", "0")
    assert plan(10, 33, 8, 200, 10, 10, 50)[4] == 0
    monkeypatch.delenv("VJF_FC_CENTROID_LDS")
    monkeypatch.setenv("VJF_FC_LOOKAHEAD", "0")
    assert plan(10, 33, 8, 200, 10, 10, 50)[4] == 5
    monkeypatch.delenv("VJF_FC_LOOKAHEAD")
    # refusals
    L = N.lib()
    for bad in ((0, 1, 1, 1, 1, 1, 0), (1, 0, 1, 1, 1, 1, 0), (1, 1, 0, 1, 1, 1, 0), (1, 1, 1, 0, 1, 1, 0), (1, 1, 1, 1, 1, 2, 0), (1, 1, 1, 1, 1, 1, -1)):
        assert plan(*bad)[0] == -20
    assert plan(12, 37, 8, 3000, 3, 3, 7)[0] == -11 and b"LDS" in L.vjf_last_error() and b"vjf_kstep_score_plan" in L.vjf_last_error()
    assert L.vjf_kstep_score_plan(12, 37, 8, 20, 3, 3, 7, None, None, None, None) == 0
