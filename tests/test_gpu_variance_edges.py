"""The trial role's variance and mean products (vjf_mega_common.h: mg_var2, mg_mma2_mm16) split their k range in the training kernel
into full steps -- no clamp, no mask, B operands at immediate LDS offsets -- and at most one partial step; mg_varN (the moments role),
the kernels without an RLS update and the L2-fed mg_mma2 keep every step clamped and masked.  Three steps on the one-launch route at
the feature counts where that split or an offset can go wrong, against the fp64 oracle at the tolerances of
test_gpu_block_layout.py, and stepwise `filter` against `filter_sequence` bit for bit, the state blob included.
The three stepwise calls are three launches: the first walks the dense square of L^-1 (a fresh model: triangle flag clear), the
later ones the triangle; the one `filter_sequence` launch walks all three steps dense.  All tests need a real MI355X:  pytest -m gpu.

    n = 4     only a partial step                      n = 72    the second batch of 64 k is nothing but a tail
    n = 16    one full 16-k step, no partial one       n = 100   config A          n = 200   config B
    n = 20    one full step and a 4-wide tail          n = 208   13 full row tiles
    n = 64    exactly one batch                        n = 224   the route's largest: 14 tiles, second-round tiles on six wavefronts
d_z in {3, 10, 16}: the mean product's K slices (empty ones at small n); B in {8, 40}: one ragged tile / two tiles, the second
with 8 trials; B = 8192: two tiles per trial workgroup.
"""
import numpy as np
import pytest
import torch

from oracle import vjf_oracle as orc
from tests.helpers import load_oracle_state, state_close
from tests.test_gpu_parity import close

pytestmark = pytest.mark.gpu

T = 3
TRAIN = dict(sgd=True, update=True, warm_up=False)
LITE = {"warmup": dict(sgd=True, update=True, warm_up=True), "sgd-only": dict(sgd=True, update=False, warm_up=False)}
SHAPES = [(n, dz, B) for n in (4, 16, 20, 64, 72, 100, 200, 208, 224) for dz in (3, 10, 16) for B in (8, 40)]


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


def _fresh(vjf, dy, dz, n, hidden, lik):
    torch.manual_seed(41)
    return vjf.VJF.make_model(dy, dz, 0, n, hidden, likelihood=lik, lr=1e-3)


def _inputs(dy, dz, B, lik):
    g = torch.Generator().manual_seed(43)
    if lik == "poisson":
        y = torch.poisson(torch.exp(0.5 * torch.randn(T, B, dy, generator=g) - 0.5), generator=g)
    else:
        y = torch.randn(T, B, dy, generator=g)
    return y, torch.randn(T, 2, B, dz, generator=g)


def _three_steps(vjf, n, dz, B, kw, dy=10, hidden=(16,), lik="gaussian"):
    hidden = list(hidden)
    y, eps = _inputs(dy, dz, B, lik)
    m = _fresh(vjf, dy, dz, n, hidden, lik)
    s = load_oracle_state(m, np.float64)
    # stepwise: three launches, every step against the oracle run with the same flags
    q, mus, lvs, losses = None, [], [], []
    mu_o = lv_o = None
    for t in range(T):
        q, loss, *comp = m.filter(y[t], None, q, verbose=True, eps=(eps[t, 0], eps[t, 1]), **kw)
        o = orc.filter_step(s, y[t].numpy().astype(np.float64), None, mu_o, lv_o, eps[t, 0].numpy().astype(np.float64),
                            eps[t, 1].numpy().astype(np.float64), **kw)
        mu_o, lv_o = o.mu_t, o.lv_t
        close(q.mean, o.mu_t, rtol=2e-6, atol=2e-6)
        close(q.logvar, o.lv_t, rtol=2e-6, atol=2e-6)
        close(torch.stack([loss, *comp]), [o.loss, o.recon, o.dyn, o.entropy], rtol=2e-5, atol=2e-5)
        close(m.transition.logvar, s.tr_logvar, rtol=0, atol=2e-5)
        mus.append(q.mean), lvs.append(q.logvar), losses.append(torch.stack([loss, *comp]))
    assert m.route(**kw) == "one-launch"
    state_close(m, s, rtol=5e-6, atol=1e-6, rls_rtol=3e-3, rls_atol=3e-5)
    assert m.status() == 0
    # the same steps as one launch: bit for bit, the whole state too
    m2 = _fresh(vjf, dy, dz, n, hidden, lik)
    mu2, lv2, loss2 = m2.filter_sequence(y, None, None, eps=eps, **kw)
    assert m2.route(**kw) == "one-launch"
    assert torch.equal(torch.stack(mus), mu2) and torch.equal(torch.stack(lvs), lv2) and torch.equal(torch.stack(losses), loss2)
    assert torch.equal(m._blob, m2._blob)
    assert m2.status() == 0


@pytest.mark.parametrize("n,dz,B", SHAPES, ids=lambda v: str(v))
def test_training_steps(vjf, n, dz, B):
    _three_steps(vjf, n, dz, B, TRAIN)


def test_two_tiles_per_trial_workgroup(vjf):
    """B = 8192: 256 tiles on 128 trial workgroups."""
    _three_steps(vjf, 200, 10, 8192, TRAIN)


@pytest.mark.parametrize("B", [40, 8192])
@pytest.mark.parametrize("n", [20, 200, 224])
@pytest.mark.parametrize("flags", sorted(LITE))
def test_launches_without_an_rls_update(vjf, flags, n, B):
    """vjf_mega_lite_kernel: the moments role's one-tile and two-tile passes through mg_varN."""
    _three_steps(vjf, n, 10, B, LITE[flags])


def test_products_fed_from_l2_config_c(vjf):
    """Config C's dimensions: the parameters do not fit LDS, every layer product runs through mg_mma2."""
    _three_steps(vjf, 200, 10, 40, TRAIN, dy=200, hidden=(128,), lik="poisson")


def test_products_fed_from_l2_ragged(vjf):
    """Ragged M and K in mg_mma2: d_y = 203, d_z = 7, hidden [120, 36], n = 100."""
    _three_steps(vjf, 100, 7, 40, TRAIN, dy=203, hidden=(120, 36), lik="poisson")
