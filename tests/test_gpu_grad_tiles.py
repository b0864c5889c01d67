"""The training kernel's gradient tiles are walked from the plan's tile table (vjf_mega_grad_tiles / mg_grad_walk, vjf_mega_common.h)
instead of one loop per tensor.  Three steps of `filter_sequence(sgd=True, update=True)` on the one-launch route at the smallest
shapes at which that table can go wrong (not the workload's own):

    bias16   hidden [15]: Kin + 1 = 16 at the heads -- the bias is the last column of a full tile; d_in = 23: two column tiles at layer 0
    bias17   hidden [16]: the bias row opens a column tile of its own with one column stored; the mean head's tile there is the dropped one
    layers2  hidden [33, 18], B = 40: two layers, M no multiple of 4 (ldm 36 / 20), a ragged second tile of 8 trials whose padding
             trials must add exact zeros
    dz16     d_z = 16 (the plan's limit) with a control input, Poisson: rows >= M of the last row tile
    layers3  hidden [20, 17, 5]: a third layer -- its tiles are a segment of their own, walked behind its delta, the running tile index
             carried over
    tiles2   B = 4481: 141 tiles of trials on at most 140 trial workgroups (n = 32: 250 compute units left of 256, 128 / 227 of them),
             so a workgroup's second tile takes the read-add-store path -- the smallest such batch

Each case: `filter_sequence` bit for bit against stepwise `filter` (the state blob included), every step against the fp64 oracle at the
tolerances test_gpu_variance_edges.py / test_gpu_block_layout.py hold the one-launch route to, the per-step route on the same inputs
(both within those tolerances of the oracle, hence of each other within their sum), and the gradient itself, recovered from one step
at lr = 1 the way tests/test_gpu_gradients.py does -- at quiet inputs chosen so that NO entry of any tensor is near the clip
(asserted on the fp64 reference before the device is touched): every entry of every tensor is compared, so a tile stored at the
wrong slab offset cannot hide behind the +-1 clip.  All tests need a real MI355X:  pytest -m gpu."""
import numpy as np
import pytest
import torch

from tests import gradient_cases as gc
from tests.helpers import load_oracle_state, state_close
from tests.test_gpu_parity import close

pytestmark = pytest.mark.gpu

T = 3
TRAIN = dict(sgd=True, update=True, warm_up=False)
CASES = {
    "bias16": (dict(dy=17, dz=3, du=0, n=32, hidden=[15], lik="gaussian"), 32),
    "bias17": (dict(dy=17, dz=3, du=0, n=32, hidden=[16], lik="gaussian"), 32),
    "layers2": (dict(dy=50, dz=10, du=0, n=32, hidden=[33, 18], lik="gaussian"), 40),
    "dz16": (dict(dy=21, dz=16, du=2, n=32, hidden=[20], lik="poisson"), 64),
    "layers3": (dict(dy=17, dz=3, du=0, n=32, hidden=[20, 17, 5], lik="gaussian"), 32),
    "tiles2": (dict(dy=17, dz=3, du=0, n=32, hidden=[16], lik="gaussian"), 4481),
}
for _name, (_shape, _B) in CASES.items():                      # (new names only: the shapes of tests/gradient_cases.py stay as they are)
    assert "gt_" + _name not in gc.SHAPES or gc.SHAPES["gt_" + _name] == _shape
    gc.SHAPES["gt_" + _name] = _shape


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


def _np(a, t=None):
    return None if a is None else (a if t is None else a[t]).numpy().astype(np.float64)


_ORACLE = {}


def oracle_steps(m, name, y, u, eps):
    """The fp64 oracle's three steps from the model's starting state: computed once per case, shared, never modified."""
    if name not in _ORACLE:
        s = load_oracle_state(m, np.float64)
        outs, mu, lv = [], None, None
        for t in range(T):
            o = gc.oracle_step(s, "Tanh", _np(y, t), _np(u, t), mu, lv, _np(eps[t], 0), _np(eps[t], 1), **TRAIN)
            mu, lv = o.mu_t, o.lv_t
            outs.append((o.mu_t.copy(), o.lv_t.copy(), [o.loss, o.recon, o.dyn, o.entropy]))
        _ORACLE[name] = (outs, s)
    return _ORACLE[name]


def against_oracle(m, outs, s, mus, lvs, losses):
    for t in range(T):
        close(mus[t], outs[t][0], rtol=2e-6, atol=2e-6)
        close(lvs[t], outs[t][1], rtol=2e-6, atol=2e-6)
        close(losses[t], outs[t][2], rtol=2e-5, atol=2e-5)
    close(m.transition.logvar, s.tr_logvar, rtol=0, atol=2e-5)
    state_close(m, s, rtol=5e-6, atol=1e-6, rls_rtol=3e-3, rls_atol=3e-5)


@pytest.mark.parametrize("name", list(CASES))
def test_three_steps(vjf, name):
    shape, B = CASES[name]
    y, u, eps = gc.inputs("gt_" + name, B, "quiet", T=T)
    ud = None if u is None else u
    # stepwise: three launches
    m = gc.build(vjf, "gt_" + name, lr=1e-3)
    outs, s = oracle_steps(m, name, y, u, eps)
    q, mus, lvs, losses = None, [], [], []
    for t in range(T):
        q, loss, *comp = m.filter(y[t], None if ud is None else ud[t], q, verbose=True, eps=(eps[t, 0], eps[t, 1]), **TRAIN)
        mus.append(q.mean), lvs.append(q.logvar), losses.append(torch.stack([loss, *comp]))
    assert m.route(**TRAIN) == "one-launch" and m.status() == 0
    against_oracle(m, outs, s, mus, lvs, losses)
    # one launch of three steps: bit for bit, the whole state too
    m2 = gc.build(vjf, "gt_" + name, lr=1e-3)
    mu2, lv2, loss2 = m2.filter_sequence(y, ud, None, eps=eps, **TRAIN)
    assert m2.route(**TRAIN) == "one-launch" and m2.status() == 0
    assert torch.equal(torch.stack(mus), mu2) and torch.equal(torch.stack(lvs), lv2) and torch.equal(torch.stack(losses), loss2)
    assert torch.equal(m._blob, m2._blob)
    # the per-step route: within the same tolerances of the oracle, so the two routes agree within their sum
    m3 = gc.build(vjf, "gt_" + name, lr=1e-3)
    m3.set_overlap(False)
    mu3, lv3, loss3 = m3.filter_sequence(y, ud, None, eps=eps, **TRAIN)
    assert m3.route(**TRAIN) == "per-step" and m3.status() == 0
    against_oracle(m3, outs, s, list(mu3), list(lv3), list(loss3))
    close(mu3, mu2.cpu().numpy(), rtol=4e-6, atol=4e-6)
    close(lv3, lv2.cpu().numpy(), rtol=4e-6, atol=4e-6)


_REFERENCES = {}


def gradient_case(vjf, name):
    """Model at lr = 1 in every group, quiet inputs and the fp64 reference of one step; NO entry of any tensor within its bound of the
    clip -- asserted here, on the reference alone, so that compare_step below compares every entry (it skips none)."""
    shape, B = CASES[name]
    m = gc.build(vjf, "gt_" + name, lr=1.0)
    gc.make_quiet(m, "gt_" + name)
    y, u, eps = gc.inputs("gt_" + name, B, "quiet")
    if name not in _REFERENCES:
        _REFERENCES[name] = gc.Reference(load_oracle_state(m, np.float64), "Tanh", y[0], None if u is None else u[0], eps[0])
    R = _REFERENCES[name]
    names = gc.trainables(R.s64, with_lik=False)
    w0 = gc.state64(m, names)
    for k in names:
        _, yard = gc.yardstick(R.ref[k], R.g32[k], True)
        bound = gc.F * yard + gc.ULP * (float(np.abs(w0[k]).max()) + 1.0)
        assert float(np.abs(R.ref[k]).max()) <= 1.0 - bound, f"{name}: {k}: max |g| {np.abs(R.ref[k]).max():.3f}: the clip is active"
    return m, (y, u, eps), R, names


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_of_every_tensor(vjf, name):
    m, (y, u, eps), R, names = gradient_case(vjf, name)
    assert {"dec_W", "dec_b", "mean_W", "lv_W", "lv_b", "rec_W0", "rec_b0"} <= set(names)
    w0 = gc.state64(m, names)
    m.filter_sequence(y.cuda(), None if u is None else u.cuda(), None, eps=eps.cuda(), **TRAIN)
    torch.cuda.synchronize()
    assert m.route(**TRAIN) == "one-launch" and m.status() == 0
    gc.compare_step(f"grad tiles {name} one-launch", w0, gc.state64(m, names), R, names, 1.0)
