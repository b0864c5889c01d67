"""The 32x32 Cholesky blocks in LDS with 33-float rows (vjf_chol_blocks.h): three training steps (`sgd=True, update=True`) on
every route that factors through those blocks, at the block counts and edges where an address of the layout can go wrong --
one block, a ragged last block with 4 valid rows, 2, 4 and 7 block columns with a ragged 7th -- against the fp64 oracle at
the tolerances of test_gpu_parity.py::test_filter_vs_oracle, and route against route bitwise where test_gpu_parity.py
asserts that (`filter_sequence` == the same steps through `filter`).  All tests need a real MI355X:  pytest -m gpu.

Routes: 'one-launch' (the Cholesky role of the resident grid, vjf_chol_loop<16>), 'per-step' (`set_overlap(False)`:
vjf_chol_lds_kernel<dzp> in post mode with the post kernels, or with its own inverse / solve tail for d_z > 16) and 'streams'
(`set_overlap(3)`: vjf_rls_pair_kernel<dzp>).  The oracle is stepped once per shape and shared by the routes.
"""
import numpy as np
import pytest
import torch

from oracle import vjf_oracle as orc
from tests.helpers import load_oracle_state, state_close
from tests.test_gpu_parity import close

pytestmark = pytest.mark.gpu

T, DY, HIDDEN = 3, 10, [16]
SHAPES = [(n, dz, B) for n in (4, 32, 36, 64, 100, 200, 224) for dz in (3, 10, 16) for B in (8, 40)]


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


def _fresh(vjf, n, dz, overlap):
    torch.manual_seed(41)
    m = vjf.VJF.make_model(DY, dz, 0, n, HIDDEN, likelihood="gaussian", lr=1e-3)
    if overlap is not None:
        m.set_overlap(overlap)
    return m


def _inputs(dz, B):
    g = torch.Generator().manual_seed(43)
    return torch.randn(T, B, DY, generator=g), torch.randn(T, 2, B, dz, generator=g)


def _oracle(model, y, eps):
    """Three oracle steps from the model's (fresh) state: the per-step outputs and the final OracleState."""
    s = load_oracle_state(model, np.float64)
    mu, lv, outs = None, None, []
    for t in range(T):
        o = orc.filter_step(s, y[t].numpy(), None, mu, lv, eps[t, 0].numpy(), eps[t, 1].numpy())
        mu, lv = o.mu_t, o.lv_t
        outs.append((o.mu_t.copy(), o.lv_t.copy(), [o.loss, o.recon, o.dyn, o.entropy], np.array(s.tr_logvar, np.float64).copy()))
    return s, outs


def _check_outputs(mu, lv, loss, outs):
    for t in range(T):
        close(mu[t], outs[t][0], rtol=2e-6, atol=2e-6)
        close(lv[t], outs[t][1], rtol=2e-6, atol=2e-6)
        close(loss[t], outs[t][2], rtol=2e-5, atol=2e-5)


def _check_state(m, s):
    close(m.transition.logvar, s.tr_logvar, rtol=0, atol=2e-5)
    state_close(m, s, rtol=5e-6, atol=1e-6, rls_rtol=3e-3, rls_atol=3e-5)      # P, W, w_chol, w_pchol at the [rls] pair
    assert m.status() == 0


def _run_steps(m, y, eps, outs=None):
    """T calls of `filter`; with `outs`, sigma is compared after every step as well."""
    q, mus, lvs, losses = None, [], [], []
    for t in range(T):
        q, loss, *comp = m.filter(y[t], None, q, sgd=True, update=True, verbose=True, eps=(eps[t, 0], eps[t, 1]))
        mus.append(q.mean), lvs.append(q.logvar), losses.append(torch.stack([loss, *comp]))
        if outs is not None:
            close(m.transition.logvar, outs[t][3], rtol=0, atol=2e-5)
    return torch.stack(mus), torch.stack(lvs), torch.stack(losses)


def _all_routes(vjf, n, dz, B, routes):
    y, eps = _inputs(dz, B)
    s = outs = None
    for overlap, want in routes:
        m = _fresh(vjf, n, dz, overlap)
        if s is None:
            s, outs = _oracle(m, y, eps)
        if overlap is None:
            mu, lv, loss = _run_steps(m, y, eps, outs)
            assert m.route() == want
            # the same steps as one `filter_sequence` call: same kernels, same order -- bitwise, the whole state too
            m2 = _fresh(vjf, n, dz, overlap)
            mu2, lv2, loss2 = m2.filter_sequence(y, None, None, eps=eps)
            assert torch.equal(mu, mu2) and torch.equal(lv, lv2) and torch.equal(loss, loss2)
            assert torch.equal(m._blob, m2._blob)
        else:
            mu, lv, loss = m.filter_sequence(y, None, None, eps=eps)
            assert m.route() == want
        _check_outputs(mu, lv, loss, outs)
        _check_state(m, s)


@pytest.mark.parametrize("n,dz,B", SHAPES, ids=lambda v: str(v))
def test_three_steps_on_every_route(vjf, n, dz, B):
    _all_routes(vjf, n, dz, B, [(None, "one-launch"), (False, "per-step"), (3, "streams")])


def test_three_steps_dz20_own_tail(vjf):
    """16 < d_z <= 32 (dzp = 32): vjf_chol_lds_kernel<32> with its own inverse and y / W tail -- X in place over L, the
    diagonal blocks copied element by element, the partial tiles of y and W in s_aux and in the region behind g.  The plan is
    served by the per-step kernels whatever the overlap setting."""
    _all_routes(vjf, 64, 20, 40, [(None, "per-step"), (False, "per-step")])


def test_largest_plan_of_the_lds_budget(vjf):
    """nbl = 6 with d_z = 20 (n = 192): 33 blocks of 33-float rows, two 192 x 32 regions and the control words are
    163,328 B, the bound of vjf_chol_lds_ok itself (with 1024-float blocks and 192 control floats it was 160,512 B): the
    last byte of the kernel's LDS layout is in use.  The launch is accepted (status 0) and the update is correct.  (That
    the predicate admits the plan is shown on the host: tools/chol_lds_plans.hip.)"""
    _all_routes(vjf, 192, 20, 8, [(False, "per-step")])
