"""The yardstick of the fixed-point tests itself (tests/fixed_point_ref.py on tests/fixed_point_cases.py): A against autograd, the
planted roots, convergence of the near starts in fp64 and fp32 -- the condition the GPU tests stand on --, monotone r2, and the
max_iter = 0 and NaN-start cases of the contract.  No GPU, no library."""
import numpy as np
import pytest
import torch

from tests import fixed_point_cases as fpc
from tests import fixed_point_ref as fr
from tests import tangent_ref as tr

NAMES = list(fpc.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_A_against_autograd(name):
    s = fpc.state(name)
    a = fpc.inputs(name, "far")
    x0 = a["x0"][:4].astype(np.float64)
    u = None if a["u"] is None else a["u"][:4].astype(np.float64)
    g, A = fr.g_and_A(s, x0, u)
    c, lw, w = (torch.tensor(v) for v in (s.centroid, s.logwidth, s.w_mean))
    for b in range(x0.shape[0]):
        def gmap(x):
            xu = x if u is None else torch.cat([x, torch.tensor(u[b])])
            d2 = ((xu[None, :] - c) ** 2).sum(1)
            return torch.exp(-0.5 * d2 / torch.exp(lw) ** 2) @ w
        want = torch.autograd.functional.jacobian(gmap, torch.tensor(x0[b])).numpy()
        assert np.abs(A[b] - want).max() <= 1e-10 * np.abs(want).max()
        np.testing.assert_allclose(g[b], gmap(torch.tensor(x0[b])).numpy(), rtol=0, atol=1e-13)
    # J = I + A is the tangent reference's Jacobian
    np.testing.assert_allclose(fr.jacobian(s, x0, u), tr.jacobian(s, x0, u), rtol=0, atol=1e-13)


@pytest.mark.parametrize("name", NAMES)
def test_the_planted_roots_are_roots(name):
    s = fpc.state(name)
    xs = fpc.roots(name)
    a = fpc.inputs(name)
    u = None if a["u"] is None else a["u"][:len(xs)].astype(np.float64)
    g = fr.g_and_A(s, xs, u)[0]
    assert np.sqrt((g * g).sum(1)).max() < 1e-6
    assert np.abs(s.w_mean).max() > 0.1          # (the projection left a map, not zeros)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", NAMES)
def test_near_starts_converge(name, dtype):
    """tol = 1e-5, max_iter = 40: every near start converges in at most 20 iterations, in fp64 and in fp32."""
    s = fpc.state(name, dtype)
    a = fpc.inputs(name, "near")
    x, res, nit, conv, hist = fr.solve(s, a["x0"], a["u"], max_iter=fpc.MAX_ITER, tol=fpc.TOL)
    print(f"{name} {np.dtype(dtype).name}: n_iter max {nit.max()}, residual max {res.max():.3e}")
    assert conv.all() and nit.max() <= 20
    assert (res <= fpc.TOL).all() and x.dtype == dtype and res.dtype == dtype
    for h in hist:
        assert all(h[i + 1] <= h[i] for i in range(len(h) - 1))
    # the reference's own result keeps the bound of the GPU test of the distance to the true root, no trial left out
    dist, lim, cond = fpc.root_distance(fpc.state(name), x, a["u"])
    print(f"{name} {np.dtype(dtype).name}: cond median {np.median(cond):.1f} max {cond.max():.1f}, worst |x - x**| / bound {(dist / lim).max():.3f}")
    assert cond.max() <= 1e5 and (dist <= 0.75 * lim).all()


@pytest.mark.parametrize("name", ["ragged3", "control"])
def test_r2_is_monotone_from_far_starts(name):
    s = fpc.state(name, np.float32)
    a = fpc.inputs(name, "far")
    x0 = a["x0"]
    x, res, nit, conv, hist = fr.solve(s, x0, a["u"], max_iter=12, tol=fpc.TOL)
    g0 = fr.g_and_A(s, x0, a["u"])[0]
    for b, h in enumerate(hist):
        assert all(h[i + 1] <= h[i] for i in range(len(h) - 1))
        assert h[0] == pytest.approx(float(np.sum(g0[b] * g0[b])), rel=1e-4)        # (a batched product rounds in another order)
    assert (nit[~conv] == 12).all() and (nit <= 12).all()
    assert (res <= np.sqrt((g0 * g0).sum(1)) * (1 + 1e-6)).all()


def test_no_iteration_returns_the_start():
    s = fpc.state("control", np.float32)
    a = fpc.inputs("control", "far")
    x, res, nit, conv, hist = fr.solve(s, a["x0"], a["u"], max_iter=0)
    g0 = fr.g_and_A(s, a["x0"], a["u"])[0]
    assert np.array_equal(x, a["x0"]) and (nit == 0).all() and not conv.any()
    np.testing.assert_allclose(res, np.sqrt((g0 * g0).sum(1)), rtol=1e-6)
    # a planted root as the start is done at the first comparison
    xs = fpc.roots("control").astype(np.float32)
    x, res, nit, conv, hist = fr.solve(s, xs, a["u"][:len(xs)], max_iter=5, tol=fpc.TOL)
    assert conv.all() and (nit <= 1).all()


def test_a_nan_start_returns_itself():
    s = fpc.state("ragged3", np.float32)
    a = fpc.inputs("ragged3", "near")
    x0 = a["x0"][:4].copy()
    x0[1, 0] = np.nan
    x, res, nit, conv, hist = fr.solve(s, x0, None, max_iter=5, tol=fpc.TOL)
    assert np.isnan(x[1, 0]) and np.array_equal(x[1, 1:], x0[1, 1:]) and np.isinf(res[1]) and not conv[1] and nit[1] == 5
    clean = fr.solve(s, a["x0"][:4], None, max_iter=5, tol=fpc.TOL)
    for r in (0, 2, 3):
        assert np.array_equal(x[r], clean[0][r]) and res[r] == clean[1][r]
