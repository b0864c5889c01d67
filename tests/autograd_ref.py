"""TEST INFRASTRUCTURE: the gradient of one VJF.filter step from torch autograd in fp64 -- the reference's own way to a gradient
(vjf/model.py:206-210 calls loss.backward()), and independent of every hand-derived backward pass here: the three in the HIP routes,
oracle.vjf_oracle.filter_step's and tests/act_oracle.py's, which all follow one derivation.

The forward pass and the loss of vjf/model.py:97-154 are written with torch tensors from an OracleState.  The trainable tensors are
leaves with requires_grad; the prior, the RBF features, the RLS weights, the state-noise variance, the inputs and both draws are
constants, as in the reference's step (vjf/model.py:110, 331; vjf/module.py:20-21, 50-52).  Nothing here calls or copies a backward
pass.  A plain module: nothing is collected by pytest.
"""
import collections

import numpy as np
import torch
from torch import nn
from torch.nn import functional

from oracle import vjf_oracle as orc

RECON, DYNAMICS, ENTROPY = "recon", "dynamics", "entropy"

Ref = collections.namedtuple("Ref", "grads loss eta pre mu_t lv_t")


def trainable_names(s):
    """The trainable tensors in the order of the state blob, named as tests.helpers.model_arrays names them."""
    names = []
    for k in range(len(s.rec_W)):
        names += [f"rec_W{k}", f"rec_b{k}"]
    names += ["mean_W", "lv_W", "lv_b", "dec_W", "dec_b"]
    if s.likelihood == orc.GAUSSIAN:
        names.append("lik_logvar")
    return names


def _leaves(s):
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)      # noqa: E731
    p = {}
    for k, (W, b) in enumerate(zip(s.rec_W, s.rec_b)):
        p[f"rec_W{k}"], p[f"rec_b{k}"] = t(W), t(b)
    for k in ("mean_W", "lv_W", "lv_b", "dec_W", "dec_b"):
        p[k] = t(getattr(s, k))
    if s.likelihood == orc.GAUSSIAN:
        p["lik_logvar"] = t(s.lik_logvar)
    return p


def _gaussian_loss(m1, lv1, m2, lv2, logvar):
    """vjf/functional.py:32-75"""
    p = torch.exp(-.5 * logvar)
    mse = functional.mse_loss(m1 * p, m2 * p, reduction='none')
    nll = .5 * (mse + logvar)
    if lv1 is not None and lv2 is not None:
        nll = nll + .5 * torch.exp(lv1 + lv2 - logvar)
    return nll.sum(-1).mean()


def step(s, y, u, mu_s, lv_s, eps_s, eps_t, *, warm_up=False, activation=None, drop=()):
    """One step's loss and its gradient.
    :param s: OracleState (read, never modified); its `likelihood` selects Gaussian or Poisson
    :param mu_s, lv_s: the previous posterior, or None for the prior
    :param activation: the recognition layers' activation as an nn.Module (default nn.Tanh())
    :param drop: loss components that are the constant 0, as vjf/model.py:138-145 makes a non-finite one: any of
                 "recon", "dynamics", "entropy"
    :return: Ref(grads {tensor name: d(batch-mean loss)/d tensor, fp64 numpy -- zeros where the loss does not reach the tensor},
                 loss, eta (the decoder's output), pre (the layers' pre-activations), mu_t, lv_t)"""
    act = nn.Tanh() if activation is None else activation
    c = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)         # noqa: E731
    y = torch.atleast_2d(c(y))
    B = y.shape[0]
    u = torch.atleast_2d(c(u)) if (u is not None and np.shape(u)[-1] > 0) else None
    if mu_s is None:                                                    # vjf/model.py:80-95
        mu_s = torch.ones(B, s.xdim, dtype=torch.float64) * c(s.prior_mean)
        lv_s = torch.ones(B, s.xdim, dtype=torch.float64) * c(s.prior_logvar)
    else:
        mu_s, lv_s = c(mu_s), c(lv_s)                                   # (detached: model.py:110)
    p = _leaves(s)

    # ---- forward (vjf/model.py:97-122)
    xs = mu_s + c(eps_s) * torch.exp(.5 * lv_s)
    xu = xs if u is None else torch.cat((xs, u), dim=-1)
    d2 = ((xu[:, None, :] - c(s.centroid)[None, :, :]) ** 2).sum(-1)
    feat = torch.exp(-.5 * d2 / torch.exp(c(s.logwidth)) ** 2)          # vjf/functional.py:20-22
    FL = feat @ c(s.w_chol)
    pt_lv = (FL * FL).sum(1).log()[:, None].expand(B, s.xdim)           # vjf/module.py:75-76
    pt_mean = xs + feat @ c(s.w_mean)
    h = torch.cat([t for t in (y, u, mu_s, lv_s) if t is not None], dim=-1)         # vjf/recognition.py:32-36
    pre = []
    for k in range(len(s.rec_W)):
        a = functional.linear(h, p[f"rec_W{k}"], p[f"rec_b{k}"])
        pre.append(a.detach().numpy().copy())
        h = act(a)
    mu_t = functional.linear(h, p["mean_W"])
    lv_t = functional.linear(h, p["lv_W"], p["lv_b"])
    xt = mu_t + c(eps_t) * torch.exp(.5 * lv_t)
    py = functional.linear(xt, p["dec_W"], p["dec_b"])

    # ---- loss (vjf/model.py:124-154)
    zero = torch.zeros((), dtype=torch.float64)
    if RECON in drop:
        l_recon = zero
    elif s.likelihood == orc.GAUSSIAN:
        l_recon = _gaussian_loss(y, None, py, None, p["lik_logvar"])    # vjf/likelihood.py:26
    else:
        l_recon = functional.poisson_nll_loss(py.clamp(max=10.), y, log_input=True, reduction='none').sum(-1).mean()
    l_dyn = zero if DYNAMICS in drop else _gaussian_loss(pt_mean, pt_lv, mu_t, lv_t, c(s.tr_logvar))
    ent = zero if ENTROPY in drop else .5 * lv_t.sum(-1).mean()
    loss = l_recon - ent
    if not warm_up:
        loss = loss + l_dyn
    loss.backward()
    grads = {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.numpy().copy()) for k, v in p.items()}
    return Ref(grads, float(loss.detach()), py.detach().numpy().copy(), pre, mu_t.detach().numpy().copy(), lv_t.detach().numpy().copy())


def gradients(s, y, u, mu_s, lv_s, eps_s, eps_t, **kw):
    """{tensor name: gradient of the batch-mean loss} of `step`."""
    return step(s, y, u, mu_s, lv_s, eps_s, eps_t, **kw).grads


def hand_gradients(grads, s):
    """The `grads` dict of oracle.filter_step / act_oracle.filter_step under the same names (fp64; an absent gradient is 0)."""
    out = {}
    for k in range(len(s.rec_W)):
        out[f"rec_W{k}"], out[f"rec_b{k}"] = grads["rec_W"][k], grads["rec_b"][k]
    for k in ("mean_W", "lv_W", "lv_b", "dec_W", "dec_b"):
        out[k] = grads[k]
    if s.likelihood == orc.GAUSSIAN:
        out["lik_logvar"] = np.zeros(()) if grads["lik_logvar"] is None else grads["lik_logvar"]
    return {k: np.asarray(v, np.float64) for k, v in out.items()}
