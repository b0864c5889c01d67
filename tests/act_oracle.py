"""numpy fp64 restatement of one VJF.filter step (vjf/model.py:179-221) and of Recognition.forward (vjf/recognition.py:31-42) with
the recognition layers' activation as a parameter (vjf/recognition.py:17-24).

Everything outside the recognition network -- RBF features, losses, the clip, the running variances, the RLS update -- is
oracle.vjf_oracle's.  The hand-derived backward of oracle.filter_step multiplies by 1 - h^2; this module restates that step with
the derivative of the activation taken from the layer's output h, as the HIP routes do (vjf_amd/csrc/vjf_act.h).  Each
derivative is the one torch's autograd uses for the module.

An activation is given as (kind, p0, p1) -- the C ABI's vjf_activation, vjf_amd.recognition.activation_code.
"""
import numpy as np

from oracle import vjf_oracle as orc
from oracle.vjf_oracle import GAUSSIAN, LIK_SIZE_CAP, TR_SIZE_CAP, StepOut, _clip, running_var

TANH, RELU, LEAKY_RELU, ELU, SOFTPLUS, SIGMOID, HARDTANH = range(7)
# fixture `act` names (tests/golden/make_golden_act.py) -> kind
KIND = {"Tanh": TANH, "ReLU": RELU, "LeakyReLU": LEAKY_RELU, "ELU": ELU, "Softplus": SOFTPLUS, "Sigmoid": SIGMOID,
        "Hardtanh": HARDTANH, "ReLU6": HARDTANH}


def act_of(z, prefix=""):
    """(kind, p0, p1) recorded in a g9_act_* fixture."""
    p = z[prefix + "act_params"]
    return KIND[str(z[prefix + "act"])], float(p[0]), float(p[1])


def fwd(act, a):
    kind, p0, p1 = act
    a = np.asarray(a)
    if kind == TANH:
        return np.tanh(a)
    if kind == RELU:
        return np.where(a < 0, 0.0, a).astype(a.dtype)
    if kind == LEAKY_RELU:
        return np.where(a > 0, a, p0 * a).astype(a.dtype)
    if kind == ELU:
        return np.where(a > 0, a, p0 * np.expm1(np.minimum(a, 0.0))).astype(a.dtype)
    if kind == SOFTPLUS:
        x = p0 * a
        return np.where(x > p1, a, np.logaddexp(0.0, x) / p0).astype(a.dtype)
    if kind == SIGMOID:
        return (0.5 * (1.0 + np.tanh(0.5 * a))).astype(a.dtype)
    if kind == HARDTANH:
        return np.clip(a, p0, p1).astype(a.dtype)
    raise ValueError(kind)


def dh(act, h):
    """dh/da from the output h."""
    kind, p0, p1 = act
    h = np.asarray(h)
    if kind == TANH:
        return 1.0 - h * h
    if kind == RELU:
        return (h > 0).astype(h.dtype)
    if kind == LEAKY_RELU:
        return np.where(h > 0, 1.0, p0).astype(h.dtype)
    if kind == ELU:
        return np.where(h > 0, 1.0, h + p0).astype(h.dtype)
    if kind == SOFTPLUS:
        return -np.expm1(-p0 * h)
    if kind == SIGMOID:
        return h * (1.0 - h)
    if kind == HARDTANH:
        return ((h > p0) & (h < p1)).astype(h.dtype)
    raise ValueError(kind)


def recognition_forward(s, act, y, mu_s, lv_s, u=None, keep=False):
    """oracle.recognition_forward with the activation `act`."""
    h = np.concatenate([x for x in (y, u, mu_s, lv_s) if x is not None], axis=-1)
    acts = [h]
    for W, b in zip(s.rec_W, s.rec_b):
        h = fwd(act, h @ W.T + b)
        acts.append(h)
    mu = h @ s.mean_W.T
    lv = h @ s.lv_W.T + s.lv_b
    return (mu, lv, acts) if keep else (mu, lv)


def filter_step(s, act, y, u, mu_s, lv_s, eps_s, eps_t, *, sgd=True, update=True, warm_up=False) -> StepOut:
    """oracle.filter_step with the activation `act` (mutates `s` as the reference mutates the model)."""
    dt = s.dtype
    y = np.atleast_2d(np.asarray(y, dt))
    B = y.shape[0]
    if u is not None:
        u = np.atleast_2d(np.asarray(u, dt))
    if mu_s is None:
        mu_s = np.ones((B, s.xdim), dt) * s.prior_mean
        lv_s = np.ones((B, s.xdim), dt) * s.prior_logvar
    eps_s = np.asarray(eps_s, dt)
    eps_t = np.asarray(eps_t, dt)

    # ---- forward (vjf/model.py:97-122)
    xs = mu_s + eps_s * np.exp(0.5 * lv_s)
    dmean, pt_lv, feat = orc.blr_predict(s, orc.nonecat(xs, u))
    pt_mean = xs + dmean
    mu_t, lv_t, acts = recognition_forward(s, act, y, mu_s, lv_s, u, keep=True)
    xt = mu_t + eps_t * np.exp(0.5 * lv_t)
    py = xt @ s.dec_W.T + s.dec_b

    # ---- loss (vjf/model.py:124-154)
    l_recon = orc.gaussian_loss(y, None, py, None, s.lik_logvar) if s.likelihood == GAUSSIAN else orc.poisson_loss(py, y)
    l_dyn = orc.gaussian_loss(pt_mean, pt_lv, mu_t, lv_t, s.tr_logvar)
    h = orc.gaussian_entropy(lv_t)
    ok_recon, ok_dyn, ok_h = bool(np.isfinite(l_recon)), bool(np.isfinite(l_dyn)), bool(np.isfinite(h))
    l_recon = l_recon if ok_recon else dt.type(0)
    l_dyn = l_dyn if ok_dyn else dt.type(0)
    h = h if ok_h else dt.type(0)
    loss = l_recon - h
    if not warm_up:
        loss = loss + l_dyn

    # ---- backward + clipped SGD (vjf/model.py:206-214)
    grads = {}
    if sgd:
        inv_b = dt.type(1.0 / B)
        r = py - y
        g_rho = None
        if not ok_recon:
            d_py = np.zeros_like(py)
        elif s.likelihood == GAUSSIAN:
            e = np.exp(-s.lik_logvar)
            d_py = e * r * inv_b
            g_rho = np.sum(0.5 * (1.0 - e * r * r)) * inv_b
        else:
            d_py = np.where(py <= 10.0, np.exp(np.minimum(py, 10.0)) - y, 0.0).astype(dt) * inv_b
        d_mu = np.zeros_like(mu_t)
        d_lv = np.zeros_like(lv_t)
        if (not warm_up) and ok_dyn:
            d_mu += -np.exp(-s.tr_logvar) * (pt_mean - mu_t) * inv_b
            d_lv += 0.5 * np.exp(pt_lv + lv_t - s.tr_logvar) * inv_b
        if ok_h:
            d_lv += -0.5 * inv_b
        g_decW = d_py.T @ xt
        g_decb = d_py.sum(0)
        d_xt = d_py @ s.dec_W
        d_mu = d_mu + d_xt
        d_lv = d_lv + d_xt * eps_t * 0.5 * np.exp(0.5 * lv_t)
        hL = acts[-1]
        g_meanW, g_lvW, g_lvb = d_mu.T @ hL, d_lv.T @ hL, d_lv.sum(0)
        d_h = d_mu @ s.mean_W + d_lv @ s.lv_W
        g_recW = [None] * len(s.rec_W)
        g_recb = [None] * len(s.rec_W)
        for k in reversed(range(len(s.rec_W))):
            d_a = d_h * dh(act, acts[k + 1])                      # (the activation's derivative from the layer's output)
            g_recW[k] = d_a.T @ acts[k]
            g_recb[k] = d_a.sum(0)
            d_h = d_a @ s.rec_W[k]
        grads = dict(lik_logvar=g_rho, dec_W=g_decW, dec_b=g_decb, mean_W=g_meanW, lv_W=g_lvW, lv_b=g_lvb, rec_W=g_recW, rec_b=g_recb)
        lr_lik, lr_dec, _lr_tr, lr_rec = (dt.type(x) for x in s.lr)
        if g_rho is not None:
            s.lik_logvar = (s.lik_logvar - lr_lik * _clip(g_rho)).astype(dt)
        if not s.freeze_decoder:
            s.dec_W = (s.dec_W - lr_dec * _clip(g_decW)).astype(dt)
            s.dec_b = (s.dec_b - lr_dec * _clip(g_decb)).astype(dt)
        s.mean_W = (s.mean_W - lr_rec * _clip(g_meanW)).astype(dt)
        s.lv_W = (s.lv_W - lr_rec * _clip(g_lvW)).astype(dt)
        s.lv_b = (s.lv_b - lr_rec * _clip(g_lvb)).astype(dt)
        for k in range(len(s.rec_W)):
            s.rec_W[k] = (s.rec_W[k] - lr_rec * _clip(g_recW[k])).astype(dt)
            s.rec_b[k] = (s.rec_b[k] - lr_rec * _clip(g_recb[k])).astype(dt)

    # ---- closed-form updates (vjf/model.py:156-177)
    rls_status = 0
    if update:
        if s.likelihood == GAUSSIAN:
            var, n = running_var(np.exp(s.lik_logvar), s.n_lik, np.mean((y - py) ** 2), B, LIK_SIZE_CAP)
            s.lik_logvar = np.asarray(np.log(var), dt)
            s.n_lik = n
        dx = xt - xs
        if not warm_up:
            rls_status = orc.rls(s, feat, dx, np.exp(s.tr_logvar), 1.0)
        residual = dx - feat @ s.w_mean
        var, n = running_var(np.exp(s.tr_logvar), s.n_tr, np.mean(residual ** 2), B, TR_SIZE_CAP)
        s.tr_logvar = np.asarray(np.log(var), dt)
        s.n_tr = n

    return StepOut(mu_t, lv_t, float(loss), float(-l_recon), float(-l_dyn), float(h), grads, xs, xt, py, pt_mean, pt_lv, rls_status)
