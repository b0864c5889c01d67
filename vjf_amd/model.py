"""vjf.model on the MI355X: VJF, RBFDS, LinearDecoder with the reference's signatures
(vjf/model.py), the filtering step running as HIP kernels behind the C ABI (include/vjf_hip.h).

Drop-in notes:
  * `filter()` is the reference's API; `feed()` is an alias (the reference has no `feed`).
  * the optimiser is the reference's clipped plain SGD with an ExponentialLR stepped per epoch in
    `fit` (vjf/model.py:69-78, 210-211, 303) -- executed on the device; `optimizer.param_groups`
    and `scheduler.step()` are kept as light host objects.
  * all parameters, the RLS state and the counters live in ONE device blob owned by the VJF
    object; module attributes (`likelihood.logvar`, `transition.velocity.w_mean`, ...) are views
    into it, updated in place by the kernels.
  * device arithmetic is fp32 whatever torch's default dtype is.
  * noise: by default the two reparametrisation draws per step come from torch's CPU generator
    in the reference's order (xs then xt), so `torch.manual_seed` reproduces the reference's
    trajectory; `noise="device"` draws on the GPU instead (faster, different stream).
"""
import atexit
import os
import ctypes
import logging
import math
import sys
import weakref
from collections import namedtuple
from itertools import zip_longest
from typing import Sequence, Tuple, Union

import torch
from torch import Tensor, nn
from torch.nn import Linear, Module, Parameter

from . import _native as N
from .distribution import Gaussian
from .functional import gaussian_entropy as entropy
from .functional import gaussian_loss
from .likelihood import GaussianLikelihood, PoissonLikelihood
from .module import RBF, LinearRegression, rebind
from .recognition import Recognition
from .util import dev32, kept_scratch, nonecat, reparametrize, running_var, storage_device, stream_ptr

try:                                   # progress bar as in the reference (vjf/model.py:245)
    from tqdm import trange
except Exception:                      # pragma: no cover
    def trange(n):
        class _R:
            def __enter__(self_): return self_
            def __exit__(self_, *a): return False
            def __iter__(self_): return iter(range(n))
            def set_postfix(self_, *a, **k): pass
        return _R()


# Native contexts are destroyed while the HIP runtime is alive: explicitly (`VJF.close()`), when a model is collected in a running
# interpreter, or -- for whatever is left -- from this hook, which is registered when the module is imported (after torch, so it runs
# BEFORE torch's and the HIP runtime's own exit handlers).  Nothing calls into the library from `__del__` during interpreter
# finalisation: by then streams and communicators may be gone.
_LIVE = weakref.WeakSet()


def _close_all():
    for m in list(_LIVE):
        try:
            m.close()
        except Exception:
            pass


atexit.register(_close_all)


# what VJF.forecast_ensemble returns: the per-step mean and population variance over the members of the latent state and of the
# decoder's output, and the members' latent states (S, n_step + 1, B, xdim) or None
ForecastEnsemble = namedtuple('ForecastEnsemble', ['x_mean', 'x_var', 'y_mean', 'y_var', 'x'])
# what RBFDS.lyapunov / VJF.lyapunov return: the exponents (B, m) in Gram-Schmidt column order, the final state (B, xdim) and
# orthonormal frame (B, xdim, m), and the per-interval log R_vv (ceil(n_step / qr_every), B, m) or None
LyapunovResult = namedtuple('LyapunovResult', ['exponents', 'x', 'q', 'log_stretch'])
FP_MAX_XDIM = 32                         # VJF_FP_MAXDOUT of vjf_fixed_points
SM_MAX_XDIM = 32                         # VJF_SM_MAXDOUT of vjf_smooth
EKF_MAX_XDIM = 32                        # VJF_EKF_MAXDOUT of vjf_ekf
LAPLACE_MAX_XDIM = 24                    # VJF_LAP_MAXDOUT of vjf_laplace_filter
LAPLACE_MAX_ITER = 64                    # VJF_LAP_MAXITER


class FixedPointResult(namedtuple('FixedPointResult', ['x', 'residual', 'converged', 'n_iter', 'jacobian'])):
    """What RBFDS.fixed_points / VJF.fixed_points return, per start: where the search ended x (B, xdim), |g(x)| there residual (B,),
    whether that is within `tol` converged (B,) bool, the steps taken n_iter (B,) int32 and the Jacobian of the mean map at x,
    jacobian (B, xdim, xdim), or None."""
    __slots__ = ()

    def unique(self, merge_tol: float = 1e-3):
        """The distinct fixed points among the converged rows, on the host: a row is kept if it is farther (Euclidean) than
        `merge_tol` from every row kept before it, in row order.
        :return: (x (K, xdim), jacobian (K, xdim, xdim) or None, count (K,) int64: the starts that reached each)"""
        idx = torch.nonzero(self.converged.cpu()).flatten()
        x = self.x.detach().cpu()
        kept, count = [], []
        for i in idx.tolist():
            for q, r in enumerate(kept):
                if float((x[i] - x[r]).norm()) <= merge_tol:
                    count[q] += 1
                    break
            else:
                kept.append(i)
                count.append(1)
        rows = torch.as_tensor(kept, dtype=torch.long, device=self.x.device)
        return self.x[rows], None if self.jacobian is None else self.jacobian[rows], torch.as_tensor(count, dtype=torch.long)


class SmoothResult(namedtuple('SmoothResult', ['mean', 'var', 'cov', 'head'])):
    """What RBFDS.smooth / VJF.smooth return: the smoothed means (T, B, xdim), the marginal variances var (T, B, xdim), the full
    covariances cov (T, B, xdim, xdim) or None, and head = (mean[0], cov of row 0 (B, xdim, xdim)): what a call on the rows before these
    takes as `after`."""
    __slots__ = ()

    def gaussian(self) -> Gaussian:
        """The smoothed marginals as the filter returns its posterior: Gaussian(mean, log var), e.g. for `model.decoder`."""
        return Gaussian(self.mean, self.var.log())


class EKFResult(namedtuple('EKFResult', ['mean', 'var', 'cov', 'loglik', 'head'])):
    """What VJF.ekf returns: the filtered means (T, B, xdim) of the model's own extended Kalman filter, the marginal variances var
    (T, B, xdim), the full covariances cov (T, B, xdim, xdim) or None, the row log-likelihoods loglik (T, B) = log p(y_t | y_1..t-1)
    (0 where a row is not observed) and head = (mean[-1], cov of the last row (B, xdim, xdim)): what a call on the following rows
    takes as `before`."""
    __slots__ = ()

    def gaussian(self) -> Gaussian:
        """The filtered marginals as `filter_sequence` returns its posterior: the diagonal Gaussian(mean, log var).  `smooth` accepts
        it -- and then treats the filtered covariance as diagonal: the off-diagonal part of `cov` is dropped."""
        return Gaussian(self.mean, self.var.log())

    def log_likelihood(self) -> Tensor:
        """The model evidence log p(y_1..T) per trial (B,), float64: the rows of `loglik` added up in float64."""
        return self.loglik.double().sum(dim=0)


class LaplaceFilterResult(namedtuple('LaplaceFilterResult', ['mean', 'var', 'cov', 'loglik', 'grad_norm', 'head'])):
    """What VJF.laplace_filter returns: the modes (T, B, xdim) of the Poisson model's own filter, the marginal variances var
    (T, B, xdim) and the full covariances cov (T, B, xdim, xdim) or None of the Laplace approximation there, the row evidences loglik
    (T, B) ~ log p(y_t | y_1..t-1) (0 where a row is not observed), grad_norm (T, B), the norm of the whitened gradient the last Newton
    step left (whether `n_iter` was enough), and head = (mean[-1], cov of the last row (B, xdim, xdim)): what a call on the following
    rows takes as `before`."""
    __slots__ = ()

    def gaussian(self) -> Gaussian:
        """The filtered marginals as `filter_sequence` returns its posterior: the diagonal Gaussian(mean, log var).  `smooth` accepts
        it -- and then treats the filtered covariance as diagonal: the off-diagonal part of `cov` is dropped."""
        return Gaussian(self.mean, self.var.log())

    def log_likelihood(self) -> Tensor:
        """The Laplace evidence log p(y_1..T) per trial (B,), float64: the rows of `loglik` added up in float64."""
        return self.loglik.double().sum(dim=0)


# what RBFDS.sample_posterior / VJF.sample_posterior return: the joint draws x (S, T, B, xdim) and head = x[:, 0] (S, B, xdim), what a
# call on the rows before these takes as `after`
PosteriorSamples = namedtuple('PosteriorSamples', ['x', 'head'])


class ForecastScore(namedtuple('ForecastScore', ['n', 'sse_x', 'base_x', 'sse_y', 'base_y', 'sst_x', 'sst_y', 'pred', 'kind'])):
    """What RBFDS.score_forecast / VJF.score_forecast return, every array with the horizon h = 0 .. n_step on its first axis and float64
    unless said otherwise, all on the record's device: n (n_step + 1,) int64, the (origin, trial) pairs whose horizon h lies inside the record, max(T - h, 0) B;
    sse_x (.., xdim), the summed squared error of the h-step prediction against the filtered mean h rows on (row 0 is exactly 0);
    base_x, the same for persistence (the origin's own mean as the prediction); sse_y, base_y (.., ydim) or None without y: under the
    Gaussian likelihood the summed squared error of the decoded prediction against y (row 0: the filter's own reconstruction error),
    under the Poisson likelihood the summed negative log-likelihood exp(min(eta, 10)) - y min(eta, 10) (without log y!); sst_x, sst_y,
    the targets' total sum of squares about their mean over the valid rows (sst_y is None under Poisson); pred (n_step, T, B, xdim)
    float32 or None, the h-step predictions themselves, NaN where t + h is beyond the record; kind: "gaussian", "poisson" or None
    (no y).  A horizon beyond the record has n = 0, sums 0 and NaN from the methods."""
    __slots__ = ()

    @staticmethod
    def _ratio(num, den):
        return 1. - num.sum(-1) / den.sum(-1)

    def r2_x(self) -> Tensor:
        """1 - sum sse_x / sum sst_x per horizon (sums over the columns)."""
        return self._ratio(self.sse_x, self.sst_x)

    def r2_y(self) -> Tensor:
        """1 - sum sse_y / sum sst_y per horizon; Gaussian likelihood only."""
        if self.sse_y is None or self.sst_y is None:
            raise ValueError("r2_y needs y and the Gaussian likelihood" if self.kind != "poisson" else
                             "r2_y is not defined under the Poisson likelihood: use skill_y")
        return self._ratio(self.sse_y, self.sst_y)

    def skill_x(self) -> Tensor:
        """1 - sum sse_x / sum base_x per horizon: above 0 where the learned map beats persistence."""
        return self._ratio(self.sse_x, self.base_x)

    def skill_y(self) -> Tensor:
        """1 - score / base per horizon for the observations (squared error, or the Poisson negative log-likelihood)."""
        if self.sse_y is None:
            raise ValueError("skill_y needs y")
        return self._ratio(self.sse_y, self.base_y)

    def mse_x(self) -> Tensor:
        """sse_x per (pair, column), per horizon."""
        return self.sse_x.sum(-1) / (self.n.to(self.sse_x.device, torch.float64) * self.sse_x.shape[-1])

    def mse_y(self) -> Tensor:
        """sse_y per (pair, column), per horizon (under Poisson: the mean negative log-likelihood)."""
        if self.sse_y is None:
            raise ValueError("mse_y needs y")
        return self.sse_y.sum(-1) / (self.n.to(self.sse_y.device, torch.float64) * self.sse_y.shape[-1])


def _suffix_sst(v: Tensor, K: int) -> Tensor:
    """(K + 1, dim) float64: per horizon h the sum of squares of rows h .. T - 1 of v (T, B, dim) about their own mean, from suffix
    sums of the values shifted by the overall mean; 0 for h >= T."""
    v = v.double()
    T, B, dim = v.shape
    v = v - v.mean((0, 1))
    # (the scan runs along the last axis of a contiguous (dim, T) array: torch's scan along an outer axis is serial per column)
    s1 = v.sum(1).t().contiguous().flip(1).cumsum(1).flip(1).t()
    s2 = (v * v).sum(1).t().contiguous().flip(1).cumsum(1).flip(1).t()
    out = torch.zeros(K + 1, dim, dtype=torch.float64, device=v.device)
    m = min(K + 1, T)
    cnt = ((T - torch.arange(m, device=v.device)) * B).to(torch.float64)[:, None]
    out[:m] = (s2[:m] - s1[:m] * s1[:m] / cnt).clamp_(min=0.)
    return out


class LinearDecoder(Module):
    """vjf/model.py:21-42"""
    def __init__(self, xdim: int, ydim: int):
        super().__init__()
        self.add_module('decode', Linear(xdim, ydim))
        for p in self.decode.parameters():
            p.requires_grad_(False)
            p.data = dev32(p.data, ndim2=False)
        self.n_sample = 0

    def forward(self, x: Union[Tensor, Gaussian]) -> Union[Tensor, Gaussian]:
        if isinstance(x, Tensor):
            x = dev32(x)
            lead = x.shape[:-1]
            x2 = x.reshape(-1, x.shape[-1])
            W, b = self.decode.weight, self.decode.bias
            out = torch.empty(x2.shape[0], W.shape[0], device=x.device, dtype=torch.float32)
            N.check(N.lib().vjf_linear_forward(N.ptr(x2), N.ptr(W), N.ptr(b), N.ptr(out), x2.shape[0], W.shape[1], W.shape[0],
                                               stream_ptr()), "vjf_linear_forward")
            return out.reshape(*lead, W.shape[0])
        elif isinstance(x, Gaussian):
            raise NotImplementedError("LinearDecoder on a Gaussian (vjf/model.py:31-40) is never taken by filter()")
        else:
            raise NotImplementedError


def detach(q: Gaussian) -> Gaussian:
    """vjf/model.py:45-47 (no autograd graph exists on the HIP path; kept for API parity)"""
    mean, logvar = q
    return Gaussian(mean.detach(), logvar.detach())


class _ParamGroups:
    """Stand-in for torch.optim.SGD's `param_groups` (vjf/model.py:69-77): four groups
    [likelihood, decoder, transition, recognition], each with its own 'lr'."""
    def __init__(self, lr):
        self.param_groups = [{'lr': lr, 'name': n} for n in ('likelihood', 'decoder', 'transition', 'recognition')]

    def zero_grad(self):
        pass


class _ExponentialLR:
    """ExponentialLR(gamma) stepped once per epoch (vjf/model.py:78, 303): lr <- lr * gamma, recursively."""
    def __init__(self, optimizer, gamma):
        self.optimizer, self.gamma = optimizer, gamma

    def step(self):
        for g in self.optimizer.param_groups:
            g['lr'] = g['lr'] * self.gamma


class RBFDS(Module):
    """RBF dynamical system  x[t] = x[t-1] + Phi([x[t-1], u[t]]) W    (vjf/model.py:327-391)"""
    def __init__(self, n_rbf: int, xdim: int, udim: int, shrink: float = 1.):
        """:param shrink: forgetting factor of the RLS update, 0 < shrink <= 1, 1 meaning no forgetfulness (vjf/module.py:80-96;
        the reference's step hard-codes 1, vjf/model.py:371)"""
        super().__init__()
        self.add_module('velocity', LinearRegression(RBF(xdim + udim, n_rbf), xdim))
        self.register_parameter('logvar', Parameter(dev32(torch.tensor(0.), ndim2=False), requires_grad=False))
        self._n_sample = 0
        self._fc_scratch = None
        self._fe_scratch = None
        self._ks_scratch = None
        object.__setattr__(self, '_owner', None)
        self._shrink = 1.
        self.shrink = shrink

    @property
    def n_sample(self):
        o = self._owner() if self._owner is not None else None
        return o._get_counter("tr") if o is not None else self._n_sample

    @n_sample.setter
    def n_sample(self, v):
        o = self._owner() if self._owner is not None else None
        if o is not None:
            o._set_counter("tr", v)
        else:
            self._n_sample = v

    @property
    def shrink(self) -> float:
        """Forgetting factor of the RLS update: P <- shrink P + Phi'Phi / v in every step that runs it (fused or operator by
        operator).  May be set between calls: the write is ordered on the current stream like the learning rates and holds from the
        next call on; the native context stays."""
        o = self._owner() if self._owner is not None else None
        return o._get_shrink() if o is not None else self._shrink

    @shrink.setter
    def shrink(self, v):
        v = float(v)
        if not 0. < v <= 1.:                        # (NaN fails both comparisons)
            raise ValueError(f"shrink must be in (0, 1], got {v}")
        o = self._owner() if self._owner is not None else None
        if o is not None:
            o._set_shrink(v)
        else:
            self._shrink = v

    def forward(self, x: Tensor, u: Tensor = None, sampling: bool = True, leak: float = 0., noise: Tensor = None):
        x = dev32(x)
        xu = nonecat(x, None if u is None else dev32(u))
        dx = self.velocity(xu, sampling=sampling, noise=noise)
        if isinstance(dx, Gaussian):
            return Gaussian((1 - leak) * x + dx.mean, dx.logvar)
        else:
            return (1 - leak) * x + dx

    def forecast(self, x0: Tensor, u: Tensor = None, n_step: int = 1, *, noise: bool = False) -> Tensor:
        """vjf/model.py:342-361: sequential sampled roll-out (a fresh weight sample every step)."""
        x0 = dev32(x0)
        x = torch.empty(n_step + 1, *x0.shape, device=x0.device, dtype=torch.float32)
        x[0] = x0
        s = torch.exp(.5 * self.logvar)
        if u is None:
            u = [None] * n_step
        else:
            u = dev32(u)
            assert u.shape[0] == n_step, 'u must have length of n_step if present'
        for t in range(n_step):
            x[t + 1] = self.forward(x[t], u[t], sampling=True)
            if noise:
                e = torch.randn(x[t + 1].shape, dtype=torch.get_default_dtype()).to(x.device, torch.float32)
                x[t + 1] = x[t + 1] + e * s
        return x

    def _noise_mode(self) -> str:
        o = self._owner() if self._owner is not None else None
        return o.noise if o is not None else "reference"

    def _forecast_inputs(self, x0, u, lead, noise, w_noise, state_noise):
        """(u, w_noise, state_noise, held) as vjf_forecast_seq / vjf_forecast_ens take them: given ones coerced, missing ones drawn.
        `lead`: the noise tensors' leading shape, (T,) for one roll-out, (S, T) for an ensemble; x0: (..., B, xdim) on its device.
        `held`: the per-step host draws, which the caller keeps until its native call is enqueued: a few hundred small tensors are
        then released while the device works, not in front of the launch."""
        vel = self.velocity
        B, dout = x0.shape[-2:]
        n, d = vel.feature.centroid.shape
        du, T = d - dout, lead[-1]
        if du > 0:
            if u is None:
                raise TypeError("u is required when udim > 0")
            u = dev32(u, ndim2=False)
            assert u.shape[0] == T, 'u must have length of n_step if present'
            if u.ndim == 2 and B == 1:
                u = u[:, None, :]
            assert u.shape == (T, B, du)
            u = u.contiguous()
        else:
            u = None
        if w_noise is not None:
            w_noise = dev32(w_noise, ndim2=False)
            assert w_noise.shape == (*lead, n, dout)
        if state_noise is not None:
            state_noise = dev32(state_noise, ndim2=False)
            if state_noise.ndim == len(lead) + 1 and B == 1:
                state_noise = state_noise.unsqueeze(-2)
            assert state_noise.shape == (*lead, B, dout)
            state_noise = state_noise.contiguous()
        want_w, want_s = w_noise is None and T > 0, state_noise is None and noise and T > 0
        ws = []
        if self._noise_mode() != "reference":
            if want_w:
                w_noise = torch.randn(*lead, n, dout, device=x0.device, dtype=torch.float32)
            if want_s:
                state_noise = torch.randn(*lead, B, dout, device=x0.device, dtype=torch.float32)
        elif want_w or want_s:
            # forecast's order, roll-out by roll-out: per step the weight draw, then the state draw.  (The state draws go straight into
            # one page-locked tensor, a contiguous slice per step -- the values and the generator state of `randn(B, xdim)` -- and from
            # there to the device in one copy: at 4096 trials the draws themselves are most of the call's time, a stack of 200 tensors
            # and a pageable copy would add half as much again)
            dt, steps = torch.get_default_dtype(), math.prod(lead)
            ss = torch.empty(steps, B, dout, dtype=dt, pin_memory=x0.is_cuda) if want_s else None
            for i in range(steps):
                if want_w:
                    ws.append(vel._draw_weight_noise())
                if want_s:
                    torch.randn(B, dout, dtype=dt, out=ss[i])
            if want_w:
                w_noise = dev32(torch.stack(ws).reshape(*lead, n, dout), ndim2=False)
            if want_s:
                state_noise = ss.to(x0.device, torch.float32, non_blocking=True).contiguous().view(*lead, B, dout)
        return u, w_noise, state_noise, ws

    def forecast_sequence(self, x0: Tensor, u: Tensor = None, n_step: int = 1, *, noise: bool = False,
                          w_noise: Tensor = None, state_noise: Tensor = None) -> Tensor:
        """`forecast` as ONE C-ABI call (vjf_forecast_seq): the weight samples of all steps from one batched product, then the
        roll-out inside one kernel per chunk of steps -- what `filter_sequence` is to `filter`.  Same shapes and return type.
        :param w_noise: (n_step, n_rbf, xdim), used in place of the per-step randn_like(w) draws
        :param state_noise: (n_step, B, xdim), used in place of the per-step process-noise draws; implies `noise`
        Draws that are not given follow the owning model's `noise`: "reference" draws on the CPU generator in `forecast`'s own order
        (per step the weight draw, then the state draw), so a seed gives the same roll-out and leaves the generator where `forecast`
        leaves it; "device" draws each tensor on the GPU in one call.  Asynchronous; reads the model's state and writes none.
        The weight samples live in ONE scratch tensor kept on this module (like `_rls_scratch`): run one roll-out per model at a time
        -- calls on different streams must be ordered by the caller, or go to different models."""
        x0 = dev32(x0)
        vel = self.velocity
        B, dout = x0.shape
        n, d = vel.feature.centroid.shape
        assert dout == vel.n_output, f"x0 has {dout} columns, expected xdim={vel.n_output}"
        T = int(n_step)
        assert T >= 0, 'n_step must not be negative'
        u, w_noise, state_noise, _held = self._forecast_inputs(x0, u, (T,), noise, w_noise, state_noise)   # (_held: freed after the launch)
        if T == 0:
            return x0[None].clone()
        L = N.lib()
        self._fc_scratch = kept_scratch(self._fc_scratch, x0.device, L.vjf_forecast_scratch_size, T, n, dout)
        x = torch.empty(T + 1, B, dout, device=x0.device, dtype=torch.float32)
        N.check(L.vjf_forecast_seq(N.ptr(x0), N.ptr(u), N.ptr(w_noise), N.ptr(state_noise), N.ptr(vel.feature.centroid),
                                   N.ptr(vel.feature.logwidth), N.ptr(vel.w_mean), N.ptr(vel.w_chol), N.ptr(self.logvar), N.ptr(x),
                                   N.ptr(self._fc_scratch), T, B, n, d, dout, stream_ptr()), "vjf_forecast_seq")
        return x

    def forecast_ensemble(self, x0: Union[Tensor, Gaussian], u: Tensor = None, n_step: int = 1, n_sample: int = 16, *,
                          noise: bool = False, w_noise: Tensor = None, state_noise: Tensor = None, x0_noise: Tensor = None,
                          return_members: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """`n_sample` independent sampled roll-outs of the whole horizon and their per-step mean and variance as ONE C-ABI call
        (vjf_forecast_ens).  `forecast` draws fresh weights at every step, so one roll-out is one draw of the model's predictive
        distribution; this is the distribution's first two moments.  Member s is exactly the roll-out `forecast_sequence` computes on
        member s's draws.  The variance is the population one, sum (v - mean)^2 / S: exactly 0 with one member.
        :param x0: (B, xdim), shared by the members; or (S, B, xdim), one start per member; or a Gaussian(mean, logvar), e.g. the
            posterior `filter` returned: member s starts at mean + x0_noise[s] * exp(logvar / 2)
        :param u: (n_step, B, udim), shared by the members
        :param w_noise: (S, n_step, n_rbf, xdim);  :param state_noise: (S, n_step, B, xdim), implies `noise`;
        :param x0_noise: (S, B, xdim), read only when x0 is a Gaussian
        Draws that are not given follow the owning model's `noise`, as in `forecast_sequence`.  "device": one torch.randn per tensor
        on the GPU.  "reference": the CPU generator, first x0_noise as one randn(S, B, xdim) (only for a Gaussian x0), then for member
        0, 1, ... exactly `forecast`'s draws (per step the weight draw, then the state draw): with a plain x0 and a seed, the members
        are bit for bit what S successive `forecast_sequence` calls under that seed return, and the generator ends in the same state.
        :return: x_mean, x_var (n_step + 1, B, xdim) and the members x (S, n_step + 1, B, xdim) if `return_members`, else None
        Asynchronous; reads the model's state and writes none.  The members' weight samples and states live in ONE bounded scratch
        tensor kept on this module (like `_fc_scratch`): run one ensemble per model at a time -- calls on different streams must be
        ordered by the caller, or go to different models."""
        x_mean, x_var, _, _, x = self._forecast_ensemble(None, x0, u, n_step, n_sample, noise, w_noise, state_noise, x0_noise,
                                                         return_members)
        return x_mean, x_var, x

    def _forecast_ensemble(self, decoder, x0, u, n_step, n_sample, noise, w_noise, state_noise, x0_noise, return_members):
        """(x_mean, x_var, y_mean, y_var, x) of forecast_ensemble; the y moments are those of decoder(x) (None without a decoder)."""
        S, T = int(n_sample), int(n_step)
        if S < 1:
            raise ValueError(f"n_sample must be at least 1, got {n_sample}")
        assert T >= 0, 'n_step must not be negative'
        vel = self.velocity
        n, d = vel.feature.centroid.shape
        reference = self._noise_mode() == "reference"
        dt = torch.get_default_dtype()
        if isinstance(x0, Gaussian):                       # the starts are formed here with torch ops: input handling, not hot path
            mean, logvar = dev32(x0.mean), dev32(x0.logvar)
            B, dout = mean.shape
            assert logvar.shape == mean.shape
            if x0_noise is None:
                x0_noise = (dev32(torch.randn(S, B, dout, dtype=dt), ndim2=False) if reference
                            else torch.randn(S, B, dout, device=mean.device, dtype=torch.float32))
            else:
                x0_noise = dev32(x0_noise, ndim2=False)
                if x0_noise.ndim == 2 and B == 1:
                    x0_noise = x0_noise[:, None, :]
            assert x0_noise.shape == (S, B, dout)
            x0 = (mean + x0_noise * torch.exp(.5 * logvar)).contiguous()
        else:
            x0 = dev32(x0, ndim2=False)
            if x0.ndim < 3:
                x0 = dev32(x0)
        B, dout = x0.shape[-2:]
        per_member = x0.ndim == 3
        assert x0.ndim == 2 or x0.shape[0] == S, f"x0 has {x0.shape[0]} starts, expected n_sample={S}"
        assert dout == vel.n_output, f"x0 has {dout} columns, expected xdim={vel.n_output}"
        u, w_noise, state_noise, _held = self._forecast_inputs(x0, u, (S, T), noise, w_noise, state_noise)   # (_held: freed after the launch)
        L = N.lib()
        self._fe_scratch = kept_scratch(self._fe_scratch, x0.device, L.vjf_forecast_ens_scratch_size, T, S, B, n, dout)
        new = lambda *shape: torch.empty(*shape, device=x0.device, dtype=torch.float32)      # noqa: E731
        x_mean, x_var = new(T + 1, B, dout), new(T + 1, B, dout)
        W = b = y_mean = y_var = None
        dy = 0
        if decoder is not None:
            W, b = decoder.decode.weight, decoder.decode.bias
            dy = W.shape[0]
            y_mean, y_var = new(T + 1, B, dy), new(T + 1, B, dy)
        x = None
        if return_members:                                 # (with no step to take the members are the starts)
            x = new(S, T + 1, B, dout) if T > 0 else (x0 if per_member else x0.expand(S, B, dout))[:, None].clone()
        N.check(L.vjf_forecast_ens(N.ptr(x0), B * dout if per_member else 0, N.ptr(u), N.ptr(w_noise), N.ptr(state_noise),
                                   N.ptr(vel.feature.centroid), N.ptr(vel.feature.logwidth), N.ptr(vel.w_mean), N.ptr(vel.w_chol),
                                   N.ptr(self.logvar), N.ptr(W), N.ptr(b), N.ptr(x_mean), N.ptr(x_var), N.ptr(y_mean), N.ptr(y_var),
                                   N.ptr(x) if T > 0 else None, N.ptr(self._fe_scratch), T, S, B, n, d, dout, dy, stream_ptr()),
                "vjf_forecast_ens")
        return x_mean, x_var, y_mean, y_var, x

    def _tangent(self, x0, u, q0, n_step, m, qr_every, lsum=None, history=False):
        """One vjf_tangent_rollout call: (x, q, lsum, lhist).  x0 (B, xdim), u (n_step, B, udim) or None, q0 (B, xdim, m) or None (the
        first m columns of I), as the library takes them; lsum (B, m): sums to go on from (None: from 0)."""
        vel = self.velocity
        B, dout = x0.shape
        n, d = vel.feature.centroid.shape
        new = lambda *shape: torch.empty(*shape, device=x0.device, dtype=torch.float32)      # noqa: E731
        x, q = new(B, dout), new(B, dout, m)
        accumulate = lsum is not None
        if qr_every > 0 and lsum is None:
            lsum = new(B, m)
        lhist = new(-(-n_step // qr_every), B, m) if history else None
        N.check(N.lib().vjf_tangent_rollout(N.ptr(x0), N.ptr(u), N.ptr(q0), N.ptr(vel.feature.centroid), N.ptr(vel.feature.logwidth),
                                            N.ptr(vel.w_mean), N.ptr(x), N.ptr(q), N.ptr(lsum), N.ptr(lhist), n_step, B, n, d, dout, m,
                                            qr_every, int(accumulate), stream_ptr()), "vjf_tangent_rollout")
        return x, q, lsum, lhist

    def _tangent_u(self, u, T, B):
        """u as (T, B, udim) on the device, or None for a model without a control input (forecast_sequence's coercion and refusals)."""
        n, d = self.velocity.feature.centroid.shape
        du = d - self.velocity.n_output
        if du == 0:
            return None
        if u is None:
            raise TypeError("u is required when udim > 0")
        u = dev32(u, ndim2=False)
        assert u.shape[0] == T, 'u must have length of burn_in + n_step if present'
        if u.ndim == 2 and B == 1:
            u = u[:, None, :]
        assert u.shape == (T, B, du)
        return u.contiguous()

    def jacobian(self, x: Tensor, u: Tensor = None) -> Tensor:
        """The Jacobian of the mean map, d/dx of the mean of `forward(x, u, sampling=False)`, as ONE C-ABI call (vjf_tangent_rollout:
        one step from the identity frame, never normalised):  J = I - w_mean^T G,  G[k, j] = phi_k (x_j - c_kj) / width_k^2.
        :param x: (B, xdim);  :param u: (B, udim), a parameter of the map, not a direction
        :return: (B, xdim, xdim), J[b, i, j] = d f_i / d x_j
        Asynchronous; reads the model's state and writes none."""
        x = dev32(x)
        B, dout = x.shape
        assert dout == self.velocity.n_output, f"x has {dout} columns, expected xdim={self.velocity.n_output}"
        if u is not None:
            u = dev32(u)[None]
        u = self._tangent_u(u, 1, B)
        return self._tangent(x, u, None, 1, dout, 0)[1]

    def lyapunov(self, x0: Tensor, u: Tensor = None, n_step: int = 1, *, n_exponent: int = None, qr_every: int = 1,
                 q0: Tensor = None, burn_in: int = 0, dt: float = 1.0, return_history: bool = False) -> LyapunovResult:
        """The leading Lyapunov exponents of the mean map x[t+1] = x[t] + Phi([x[t], u[t]]) w_mean along the trajectory from `x0`, the
        whole horizon as ONE C-ABI call (vjf_tangent_rollout): the state and a frame of `n_exponent` tangent vectors per trial stay
        on chip, the frame is mapped by the Jacobian at every step and re-orthonormalised every `qr_every` steps (and behind the last)
        by one pass of modified Gram-Schmidt in column order; the logs of the diagonal of R are summed.
        :param x0: (B, xdim);  :param u: (burn_in + n_step, B, udim) when the model has a control input
        :param n_exponent: m, 1 <= m <= xdim (default xdim);  :param q0: (B, xdim, m), the frame to start from (default: the first m
            columns of I); it should be orthonormal, as a returned `q` is
        :param burn_in: steps that run first through the same entry point; their sums are discarded, the state and frame carry on
        :param dt: the time one step stands for: exponents = sums / (n_step dt)
        :return: LyapunovResult(exponents (B, m), x (B, xdim), q (B, xdim, m), log_stretch (ceil(n_step / qr_every), B, m) if
            `return_history` else None).  The exponents are in Gram-Schmidt column order -- ordered by construction (column v of the
            frame converges to the v-th most expanding direction), NOT sorted: over a short horizon they need not decrease.  `x` is the
            final state and `q` the final orthonormal frame: pass them back as `x0` / `q0` (with burn_in = 0) to continue the run; when
            n_step is a multiple of qr_every the continued run computes the bits of the undivided one.  n_step = 0: x0 itself, q0
            orthonormalised once, exponents NaN.
        Asynchronous; reads the model's state and writes none; no scratch."""
        x0 = dev32(x0)
        B, dout = x0.shape
        assert dout == self.velocity.n_output, f"x0 has {dout} columns, expected xdim={self.velocity.n_output}"
        T, T0, qr = int(n_step), int(burn_in), int(qr_every)
        assert T >= 0, 'n_step must not be negative'
        assert T0 >= 0, 'burn_in must not be negative'
        m = dout if n_exponent is None else int(n_exponent)
        if not 1 <= m <= dout:
            raise ValueError(f"n_exponent must be in 1..xdim={dout}, got {n_exponent}")
        if qr < 1:
            raise ValueError(f"qr_every must be at least 1, got {qr_every}")
        dt = float(dt)
        if not dt > 0.:
            raise ValueError(f"dt must be positive, got {dt}")
        if q0 is not None:
            q0 = dev32(q0, ndim2=False)
            if q0.ndim == 2 and B == 1:
                q0 = q0[None]
            assert q0.shape == (B, dout, m), f"q0 is {tuple(q0.shape)}, expected {(B, dout, m)}"
            q0 = q0.contiguous()
        u = self._tangent_u(u, T0 + T, B)
        if T0 > 0:
            x0, q0, _, _ = self._tangent(x0, None if u is None else u[:T0], q0, T0, m, qr)
        x, q, lsum, hist = self._tangent(x0, None if u is None else u[T0:], q0, T, m, qr, history=return_history)
        exponents = lsum / (T * dt) if T > 0 else torch.full_like(lsum, float('nan'))
        return LyapunovResult(exponents, x, q, hist)

    def fixed_points(self, x0: Tensor, u: Tensor = None, *, max_iter: int = 64, tol: float = 1e-5, damping: float = 1e-3,
                     return_jacobian: bool = True) -> FixedPointResult:
        """Fixed points of the mean map, x with g(x, u) = Phi([x, u]) w_mean = 0, from every start of `x0` as ONE C-ABI call
        (vjf_fixed_points): a damped Newton (Levenberg-Marquardt) search on |g|^2 whose whole iteration stays on chip -- a step is
        accepted only if it lowers |g|, the damping falls by 10 after an accepted step and rises by 10 after a rejected one.
        :param x0: (B, xdim), the starts;  :param u: (B, udim), a constant input per start: a parameter of the map
        :param max_iter: candidates tried at most;  :param tol: a start has converged once |g(x)| <= tol
        :param damping: the first damping, relative to the mean diagonal of A^T A (A = dg/dx)
        :return: FixedPointResult(x (B, xdim), residual (B,), converged (B,) bool, n_iter (B,) int32, jacobian (B, xdim, xdim) =
            d f / d x of f = x + g at x if `return_jacobian` else None).  A start that has not converged returns the best point it
            reached (never worse than the start); the moduli of the eigenvalues of `jacobian` tell a stable fixed point (all < 1).
        Asynchronous; reads the model's state and writes none; no scratch."""
        x0 = dev32(x0)
        B, dout = x0.shape
        assert dout == self.velocity.n_output, f"x0 has {dout} columns, expected xdim={self.velocity.n_output}"
        if dout > FP_MAX_XDIM:
            raise NotImplementedError(f"fixed_points covers xdim <= {FP_MAX_XDIM}, this model has xdim = {dout}")
        max_iter, tol, damping = int(max_iter), float(tol), float(damping)
        if max_iter < 0:
            raise ValueError(f"max_iter must not be negative, got {max_iter}")
        if not 0. < tol < float('inf'):
            raise ValueError(f"tol must be positive and finite, got {tol}")
        if not 0. < damping < float('inf'):
            raise ValueError(f"damping must be positive and finite, got {damping}")
        if u is not None:
            u = dev32(u)[None]
        u = self._tangent_u(u, 1, B)
        vel = self.velocity
        n, d = vel.feature.centroid.shape
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, device=x0.device, dtype=dtype)      # noqa: E731
        x, residual, n_iter, conv = new(B, dout), new(B), new(B, dtype=torch.int32), new(B, dtype=torch.int32)
        jac = new(B, dout, dout) if return_jacobian else None
        N.check(N.lib().vjf_fixed_points(N.ptr(x0), N.ptr(u), N.ptr(vel.feature.centroid), N.ptr(vel.feature.logwidth), N.ptr(vel.w_mean),
                                         N.ptr(x), N.ptr(residual), N.ptr(n_iter), N.ptr(conv), N.ptr(jac), B, n, d, dout, max_iter,
                                         tol, damping, stream_ptr()), "vjf_fixed_points")
        return FixedPointResult(x, residual, conv != 0, n_iter, jac)

    def smooth(self, q: Union[Gaussian, Tuple[Tensor, Tensor]], u: Tensor = None, *, state_var: float = None,
               after: Tuple[Tensor, Tensor] = None, return_cov: bool = False) -> SmoothResult:
        """The smoothed posterior q(x_t | y_1..T) of a filtered sequence as ONE C-ABI call (vjf_smooth): the extended
        Rauch-Tung-Striebel pass with the learned mean map and its Jacobian, backwards over the whole record on chip, in the
        information form stated in include/vjf_hip.h (a sum of two positive semi-definite terms per row, one factorisation of a matrix
        bounded below by I).
        :param q: the filtered posterior, a Gaussian or a (mu, logvar) pair of (T, B, xdim) -- what `filter_sequence` / `fit` return;
            a (T, xdim) pair is one trial
        :param u: (T, B, udim), the array that went into the filter (the step from row t to t + 1 reads u[t + 1]; u[0] is never
            read); with `after`, (T + 1, B, udim): u[T] drives the step into the after-row
        :param state_var: the scalar state-noise variance, positive; default exp(self.logvar) -- reading that default copies one
            scalar to the host, which synchronises the stream; pass a float to stay asynchronous
        :param after: (mean (B, xdim), cov (B, xdim, xdim)), the smoothed moments of the row behind the last one, such as a previous
            result's `head`: smoothing rows [k, T) first and rows [0, k) with after = that head second gives the bits of one call
        :param return_cov: also return the full covariances
        :return: SmoothResult(mean, var (T, B, xdim), cov (T, B, xdim, xdim) or None, head = (mean[0], cov of row 0)).  A trial with
            a non-finite input at some row has NaN from that row back to row 0.
        Every xdim <= 24 with n_rbf <= 256 and udim <= 8 is accepted.  Beyond it the shape has to fit one workgroup's LDS: without a
        control input n_rbf <= 753 at xdim = 24, 660 at 25, 463 at 27, 360 at 28, 141 at 30 and 27 at 31 (eight control inputs take 7
        or 8 off); xdim = 32 never fits.  What does not fit raises NotImplementedError naming the limit before anything is launched.
        These shapes are tested up to the last admitted n_rbf (tests/test_gpu_shape_range.py).
        Reads the model's state and writes none; no scratch."""
        mu, lv = (q.mean, q.logvar) if isinstance(q, Gaussian) else q
        mu, lv = dev32(mu, ndim2=False), dev32(lv, ndim2=False)
        mu, lv = (t[:, None, :] if t.ndim == 2 else t for t in (mu, lv))        # (T, xdim): one trial
        assert mu.ndim == 3 and lv.shape == mu.shape, f"q is {tuple(mu.shape)} and {tuple(lv.shape)}, expected two (T, B, xdim)"
        mu, lv = mu.contiguous(), lv.contiguous()
        T, B, dout = mu.shape
        assert T >= 1, 'q must have at least one row'
        assert dout == self.velocity.n_output, f"q has {dout} columns, expected xdim={self.velocity.n_output}"
        if dout > SM_MAX_XDIM:
            raise NotImplementedError(f"smooth covers xdim <= {SM_MAX_XDIM}, this model has xdim = {dout}")
        state_var = float(self.logvar.exp()) if state_var is None else float(state_var)
        if not 0. < state_var < float('inf'):
            raise ValueError(f"state_var must be positive and finite, got {state_var}")
        a_mean = a_cov = None
        if after is not None:
            a_mean, a_cov = after
            a_mean, a_cov = dev32(a_mean), dev32(a_cov, ndim2=False)
            if a_cov.ndim == 2:
                a_cov = a_cov[None]
            assert a_mean.shape == (B, dout), f"after[0] is {tuple(a_mean.shape)}, expected {(B, dout)}"
            assert a_cov.shape == (B, dout, dout), f"after[1] is {tuple(a_cov.shape)}, expected {(B, dout, dout)}"
            a_cov = a_cov.contiguous()
        vel = self.velocity
        n, d = vel.feature.centroid.shape
        rows = T + (after is not None)
        if d > dout and u is not None:
            u = dev32(u, ndim2=False)
            assert u.shape[0] == rows, f"u has {u.shape[0]} rows, expected {rows} (T{' + 1 with `after`' if after is not None else ''})"
        u = self._tangent_u(u, rows, B)
        new = lambda *shape: torch.empty(*shape, device=mu.device, dtype=torch.float32)      # noqa: E731
        mean, var, cov0 = new(T, B, dout), new(T, B, dout), new(B, dout, dout)
        cov = new(T, B, dout, dout) if return_cov else None
        rc = N.lib().vjf_smooth(N.ptr(mu), N.ptr(lv), N.ptr(u), N.ptr(vel.feature.centroid), N.ptr(vel.feature.logwidth),
                                N.ptr(vel.w_mean), N.ptr(a_mean), N.ptr(a_cov), N.ptr(mean), N.ptr(var), N.ptr(cov), N.ptr(cov0),
                                T, B, n, d, dout, state_var, stream_ptr())
        if rc == -11:                             # the shape is beyond the plan (vjf_smooth_plan): nothing was launched
            raise NotImplementedError(N.lib().vjf_last_error().decode("utf-8", "replace"))
        N.check(rc, "vjf_smooth")
        return SmoothResult(mean, var, cov, (mean[0], cov0))

    def sample_posterior(self, q: Union[Gaussian, Tuple[Tensor, Tensor]], u: Tensor = None, n_sample: int = 16, *,
                         state_var: float = None, noise: Tensor = None, after: Tensor = None) -> PosteriorSamples:
        """`n_sample` joint draws per trial from the smoothed posterior of a filtered sequence as ONE C-ABI call (vjf_smooth_sample):
        backward sampling with the learned mean map and its Jacobian, the contract stated in include/vjf_hip.h.  Each row is
        conditioned on the draw of the row behind it; the gain and the factor of a row depend on the filtered row alone and are shared
        by the members.  The draws are exactly Gaussian: their row means and covariances are `smooth`'s, and whole trajectories carry
        the posterior's correlation across rows, which the marginals of `smooth` cannot.
        :param q, u, state_var: as `smooth` (a Gaussian or a (mu, logvar) pair of (T, B, xdim), a (T, xdim) pair is one trial; u the
            array that went into the filter, with `after` one row more; the default state_var reads one scalar from the device)
        :param n_sample: S, the draws per trial
        :param noise: (S, T, B, xdim) standard-normal values, used as they are.  Not given, they follow the owning model's `noise`:
            "device" is one torch.randn of that shape on the GPU, "reference" one randn of that shape on the CPU generator in the
            default dtype, so a seed fixes the draws
        :param after: (S, B, xdim), the draws of the row behind the last one, such as a previous result's `head`: drawing rows [k, T)
            first and rows [0, k) with after = that head (and the same noise rows) second gives the bits of one call
        :return: PosteriorSamples(x (S, T, B, xdim), head = x[:, 0]).  A trial with a non-finite input at some row has NaN in every
            member from that row back to row 0.
        Accepted wherever `smooth` is, xdim 25 to 31 beside fewer features included (its docstring has the limits; tested up to the
        last admitted n_rbf, tests/test_gpu_shape_range.py); the members go in as many chunks per tile as the LDS asks for.
        Reads the model's state and writes none; no scratch."""
        mu, lv = (q.mean, q.logvar) if isinstance(q, Gaussian) else q
        mu, lv = dev32(mu, ndim2=False), dev32(lv, ndim2=False)
        mu, lv = (t[:, None, :] if t.ndim == 2 else t for t in (mu, lv))        # (T, xdim): one trial
        assert mu.ndim == 3 and lv.shape == mu.shape, f"q is {tuple(mu.shape)} and {tuple(lv.shape)}, expected two (T, B, xdim)"
        mu, lv = mu.contiguous(), lv.contiguous()
        T, B, dout = mu.shape
        assert T >= 1, 'q must have at least one row'
        assert dout == self.velocity.n_output, f"q has {dout} columns, expected xdim={self.velocity.n_output}"
        S = int(n_sample)
        if S < 1:
            raise ValueError(f"n_sample must be at least 1, got {n_sample}")
        if dout > SM_MAX_XDIM:
            raise NotImplementedError(f"sample_posterior covers xdim <= {SM_MAX_XDIM}, this model has xdim = {dout}")
        state_var = float(self.logvar.exp()) if state_var is None else float(state_var)
        if not 0. < state_var < float('inf'):
            raise ValueError(f"state_var must be positive and finite, got {state_var}")
        if after is not None:
            after = dev32(after, ndim2=False)
            if after.ndim == 2 and B == 1:
                after = after[:, None, :]
            assert after.shape == (S, B, dout), f"after is {tuple(after.shape)}, expected {(S, B, dout)}"
            after = after.contiguous()
        if noise is None:
            if self._noise_mode() == "reference":
                noise = dev32(torch.randn(S, T, B, dout, dtype=torch.get_default_dtype()), ndim2=False)
            else:
                noise = torch.randn(S, T, B, dout, device=mu.device, dtype=torch.float32)
        else:
            noise = dev32(noise, ndim2=False)
            if noise.ndim == 3 and B == 1:
                noise = noise[:, :, None, :]
            assert noise.shape == (S, T, B, dout), f"noise is {tuple(noise.shape)}, expected {(S, T, B, dout)}"
            noise = noise.contiguous()
        vel = self.velocity
        n, d = vel.feature.centroid.shape
        rows = T + (after is not None)
        if d > dout and u is not None:
            u = dev32(u, ndim2=False)
            assert u.shape[0] == rows, f"u has {u.shape[0]} rows, expected {rows} (T{' + 1 with `after`' if after is not None else ''})"
        u = self._tangent_u(u, rows, B)
        x = torch.empty(S, T, B, dout, device=mu.device, dtype=torch.float32)
        rc = N.lib().vjf_smooth_sample(N.ptr(mu), N.ptr(lv), N.ptr(u), N.ptr(vel.feature.centroid), N.ptr(vel.feature.logwidth),
                                       N.ptr(vel.w_mean), N.ptr(noise), N.ptr(after), N.ptr(x), T, S, B, n, d, dout, state_var,
                                       stream_ptr())
        if rc == -11:                             # the shape is beyond the plan (vjf_smooth_sample_plan): nothing was launched
            raise NotImplementedError(N.lib().vjf_last_error().decode("utf-8", "replace"))
        N.check(rc, "vjf_smooth_sample")
        return PosteriorSamples(x, x[:, 0])

    def score_forecast(self, mu: Tensor, u: Tensor = None, n_step: int = 8, *, return_pred: bool = False) -> ForecastScore:
        """The k-step-ahead prediction error of the mean map over a filtered record as ONE C-ABI call (vjf_kstep_score; the contract
        and the summation order are stated in include/vjf_hip.h): from every row t the map x <- x + Phi([x, u]) w_mean is rolled
        h = 1 .. n_step steps from mu[t] and compared with mu[t + h], summed per horizon and column over the pairs with t + h inside
        the record, beside the same sums for persistence.
        :param mu: the filtered means (T, B, xdim) -- what `filter_sequence` / `fit` return; (T, xdim) is one trial
        :param u: (T, B, udim), the array that went into the filter (the step from row t to t + 1 reads u[t + 1]; u[0] is never read)
        :param return_pred: also return the predictions (n_step, T, B, xdim) -- for plots, not for large records
        :return: ForecastScore without the y fields.  The sums are deterministic, bit for bit, and depend on the order of the trials
            (not on the stream or the chunking).
        Asynchronous; reads the model's state and writes none.  The partial sums live in ONE bounded scratch tensor kept on this
        module (like `_fc_scratch`): run one call per model at a time."""
        return self._score_forecast(None, None, mu, None, u, n_step, return_pred)

    def _score_forecast(self, decoder, kind, mu, y, u, n_step, return_pred):
        K = int(n_step)
        if K < 1:
            raise ValueError(f"n_step must be at least 1, got {n_step}")
        mu = dev32(mu, ndim2=False)
        if mu.ndim == 2:
            mu = mu[:, None, :]                              # (T, xdim): one trial
        assert mu.ndim == 3, f"mu is {tuple(mu.shape)}, expected (T, B, xdim)"
        mu = mu.contiguous()
        T, B, dout = mu.shape
        assert T >= 1, 'mu must have at least one row'
        vel = self.velocity
        n, d = vel.feature.centroid.shape
        assert dout == vel.n_output, f"mu has {dout} columns, expected xdim={vel.n_output}"
        if d > dout and u is not None:
            u = dev32(u, ndim2=False)
            assert u.shape[0] == T, f"u has {u.shape[0]} rows, expected {T}"
        u = self._tangent_u(u, T, B)
        W = b = None
        dy = 0
        if y is not None:
            W, b = decoder.decode.weight, decoder.decode.bias
            dy = W.shape[0]
            y = dev32(y, ndim2=False)
            if y.ndim == 2 and B == 1:
                y = y[:, None, :]
            assert y.shape == (T, B, dy), f"y is {tuple(y.shape)}, expected {(T, B, dy)}"
            y = y.contiguous()
        else:
            kind = None
        L = N.lib()
        rc = L.vjf_kstep_score_plan(T, B, K, n, d, dout, dy, None, None, None, None)
        if rc == -11:                             # the shape is beyond one workgroup's LDS: nothing was launched
            raise NotImplementedError(L.vjf_last_error().decode("utf-8", "replace"))
        N.check(rc, "vjf_kstep_score_plan")
        self._ks_scratch = kept_scratch(self._ks_scratch, mu.device, L.vjf_kstep_score_scratch_size, T, B, K, dout, dy)
        new64 = lambda *shape: torch.empty(*shape, device=mu.device, dtype=torch.float64)    # noqa: E731
        sse_x, base_x = new64(K + 1, dout), new64(K + 1, dout)
        sse_y, base_y = (new64(K + 1, dy), new64(K + 1, dy)) if dy else (None, None)
        pred = torch.empty(K, T, B, dout, device=mu.device, dtype=torch.float32) if return_pred else None
        rc = L.vjf_kstep_score(N.ptr(mu), N.ptr(y), N.ptr(u), N.ptr(vel.feature.centroid), N.ptr(vel.feature.logwidth),
                               N.ptr(vel.w_mean), N.ptr(W), N.ptr(b), N.ptr(sse_x), N.ptr(base_x), N.ptr(sse_y), N.ptr(base_y),
                               N.ptr(pred), N.ptr(self._ks_scratch), T, B, K, n, d, dout, dy, int(kind == "poisson"), stream_ptr())
        if rc == -11:
            raise NotImplementedError(L.vjf_last_error().decode("utf-8", "replace"))
        N.check(rc, "vjf_kstep_score")
        cnt = (T - torch.arange(K + 1, device=mu.device)).clamp_(min=0) * B
        sst_y = _suffix_sst(y, K) if dy and kind != "poisson" else None
        return ForecastScore(cnt, sse_x, base_x, sse_y, base_y, _suffix_sst(mu, K), sst_y, pred, kind)

    def _record_args(self, decoder, y, u, prior_mean, prior_logvar, prior_cov, observed, what, max_xdim, variances):
        """What `_ekf` and `_laplace_filter` share: the coercions and the refusals of a record y, its control input, the prior of the
        row before row 0 and the `observed` flags; `variances`: (name, value) pairs that must be positive and finite.
        :return: y (T, B, ydim), u, prior_mean, prior_logvar, prior_cov, observed (uint8 or None)"""
        dy, dout = decoder.decode.weight.shape
        y = dev32(y, ndim2=False)
        if y.ndim == 2:
            y = y[:, None, :]                                # (T, ydim): one trial
        assert y.ndim == 3 and y.shape[2] == dy, f"y is {tuple(y.shape)}, expected (T, B, {dy})"
        y = y.contiguous()
        T, B = y.shape[:2]
        assert T >= 1, 'y must have at least one row'
        if dout > max_xdim:
            raise NotImplementedError(f"{what} covers xdim <= {max_xdim}, this model has xdim = {dout}")
        for name, v in variances:
            if not 0. < v < float('inf'):
                raise ValueError(f"{name} must be positive and finite, got {v}")
        prior_mean = dev32(prior_mean)
        assert prior_mean.shape == (B, dout), f"the prior mean is {tuple(prior_mean.shape)}, expected {(B, dout)}"
        if prior_cov is not None:
            prior_cov = dev32(prior_cov, ndim2=False)
            if prior_cov.ndim == 2:
                prior_cov = prior_cov[None]
            assert prior_cov.shape == (B, dout, dout), f"before[1] is {tuple(prior_cov.shape)}, expected {(B, dout, dout)}"
            prior_cov = prior_cov.contiguous()
        else:
            prior_logvar = dev32(prior_logvar)
            assert prior_logvar.shape == (B, dout), f"the prior log-variance is {tuple(prior_logvar.shape)}, expected {(B, dout)}"
        if observed is not None:
            observed = torch.as_tensor(observed)
            if observed.ndim == 1 and B == 1:
                observed = observed[:, None]
            assert observed.shape == (T, B), f"observed is {tuple(observed.shape)}, expected {(T, B)}"
            observed = (observed != 0).to(device=y.device, dtype=torch.uint8).contiguous()
        d = self.velocity.feature.centroid.shape[1]
        if d > dout and u is not None:
            u = dev32(u, ndim2=False)
            assert u.shape[0] == T, f"u has {u.shape[0]} rows, expected {T}"
        u = self._tangent_u(u, T, B)
        return y, u, prior_mean, prior_logvar, prior_cov, observed

    def _ekf(self, decoder, y, u, prior_mean, prior_logvar, prior_cov, state_var, obs_var, observed, return_cov):
        """VJF.ekf behind its choice of prior and variances: the coercions, the refusals and the one call (vjf_ekf)."""
        W, b = decoder.decode.weight, decoder.decode.bias
        dy, dout = W.shape
        y, u, prior_mean, prior_logvar, prior_cov, observed = self._record_args(
            decoder, y, u, prior_mean, prior_logvar, prior_cov, observed, "ekf", EKF_MAX_XDIM, (("state_var", state_var), ("obs_var", obs_var)))
        T, B = y.shape[:2]
        vel = self.velocity
        n, d = vel.feature.centroid.shape
        new = lambda *shape: torch.empty(*shape, device=y.device, dtype=torch.float32)       # noqa: E731
        mean, var, loglik, cov_last = new(T, B, dout), new(T, B, dout), new(T, B), new(B, dout, dout)
        cov = new(T, B, dout, dout) if return_cov else None
        rc = N.lib().vjf_ekf(N.ptr(y), N.ptr(u), N.ptr(observed), N.ptr(vel.feature.centroid), N.ptr(vel.feature.logwidth),
                             N.ptr(vel.w_mean), N.ptr(W), N.ptr(b), N.ptr(prior_mean), N.ptr(prior_logvar), N.ptr(prior_cov),
                             N.ptr(mean), N.ptr(var), N.ptr(cov), N.ptr(loglik), N.ptr(cov_last), T, B, n, d, dout, dy,
                             state_var, obs_var, stream_ptr())
        if rc == -11:                             # the shape is beyond the plan (vjf_ekf_plan): nothing was launched
            raise NotImplementedError(N.lib().vjf_last_error().decode("utf-8", "replace"))
        N.check(rc, "vjf_ekf")
        return EKFResult(mean, var, cov, loglik, (mean[-1], cov_last))

    def _laplace_filter(self, decoder, y, u, prior_mean, prior_logvar, prior_cov, state_var, observed, n_iter, return_cov):
        """VJF.laplace_filter behind its choice of prior and variance: the coercions, the refusals and the one call
        (vjf_laplace_filter)."""
        W, b = decoder.decode.weight, decoder.decode.bias
        dy, dout = W.shape
        if int(n_iter) != n_iter or not 1 <= n_iter <= LAPLACE_MAX_ITER:
            raise ValueError(f"n_iter must be an integer in 1 .. {LAPLACE_MAX_ITER}, got {n_iter}")
        y, u, prior_mean, prior_logvar, prior_cov, observed = self._record_args(
            decoder, y, u, prior_mean, prior_logvar, prior_cov, observed, "laplace_filter", LAPLACE_MAX_XDIM, (("state_var", state_var),))
        T, B = y.shape[:2]
        vel = self.velocity
        n, d = vel.feature.centroid.shape
        new = lambda *shape: torch.empty(*shape, device=y.device, dtype=torch.float32)       # noqa: E731
        mean, var, loglik, gnorm, cov_last = new(T, B, dout), new(T, B, dout), new(T, B), new(T, B), new(B, dout, dout)
        cov = new(T, B, dout, dout) if return_cov else None
        rc = N.lib().vjf_laplace_filter(N.ptr(y), N.ptr(u), N.ptr(observed), N.ptr(vel.feature.centroid), N.ptr(vel.feature.logwidth),
                                        N.ptr(vel.w_mean), N.ptr(W), N.ptr(b), N.ptr(prior_mean), N.ptr(prior_logvar),
                                        N.ptr(prior_cov), N.ptr(mean), N.ptr(var), N.ptr(cov), N.ptr(loglik), N.ptr(gnorm),
                                        N.ptr(cov_last), T, B, n, d, dout, dy, int(n_iter), state_var, stream_ptr())
        if rc == -11:                             # the shape is beyond the plan (vjf_laplace_filter_plan): nothing was launched
            raise NotImplementedError(N.lib().vjf_last_error().decode("utf-8", "replace"))
        N.check(rc, "vjf_laplace_filter")
        return LaplaceFilterResult(mean, var, cov, loglik, gnorm, (mean[-1], cov_last))

    @torch.no_grad()
    def update(self, xt: Tensor, xs: Tensor, ut: Tensor = None, *, warm_up=False):
        """Train regression, operator by operator (vjf/model.py:363-377).  VJF.filter does the same
        inside its fused step; this method serves direct callers."""
        xs, xt = dev32(xs), dev32(xt)
        xu = nonecat(xs, None if ut is None else dev32(ut))
        dx = xt - xs
        if not warm_up:
            self.velocity.rls(xu, dx, self.logvar.exp(), shrink=self.shrink)
        residual = dx - self.velocity(xu, sampling=False).mean
        mse = residual.pow(2).mean()
        var, n_sample = running_var(self.logvar.exp(), self.n_sample, mse, xs.shape[0], size_cap=500)
        self.logvar.copy_(var.log())
        self.n_sample = n_sample

    @torch.no_grad()
    def initialize(self, xt: Tensor, xs: Tensor, ut: Tensor = None):
        """vjf/model.py:379-388"""
        xs, xt = dev32(xs), dev32(xt)
        xu = nonecat(xs, None if ut is None else dev32(ut))
        mse = (xt - xs).pow(2).mean()
        self.velocity.initialize(xu, xt - xs, mse)
        d, V = self.velocity(xu, sampling=False)
        mse = (xt - xs - d).pow(2).mean()
        self.logvar.copy_(mse.log())

    def loss(self, pt, qt) -> Tensor:
        return gaussian_loss(pt, qt, self.logvar)


class VJF(Module):
    def __init__(self, ydim: int, xdim: int, likelihood: Module, transition: Module, recognition: Module,
                 *, lr: float = 1e-4, lr_decay: float = .9, noise: str = "reference", shrink: float = None):
        """
        Use VJF.make_model   (vjf/model.py:50-78)
        :param likelihood: GLM likelihood, Gaussian or Poisson
        :param transition: f(x[t-1], u[t]) -> x[t]
        :param recognition: y[t], f(x[t-1], u[t]) -> x[t]
        :param lr_decay: multiplicative factor of learning rate decay
        :param noise: "reference" (CPU generator, reference draw order) or "device"
        :param shrink: forgetting factor of the transition's RLS update, 0 < shrink <= 1 (`transition.shrink`; None keeps the
                       transition's own, which is 1 -- no forgetfulness, the reference's step -- unless it was built otherwise)
        """
        super().__init__()
        self.add_module('likelihood', likelihood)
        self.add_module('transition', transition)
        self.add_module('recognition', recognition)
        self.add_module('decoder', LinearDecoder(xdim, ydim))
        self.register_parameter('mean', Parameter(dev32(torch.zeros(xdim), ndim2=False), requires_grad=False))
        self.register_parameter('logvar', Parameter(dev32(torch.zeros(xdim), ndim2=False), requires_grad=False))
        self.optimizer = _ParamGroups(lr)
        self.scheduler = _ExponentialLR(self.optimizer, gamma=lr_decay)

        if noise not in ("reference", "device"):
            raise ValueError("noise must be 'reference' or 'device'")
        self.noise = noise
        if shrink is not None:
            transition.shrink = shrink
        self.ydim, self.xdim = ydim, xdim
        feat = transition.velocity.feature
        self.udim = feat.centroid.shape[1] - xdim
        self.n_rbf = feat.n_basis
        self.hidden_sizes = list(recognition.hidden_sizes)
        if isinstance(likelihood, GaussianLikelihood):
            self._lik = N.LIK_GAUSSIAN
        elif isinstance(likelihood, PoissonLikelihood):
            self._lik = N.LIK_POISSON
        else:
            raise TypeError("likelihood must be GaussianLikelihood or PoissonLikelihood")
        self._lib = None            # tests may inject a stand-in for the C ABI
        self._ctx = None
        self._ctx_batch = 0
        self._workspace = None
        self._pushed_lr = None
        self._adopt_state()

    # ------------------------------------------------------------------ device state
    def _backend(self):
        if self._lib is None:
            self._lib = N.lib()
        return self._lib

    def _config(self, max_batch):
        dev = torch.cuda.current_device() if torch.cuda.is_available() else 0
        return N.make_config(self.ydim, self.xdim, self.udim, self.n_rbf, self.hidden_sizes, self._lik, max_batch, dev)

    def _adopt_state(self):
        """Allocate the state blob and turn every module tensor into a view of it (include/vjf_hip.h, enum vjf_slot)."""
        n, off, size = N.state_layout(self._config(1))
        self._blob = torch.zeros(n, dtype=torch.float32, device=storage_device())

        def view(slot, shape):
            return self._blob[off[slot]:off[slot] + size[slot]].view(shape)

        vel, feat, rec = self.transition.velocity, self.transition.velocity.feature, self.recognition
        nr, dz, du, dy = self.n_rbf, self.xdim, self.udim, self.ydim
        rebind(self, 'mean', view(N.SLOT_PRIOR_MEAN, (dz,)))
        rebind(self, 'logvar', view(N.SLOT_PRIOR_LOGVAR, (dz,)))
        if self._lik == N.LIK_GAUSSIAN:
            rebind(self.likelihood, 'logvar', view(N.SLOT_LIK_LOGVAR, ()))
            object.__setattr__(self.likelihood, '_owner', weakref.ref(self))
        rebind(self.transition, 'logvar', view(N.SLOT_TR_LOGVAR, ()))
        object.__setattr__(self.transition, '_owner', weakref.ref(self))
        rebind(feat, 'centroid', view(N.SLOT_CENTROID, (nr, dz + du)))
        rebind(feat, 'logwidth', view(N.SLOT_LOGWIDTH, (nr,)))
        prev = dy + du + 2 * dz
        for k, lin in enumerate(rec.linears()):
            rebind(lin, 'weight', view(N.SLOT_REC_W0 + 2 * k, (self.hidden_sizes[k], prev)))
            rebind(lin, 'bias', view(N.SLOT_REC_B0 + 2 * k, (self.hidden_sizes[k],)))
            prev = self.hidden_sizes[k]
        rebind(rec.mean, 'weight', view(N.SLOT_MEAN_W, (dz, prev)))
        rebind(rec.logvar, 'weight', view(N.SLOT_LV_W, (dz, prev)))
        rebind(rec.logvar, 'bias', view(N.SLOT_LV_B, (dz,)))
        rebind(self.decoder.decode, 'weight', view(N.SLOT_DEC_W, (dy, dz)))
        rebind(self.decoder.decode, 'bias', view(N.SLOT_DEC_B, (dy,)))
        rebind(vel, 'w_mean', view(N.SLOT_W_MEAN, (nr, dz)))
        rebind(vel, 'w_chol', view(N.SLOT_W_CHOL, (nr, nr)))
        rebind(vel, 'w_precision', view(N.SLOT_W_PREC, (nr, nr)))
        rebind(vel, 'w_pchol', view(N.SLOT_W_PCHOL, (nr, nr)))
        self._scalars = self._blob[off[N.SLOT_SCALARS]:off[N.SLOT_SCALARS] + N.N_SCALARS]
        self._scalars[N.SC_N_LIK] = float(getattr(self.likelihood, "_n_sample", 0))
        self._scalars[N.SC_N_TR] = float(self.transition._n_sample)
        self._scalars[N.SC_SHRINK] = float(getattr(self.transition, "_shrink", 1.))
        self._push_lr(force=True)

    def _get_counter(self, which):
        return int(self._scalars[N.SC_N_LIK if which == "lik" else N.SC_N_TR].item())

    def _set_counter(self, which, v):
        self._scalars[N.SC_N_LIK if which == "lik" else N.SC_N_TR] = float(v)

    def _get_shrink(self):
        v = float(self._scalars[N.SC_SHRINK].item())
        return v if v != 0. else 1.                  # (a stored 0 reads as 1, on the device too: include/vjf_hip.h)

    def _set_shrink(self, v):
        self._scalars[N.SC_SHRINK] = float(v)

    def _push_lr(self, force=False):
        lrs = [float(g['lr']) for g in self.optimizer.param_groups]
        if force or lrs != self._pushed_lr:
            self._scalars[N.SC_LR_LIK:N.SC_LR_LIK + 4] = torch.tensor(lrs, dtype=torch.float32)
            self._pushed_lr = lrs

    def freeze_decoder(self, frozen: bool = True):
        """decoder.requires_grad_(False) of the reference (vjf/model.py:283)."""
        self._scalars[N.SC_FREEZE_DEC] = 1.0 if frozen else 0.0

    def set_overlap(self, enable: bool = True):
        """filter_sequence runs a step's RLS chain on a second stream beside the trial / SGD chain (default);
        False forces the one-stream order.  Results are bit-identical either way."""
        self._overlap = int(enable) if enable in (0, 1, 2, 3, True, False) else 1     # 3: the per-step three-stream route on one rank
        if self._ctx is not None:
            rc = self._backend().vjf_set_overlap(self._ctx, int(self._overlap))       # returns the resulting setting
            if rc < 0:
                N.check(rc, "vjf_set_overlap")

    def route(self, sgd: bool = True, update: bool = True, warm_up: bool = False) -> str:
        """The schedule `filter_sequence` would use now for this batch size: 'one-launch', 'streams' (three streams: the RCCL
        path), 'two-stream' (plans whose RLS update is a sequence of launches: that update beside the trial chain) or 'per-step'."""
        if self._ctx is None:
            return "unsized"
        rc = self._backend().vjf_route(self._ctx, (N.FLAG_SGD if sgd else 0) | (N.FLAG_UPDATE if update else 0)
                                       | (N.FLAG_WARM_UP if warm_up else 0))
        if rc < 0:
            N.check(rc, "vjf_route")
        return {1: "one-launch", 2: "two-stream", 3: "streams", 4: "packed"}.get(rc, "per-step")

    # ------------------------------------------------------------------ state I/O (the reference has no format)
    _RLS_KEYS = ("w_mean", "w_chol", "w_precision", "w_pchol")

    def get_state(self) -> dict:
        """Everything a run needs to resume, as numpy arrays: the 13 `state_dict` tensors, the RLS tensors of
        `transition.velocity` (plain attributes in the reference: vjf/module.py:45-54), the two sample counters, the
        four group learning rates, the decoder-freeze flag and the shape of the model -- and, where it is not 1, the forgetting
        factor of the RLS update as `"transition.shrink"`.  The format rule: an absent key means 1 (`set_state`), so a state at the
        default has the keys it had before the factor existed and older states load unchanged."""
        import numpy as np
        self.check_status()                  # (raises if a device-side wait of an earlier call timed out: that state is not one to keep)
        st = {k: v.detach().cpu().numpy().copy() for k, v in self.state_dict().items()}
        lr = self.transition.velocity
        for k in self._RLS_KEYS:
            st["transition.velocity." + k] = getattr(lr, k).detach().cpu().numpy().copy()
        st["likelihood.n_sample"] = np.int64(self._get_counter("lik"))
        st["transition.n_sample"] = np.int64(self._get_counter("tr"))
        if self._get_shrink() != 1.:         # (1, no forgetting, is what a state without the key means: such a state keeps the
            st["transition.shrink"] = np.float64(self._get_shrink())                     #  format it had before the factor)
        st["optimizer.lr"] = np.array([float(g["lr"]) for g in self.optimizer.param_groups], np.float64)
        st["decoder.frozen"] = np.int64(int(self._scalars[N.SC_FREEZE_DEC].item() != 0))
        st["config"] = np.array([self.ydim, self.xdim, self.udim, self.n_rbf, self._lik] + list(self.hidden_sizes), np.int64)
        return st

    def set_state(self, st: dict):
        """Inverse of `get_state` (same model shape required).  Clears the sticky status bits and marks `w_chol` /
        `w_pchol` as possibly dense, so the first RLS update re-establishes their triangles."""
        import numpy as np
        cfg = [int(v) for v in np.asarray(st["config"]).tolist()]
        mine = [self.ydim, self.xdim, self.udim, self.n_rbf, self._lik] + list(self.hidden_sizes)
        if cfg != mine:
            raise ValueError(f"state is for a model of shape {cfg}, this one is {mine}")
        shrink = float(st["transition.shrink"]) if "transition.shrink" in st else 1.   # (a state from before the key: no forgetting)
        if not 0. < shrink <= 1.:
            raise ValueError(f"shrink must be in (0, 1], got {shrink}")
        own = self.state_dict()
        with torch.no_grad():
            for k, v in own.items():
                v.copy_(torch.as_tensor(np.asarray(st[k]), dtype=torch.float32).reshape(v.shape))
            lr = self.transition.velocity
            for k in self._RLS_KEYS:
                t = getattr(lr, k)
                t.copy_(torch.as_tensor(np.asarray(st["transition.velocity." + k]), dtype=torch.float32).reshape(t.shape))
        self._set_counter("lik", int(st["likelihood.n_sample"]))
        self._set_counter("tr", int(st["transition.n_sample"]))
        self.transition.shrink = shrink
        for g, v in zip(self.optimizer.param_groups, np.asarray(st["optimizer.lr"]).tolist()):
            g["lr"] = float(v)
        self._push_lr(force=True)
        self.freeze_decoder(bool(int(st["decoder.frozen"])))
        self._scalars[N.SC_TRI_CLEAN] = 0.0
        self._scalars[N.SC_STATUS] = 0.0

    def save_state(self, path):
        import numpy as np
        np.savez(path, **self.get_state())

    def load_state(self, path):
        import numpy as np
        with np.load(path) as z:
            self.set_state({k: z[k] for k in z.files})

    def status(self) -> int:
        """Sticky VJF_STATUS_* bits raised by the device since the last call (clears them)."""
        if self._ctx is None:
            return 0
        s = ctypes.c_uint32()
        N.check(self._backend().vjf_get_status(self._ctx, ctypes.byref(s)), "vjf_get_status")
        return s.value

    def _ensure_ctx(self, B):
        if self._ctx is not None and B <= self._ctx_batch:
            return
        L = self._backend()
        if self._ctx is not None:
            torch.cuda.synchronize() if torch.cuda.is_available() else None
            L.vjf_ctx_destroy(self._ctx)
            self._ctx = None
        cfg = self._config(B)
        nbytes = ctypes.c_int64()
        N.check(L.vjf_workspace_size(ctypes.byref(cfg), ctypes.byref(nbytes)), "vjf_workspace_size")
        self._workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=self._blob.device)
        poison = os.environ.get("VJF_DEBUG_POISON_WS")         # (tests: a workspace of NaNs / of a byte pattern shows any read of a
        if poison:                                             #  region the library has not written)
            self._workspace.fill_(int(poison, 0) & 0xFF)
        ctx = ctypes.c_void_p()
        N.check(L.vjf_ctx_create(ctypes.byref(cfg), N.ptr(self._blob), N.ptr(self._workspace), nbytes.value, stream_ptr(),
                                 ctypes.byref(ctx)), "vjf_ctx_create")
        self._ctx, self._ctx_batch = ctx, B
        _LIVE.add(self)
        act = getattr(self.recognition, "act_code", (N.ACT_TANH, 0.0, 0.0))
        if act[0] != N.ACT_TANH:                               # (another activation than the reference's default: the act kernels)
            N.check(L.vjf_set_activation(ctx, ctypes.byref(N.VjfActivation(*act))), "vjf_set_activation")
        if getattr(self, "_collectives", 2) != 2:
            N.check(L.vjf_set_collectives(ctx, int(self._collectives)), "vjf_set_collectives")
        if getattr(self, "_overlap", 1) != 1:
            rc = L.vjf_set_overlap(ctx, int(self._overlap))
            if rc < 0:
                N.check(rc, "vjf_set_overlap")
        p, n = ctypes.c_void_p(), ctypes.c_int64()
        N.check(L.vjf_reduce_buffer(ctx, ctypes.byref(p), ctypes.byref(n)), "vjf_reduce_buffer")
        o = p.value - self._workspace.data_ptr()
        self._reduce = self._workspace[o:o + 4 * n.value].view(torch.float32)

    def close(self):
        """Destroy the native context (its streams are synchronised first; RCCL communicators and the extra streams of the sharded
        route are released).  The model stays usable: the next call makes a new context.  Called for every live model at
        interpreter exit, before the HIP runtime's own exit handlers."""
        ctx, self._ctx = self._ctx, None
        self._ctx_batch = 0
        if ctx is not None and self._lib is not None:
            self._lib.vjf_ctx_destroy(ctx)

    def __del__(self):
        if sys.is_finalizing():               # (no native call at interpreter shutdown: `_close_all` has run)
            return
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ noise
    def _draw(self, shape):
        """One reparametrisation draw.  "reference": torch.randn on the CPU generator in the default
        dtype == randn_like(mean) of vjf/util.py:13 for the contiguous means filter produces."""
        if self.noise == "reference":
            return torch.randn(shape, dtype=torch.get_default_dtype()).to(self._blob.device, torch.float32)
        return torch.randn(shape, device=self._blob.device, dtype=torch.float32)

    @staticmethod
    def _world():
        import os
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            w = dist.get_world_size()
            # VJF_FORCE_DIST=1: take the sharded path (local half -> all-reduce -> global half) even with one rank, so that it
            # can be exercised on a single GPU
            return (w, True) if (w > 1 or os.environ.get("VJF_FORCE_DIST") == "1") else (1, False)
        return 1, False

    @staticmethod
    def _all_reduce_sum(t: Tensor):
        """Sum over ranks, in place.  A gloo group (several ranks sharing one GPU in tests, or a CPU control plane) gets the
        buffer through the host; RCCL takes the device tensor as it is."""
        import torch.distributed as dist
        if dist.get_backend() == "gloo" and t.is_cuda:
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            t.copy_(h)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)

    def _native_comm(self, world) -> bool:
        """RCCL communicators inside the context (collective over the ranks; once per context).  False -> the caller keeps
        the all-reduce on its side (vjf_filter_local / torch.distributed.all_reduce / vjf_filter_global)."""
        import os
        import torch.distributed as dist
        if getattr(self, "_comm_ctx", None) is self._ctx:
            return self._comm_ok
        self._comm_ctx, self._comm_ok = self._ctx, False
        L = self._backend()
        ids = (ctypes.c_char * 256)()
        ok = (os.environ.get("VJF_NATIVE_RCCL", "1") != "0" and self._overlap_flag() and L.vjf_set_overlap(self._ctx, int(getattr(self, "_overlap", 1))) >= 1
              and L.vjf_comm_unique_id(ids) == 0)
        # (control plane only: with a gloo group the two exchanges go through host tensors and no collective stream of
        #  torch's is created beside the four of vjf_filter_seq)
        cdev = "cpu" if dist.get_backend() == "gloo" else self._blob.device
        flag = torch.tensor([1 if ok else 0], device=cdev, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)                 # every rank takes the same route
        if int(flag.item()) == 0:
            return False
        t = torch.frombuffer(bytearray(bytes(ids)), dtype=torch.uint8).to(cdev)
        dist.broadcast(t, src=0)
        buf = (ctypes.c_char * 256).from_buffer_copy(t.cpu().numpy().tobytes())
        N.check(L.vjf_comm_init(self._ctx, buf, dist.get_rank(), world), "vjf_comm_init")
        self._comm_ok = True
        return True

    def set_collectives(self, per_step: int = 2):
        """Sums over ranks per step on the in-library RCCL route: 2 (two all-reduces on two overlapping chains, default) or 1 (the
        whole reduce buffer in one).  Takes effect from the next call."""
        if per_step not in (1, 2):
            raise ValueError("per_step must be 1 or 2")
        self._collectives = per_step
        if self._ctx is not None:
            N.check(self._backend().vjf_set_collectives(self._ctx, per_step), "vjf_set_collectives")

    def comm_ranks(self):
        """[ranks of the gradient chain's communicator, of the statistics chain's] as RCCL reports them (ncclCommCount);
        [0, 0] when the context has none (single rank, or the sums over ranks on the caller's side)."""
        if self._ctx is None:
            return [0, 0]
        r = (ctypes.c_int32 * 2)()
        N.check(self._backend().vjf_comm_ranks(self._ctx, r), "vjf_comm_ranks")
        return [int(r[0]), int(r[1])]

    def _overlap_flag(self) -> bool:
        return bool(getattr(self, "_overlap", 1))

    # Trials sharded over ranks: True replays a step whose loss has a non-finite component exactly as the reference defines it
    # (vjf/model.py:138-149) at the price of a second sum over ranks in every step; False (default) skips such a step's SGD update
    # and raises the status bit.  One rank always replays (include/vjf_hip.h, VJF_FLAG_EXACT_NONFINITE).
    exact_nonfinite = False

    def _flags(self, sgd, update, warm_up):
        return ((N.FLAG_SGD if sgd else 0) | (N.FLAG_UPDATE if update else 0) | (N.FLAG_WARM_UP if warm_up else 0)
                | (N.FLAG_EXACT_NONFINITE if self.exact_nonfinite else 0))

    # ------------------------------------------------------------------ operator-level API (reference structure)
    def prior(self, y: Tensor) -> Gaussian:
        """vjf/model.py:80-95"""
        assert y.ndim == 2
        n_batch = y.shape[0]
        one = torch.ones(n_batch, self.xdim, device=self._blob.device)
        return Gaussian(one * torch.atleast_2d(self.mean), one * torch.atleast_2d(self.logvar))

    def forward(self, y: Tensor, qs: Gaussian, u: Tensor = None, *, eps=None) -> Tuple:
        """encode / predict / decode, one operator at a time (vjf/model.py:97-122).
        :return: xs, pt, qt, xt, py"""
        y = dev32(y)
        qs = self.prior(y) if qs is None else detach(Gaussian(dev32(qs.mean), dev32(qs.logvar)))
        e1, e2 = (None, None) if eps is None else (dev32(eps[0]), dev32(eps[1]))
        xs = reparametrize(qs, e1 if e1 is not None else self._draw(qs.mean.shape))
        pt = self.transition(xs, u, sampling=False)
        qt = self.recognition(y, qs, u)
        xt = reparametrize(qt, e2 if e2 is not None else self._draw(qt.mean.shape))
        py = self.decoder(xt)
        return xs, pt, qt, xt, py

    def loss(self, y: Tensor, xs: Tensor, pt, qt: Gaussian, xt: Tensor, py: Tensor,
             components: bool = False, warm_up: bool = False):
        """vjf/model.py:124-154"""
        l_recon = self.likelihood.loss(py, dev32(y))
        l_dynamics = self.transition.loss(pt, qt)
        h = entropy(qt)
        zero = torch.zeros((), device=l_recon.device)
        if not torch.isfinite(l_recon):
            l_recon = zero
        if not torch.isfinite(l_dynamics):
            l_dynamics = zero
        if not torch.isfinite(h):
            h = zero
        loss = l_recon - h
        if not warm_up:
            loss = loss + l_dynamics
        if components:
            return loss, -l_recon, -l_dynamics, h
        return loss

    @torch.no_grad()
    def update(self, y: Tensor, xs: Tensor, u: Tensor, pt, qt: Gaussian, xt: Tensor, py: Tensor, *,
               likelhood=True, decoder=True, transition=True, recognition=True, warm_up=False):
        """Learning without gradient (vjf/model.py:156-177)"""
        if likelhood:
            self.likelihood.update(py, y)
        if transition:
            self.transition.update(xt, xs, u, warm_up=warm_up)

    # ------------------------------------------------------------------ the hot path
    def filter(self, y: Tensor, u: Tensor = None, qs: Gaussian = None, *,
               sgd: bool = True, update: bool = True, verbose: bool = False, warm_up: bool = False, eps=None):
        """
        Filter a step   (vjf/model.py:179-221) -- one fused device step for the whole batch of trials.
        :param y: observation (batch, dim); a missing batch axis is prepended.
        :param u: control
        :param qs: previous posterior. use prior if None.
        :param sgd: flag to enable gradient step
        :param update: flag to update DS
        :param verbose: verbose output
        :param warm_up: do not learn dynamics if True, default=False
        :param eps: optional (eps_s, eps_t) noise, each (batch, xdim); drawn if None
        (Asynchronous, like `filter_sequence`: the device's status word -- 'RLS failed.', a timed-out hand-off -- is read by
        `check_status()`, which a caller runs before relying on the outputs or the state; `fit`, `get_state`, `save_state` do.)
        :return:
            qt: posterior
            loss: negative elbo   [, -l_recon, -l_dynamics, entropy if verbose]
        """
        y = dev32(y)
        if y.shape[1] != self.ydim:
            raise AssertionError(f"y has {y.shape[1]} columns, expected ydim={self.ydim}")
        B = y.shape[0]
        if self.udim > 0:
            if u is None:
                raise TypeError("u is required when udim > 0")
            u = dev32(u)
            assert u.shape == (B, self.udim)
        else:
            u = None
        if qs is None:
            mu_s = lv_s = None
        else:
            mu_s, lv_s = dev32(qs.mean), dev32(qs.logvar)
            assert mu_s.shape == (B, self.xdim) and lv_s.shape == (B, self.xdim)
        if eps is None:
            eps_s = self._draw((B, self.xdim))
            eps_t = self._draw((B, self.xdim))
        else:
            eps_s, eps_t = dev32(eps[0]), dev32(eps[1])
            assert eps_s.shape == (B, self.xdim) and eps_t.shape == (B, self.xdim)
        self._ensure_ctx(B)
        self._push_lr()
        L = self._backend()
        dev = self._blob.device
        mu_t = torch.empty(B, self.xdim, device=dev, dtype=torch.float32)
        lv_t = torch.empty(B, self.xdim, device=dev, dtype=torch.float32)
        loss4 = torch.empty(4, device=dev, dtype=torch.float32)
        flags = self._flags(sgd, update, warm_up)
        L.vjf_set_stream(self._ctx, stream_ptr())
        world, sharded = self._world()
        if not sharded:
            N.check(L.vjf_filter_step(self._ctx, B, N.ptr(y), N.ptr(u), N.ptr(mu_s), N.ptr(lv_s), N.ptr(eps_s), N.ptr(eps_t),
                                      N.ptr(mu_t), N.ptr(lv_t), N.ptr(loss4), flags), "vjf_filter_step")
        else:
            import torch.distributed as dist
            N.check(L.vjf_filter_local(self._ctx, B, N.ptr(y), N.ptr(u), N.ptr(mu_s), N.ptr(lv_s), N.ptr(eps_s), N.ptr(eps_t),
                                       N.ptr(mu_t), N.ptr(lv_t), flags), "vjf_filter_local")
            self._all_reduce_sum(self._reduce)                        # the ONE collective of a step
            N.check(L.vjf_filter_global(self._ctx, B * world, N.ptr(loss4), flags), "vjf_filter_global")
        if update and not warm_up:
            if not self.transition.velocity._w_colmajor:     # (nn.Module.__setattr__ costs 2.5 us: only when it changes)
                self.transition.velocity._w_colmajor = True  # see LinearRegression._draw_weight_noise
        qt = Gaussian(mu_t, lv_t)
        if verbose:
            return qt, loss4[0], loss4[1], loss4[2], loss4[3]
        return qt, loss4[0]

    feed = filter      # the north-star's name for one step; the reference itself has no `feed`

    def filter_sequence(self, y: Tensor, u: Tensor = None, qs: Gaussian = None, *, sgd: bool = True, update: bool = True,
                        warm_up: bool = False, eps: Tensor = None):
        """T successive `filter` steps in one C-ABI call (the inner loop of fit, vjf/model.py:252-261).
        y (T,B,ydim); u (T,B,udim) or None; eps (T,2,B,xdim) or None (drawn in the reference's order).
        :return: mu (T,B,xdim), logvar (T,B,xdim), loss (T,4) = [loss, -l_recon, -l_dynamics, entropy]

        The call is ASYNCHRONOUS and does not read the device's status word.  **Call `check_status()` before you rely on the
        outputs or on the model's state**: it warns 'RLS failed.' as the reference does, and RAISES when a hand-off inside the
        launch timed out (compute units held by another process for seconds: the outputs and the SGD / RLS state of that call are
        then not valid -- restore from `get_state()` of an earlier point and run again).  `fit` does this after every sequence;
        `get_state` / `save_state` do it before they copy anything."""
        y = dev32(y, ndim2=False)
        assert y.ndim == 3 and y.shape[2] == self.ydim
        T, B = y.shape[:2]
        u = dev32(u, ndim2=False) if (u is not None and self.udim > 0) else None
        if self.udim > 0 and u is None:
            raise TypeError("u is required when udim > 0")
        if eps is None:
            if self.noise == "reference":      # per step: xs draw then xt draw, each its own randn call
                eps = torch.stack([torch.stack([torch.randn(B, self.xdim, dtype=torch.get_default_dtype()) for _ in range(2)])
                                   for _ in range(T)])
            else:
                eps = torch.randn(T, 2, B, self.xdim, device=self._blob.device)
        eps = dev32(eps, ndim2=False)
        assert eps.shape == (T, 2, B, self.xdim)
        mu0 = lv0 = None
        if qs is not None:
            mu0, lv0 = dev32(qs.mean), dev32(qs.logvar)
        self._ensure_ctx(B)
        self._push_lr()
        L = self._backend()
        dev = self._blob.device
        # (one allocation for the three outputs: the call's host time is what a short sequence pays per step)
        nz = T * B * self.xdim
        out = torch.empty(2 * nz + 4 * T, device=dev, dtype=torch.float32)
        st3 = (B * self.xdim, self.xdim, 1)                     # (as_strided: a third of the host time of slice + view)
        mu, lv, loss = out.as_strided((T, B, self.xdim), st3, 0), out.as_strided((T, B, self.xdim), st3, nz), out.as_strided((T, 4), (4, 1), 2 * nz)
        flags = self._flags(sgd, update, warm_up)
        L.vjf_set_stream(self._ctx, stream_ptr())
        world, sharded = self._world()
        if not sharded or ((getattr(self, "_collectives", 2) == 1 or (update and not warm_up and T > 1)) and self._native_comm(world)):
            # one C-ABI call for the whole sequence; with ranks, the library sums statistics and gradients over them itself
            N.check(L.vjf_filter_seq(self._ctx, T, B, N.ptr(y), N.ptr(u), N.ptr(eps), N.ptr(mu0), N.ptr(lv0), N.ptr(mu), N.ptr(lv),
                                     N.ptr(loss), flags), "vjf_filter_seq")
        else:
            import torch.distributed as dist
            ms, ls = mu0, lv0
            for t in range(T):
                N.check(L.vjf_filter_local(self._ctx, B, N.ptr(y[t]), N.ptr(None if u is None else u[t]), N.ptr(ms), N.ptr(ls),
                                           N.ptr(eps[t, 0]), N.ptr(eps[t, 1]), N.ptr(mu[t]), N.ptr(lv[t]), flags), "vjf_filter_local")
                self._all_reduce_sum(self._reduce)
                N.check(L.vjf_filter_global(self._ctx, B * world, N.ptr(loss[t]), flags), "vjf_filter_global")
                ms, ls = mu[t], lv[t]
        if update and not warm_up and not self.transition.velocity._w_colmajor:
            self.transition.velocity._w_colmajor = True
        return mu, lv, loss

    # sticky status bits that mean "the results of the call are not to be used" (include/vjf_hip.h: VJF_STATUS_WAIT_*)
    _WAIT_BITS = 0x3ff00

    def check_status(self) -> int:
        """Read (and clear) the device's sticky status word -- one host synchronisation.  'RLS failed.' is warned about as the
        reference does from LinearRegression.rls (vjf/module.py:112); a hand-off time-out inside a launch raises."""
        import warnings
        st = self.status()
        if st & self._WAIT_BITS:
            raise RuntimeError(f"vjf: a device-side wait timed out (status 0x{st:x}); the outputs of the call are not valid")
        if st & N.STATUS_RLS_FAILED:
            warnings.warn('RLS failed.')
        return st

    # ------------------------------------------------------------------ harness
    def fit(self, y: Tensor, u: Tensor = None, *,
            max_iter: int = 200, beta: float = 0.1, verbose: bool = False, rtol: float = 1e-4):
        """
        vjf/model.py:223-307: epochs over the time axis with warm-up, decoder freeze, RBF
        re-initialisation, convergence test and per-epoch learning-rate decay.  Each epoch is one
        `filter_sequence` call.
        :param y: observation, (time, ..., dim)
        :param u: control input, None if autonomous
        :return: mu (time, batch, xdim), logvar (time, batch, xdim), epoch_loss
        """
        y = dev32(y)
        if y.ndim == 2:
            y = y[:, None, :]                    # (time, dim): every step is a batch of one trial
        if u is not None and self.udim > 0:
            u_ = dev32(u)
            if u_.ndim == 2:
                u_ = u_[:, None, :]
        else:
            u_ = None
        T = y.shape[0]

        warm_up = True
        epoch_loss = torch.tensor(float('nan'))
        mu = lv = None
        with trange(max_iter) as progress:
            running_loss = torch.tensor(float('nan'))
            for i in progress:
                mu, lv, losses = self.filter_sequence(y, u_, None, sgd=True, update=True, warm_up=warm_up)
                losses = losses.detach().cpu().to(torch.get_default_dtype())
                self.check_status()                  # (the copy above has synchronised the stream already)
                epoch_loss = losses[:, 0].sum() / T
                if verbose:
                    progress.set_postfix({'Loss': running_loss.item(), 'Recon': losses[-1, 1].item(),
                                          'Dynamics': losses[-1, 2].item(), 'Entropy': losses[-1, 3].item()})
                if warm_up:
                    if epoch_loss.isclose(running_loss, rtol=rtol):
                        warm_up = False
                        running_loss = epoch_loss
                        print('\nWarm up stopped.\n')
                        self.freeze_decoder(True)                    # freeze decoder after warm up
                        m = mu
                        if u_ is not None:
                            u_init = u_[1:].reshape(-1, u_.shape[-1])
                        else:
                            u_init = None
                        self.transition.initialize(m[1:].reshape(-1, m.shape[-1]),
                                                   m[:-1].reshape(-1, m.shape[-1]),
                                                   u_init)
                else:
                    if epoch_loss.isclose(running_loss, rtol=rtol):
                        print('\nConverged.\n')
                        break
                running_loss = beta * running_loss + (1 - beta) * epoch_loss if i > 0 else epoch_loss
                progress.set_postfix({'Loss': running_loss.item()})
                self.scheduler.step()
        return mu, lv, epoch_loss

    @classmethod
    def make_model(cls, ydim: int, xdim: int, udim: int, n_rbf: int, hidden_sizes: Sequence[int],
                   likelihood: str = 'poisson', *args, **kwargs):
        """vjf/model.py:309-319 -- same construction (and RNG consumption) order as the reference."""
        if likelihood.lower() == 'poisson':
            likelihood = PoissonLikelihood()
        elif likelihood.lower() == 'gaussian':
            likelihood = GaussianLikelihood()
        model = VJF(ydim, xdim, likelihood, RBFDS(n_rbf, xdim, udim), Recognition(ydim, xdim, udim, hidden_sizes),
                    *args, **kwargs)
        return model

    def forecast(self, x0: Tensor, u: Tensor = None, n_step: int = 1, *, noise: bool = False) -> Tuple[Tensor, Tensor]:
        """vjf/model.py:321-324"""
        x = self.transition.forecast(x0, u, n_step, noise=noise)
        y = self.decoder(x)
        return x, y

    def forecast_sequence(self, x0: Tensor, u: Tensor = None, n_step: int = 1, *, noise: bool = False,
                          w_noise: Tensor = None, state_noise: Tensor = None) -> Tuple[Tensor, Tensor]:
        """`forecast` with the whole horizon in one native call (RBFDS.forecast_sequence), then one decoding of all rows.
        :return: x (n_step + 1, B, xdim), y (n_step + 1, B, ydim)"""
        x = self.transition.forecast_sequence(x0, u, n_step, noise=noise, w_noise=w_noise, state_noise=state_noise)
        y = self.decoder(x)
        return x, y

    def forecast_ensemble(self, x0: Union[Tensor, Gaussian], u: Tensor = None, n_step: int = 1, n_sample: int = 16, *,
                          noise: bool = False, w_noise: Tensor = None, state_noise: Tensor = None, x0_noise: Tensor = None,
                          return_members: bool = False) -> ForecastEnsemble:
        """Forecast with uncertainty: `n_sample` sampled roll-outs of the whole horizon in one native call, reduced to the per-step
        mean and population variance of the latent state x and of y (RBFDS.forecast_ensemble has the arguments and the draw order).
        y is the decoder's output, exactly what `forecast` returns as y, for both likelihoods: under the Poisson likelihood it is the
        linear predictor (the log rate), not the rate.  Every member is decoded on chip; no (S, n_step + 1, B, ydim) array is formed.
        :return: ForecastEnsemble(x_mean, x_var (n_step + 1, B, xdim), y_mean, y_var (n_step + 1, B, ydim),
                 x (S, n_step + 1, B, xdim) if `return_members` else None)"""
        return ForecastEnsemble(*self.transition._forecast_ensemble(self.decoder, x0, u, n_step, n_sample, noise, w_noise, state_noise,
                                                                    x0_noise, return_members))

    def jacobian(self, x: Union[Tensor, Gaussian], u: Tensor = None) -> Tensor:
        """The Jacobian of the learned mean map at `x` (RBFDS.jacobian); a Gaussian stands for its mean, e.g. the last posterior.
        :return: (B, xdim, xdim), J[b, i, j] = d f_i / d x_j"""
        return self.transition.jacobian(x.mean if isinstance(x, Gaussian) else x, u)

    def lyapunov(self, x0: Union[Tensor, Gaussian], u: Tensor = None, n_step: int = 1, *, n_exponent: int = None, qr_every: int = 1,
                 q0: Tensor = None, burn_in: int = 0, dt: float = 1.0, return_history: bool = False) -> LyapunovResult:
        """The Lyapunov spectrum of the learned mean map from `x0` in one native call (RBFDS.lyapunov has the arguments and what
        the columns mean); a Gaussian stands for its mean, e.g. the last posterior `filter` returned."""
        return self.transition.lyapunov(x0.mean if isinstance(x0, Gaussian) else x0, u, n_step, n_exponent=n_exponent,
                                        qr_every=qr_every, q0=q0, burn_in=burn_in, dt=dt, return_history=return_history)

    def fixed_points(self, x0: Union[Tensor, Gaussian], u: Tensor = None, *, max_iter: int = 64, tol: float = 1e-5,
                     damping: float = 1e-3, return_jacobian: bool = True) -> FixedPointResult:
        """The fixed points of the learned mean map reached from the starts `x0` in one native call (RBFDS.fixed_points has the
        arguments); a Gaussian stands for its mean, e.g. the last posterior `filter` returned."""
        return self.transition.fixed_points(x0.mean if isinstance(x0, Gaussian) else x0, u, max_iter=max_iter, tol=tol,
                                            damping=damping, return_jacobian=return_jacobian)

    def smooth(self, q: Union[Gaussian, Tuple[Tensor, Tensor]], u: Tensor = None, *, state_var: float = None,
               after: Tuple[Tensor, Tensor] = None, return_cov: bool = False) -> SmoothResult:
        """The smoothed posterior q(x_t | y_1..T) of a filtered sequence -- what `filter_sequence` / `fit` returned -- in one native
        call (RBFDS.smooth has the arguments); `model.decoder(res.gaussian().mean)` gives the smoothed observations."""
        return self.transition.smooth(q, u, state_var=state_var, after=after, return_cov=return_cov)

    def ekf(self, y: Tensor, u: Tensor = None, *, x0: Gaussian = None, before: Tuple[Tensor, Tensor] = None, state_var: float = None,
            obs_var: float = None, observed: Tensor = None, return_cov: bool = False) -> EKFResult:
        """The extended Kalman filter of the learned generative model over a record as ONE C-ABI call (vjf_ekf; the contract is
        stated in include/vjf_hip.h): the mean map and its Jacobian, the state noise, the linear decoder and the Gaussian
        observation noise -- no recognition network.  It returns the filtered posterior with its full covariance and, row by row, the
        model evidence log p(y_t | y_1..t-1), and it steps over rows that were not observed.
        :param y: (T, B, ydim); (T, ydim) is one trial
        :param u: (T, B, udim): u[t] drives the transition INTO row t, as in `filter`; row 0 is predicted from the prior with u[0]
        :param x0: the prior of the row before row 0: None (the model's `prior`) or a Gaussian of (B, xdim)
        :param before: (mean (B, xdim), cov (B, xdim, xdim)) in x0's place, such as a previous result's `head`: rows [0, k) first and
            rows [k, T) with before = that head second give the bits of one call.  Giving both x0 and before is a ValueError
        :param state_var: the scalar state-noise variance, default exp(transition.logvar);  obs_var: the scalar observation variance,
            default exp(likelihood.logvar).  Reading a default copies one scalar to the host, which synchronises the stream; pass
            floats to stay asynchronous
        :param observed: (T, B) of booleans or 0 / 1, None: every row.  A row that is not observed is predicted only (its loglik is 0)
            and its y is never used: it may hold NaN
        :param return_cov: also return the full covariances of every row
        :return: EKFResult(mean, var (T, B, xdim), cov (T, B, xdim, xdim) or None, loglik (T, B), head = (mean[-1], cov of the last
            row)); `.gaussian()` is the diagonal posterior `smooth` takes (which then treats the filtered covariance as diagonal),
            `.log_likelihood()` the evidence per trial.  A trial with a non-finite observed y, u or prior at some row, or a prior
            covariance that is not positive definite, has NaN from that row on.
        Every xdim <= 24 with n_rbf <= 256 and udim <= 8 is accepted whatever ydim is.  Beyond it the shape has to fit one
        workgroup's LDS: without a control input n_rbf <= 461 at xdim = 24, 344 at 25 and 96 at 27 (eight control inputs take 7 or 8
        off); xdim >= 28 never fits.  What does not fit raises NotImplementedError naming the limit before anything is launched.
        These shapes are tested up to the last admitted n_rbf (tests/test_gpu_shape_range.py).
        Under the Poisson likelihood this raises NotImplementedError: the update is the Gaussian one; `laplace_filter` is the
        filter of a Poisson model.  Reads the model's state and writes none; no scratch."""
        if isinstance(self.likelihood, PoissonLikelihood):
            raise NotImplementedError("ekf needs the Gaussian likelihood: under the Poisson likelihood the update is not Gaussian "
                                      "(use laplace_filter)")
        if x0 is not None and before is not None:
            raise ValueError("give x0 (a diagonal Gaussian) or before (mean, cov), not both")
        y = dev32(y, ndim2=False)
        B = 1 if y.ndim == 2 else y.shape[1]
        p_mean = p_lv = p_cov = None
        if before is not None:
            p_mean, p_cov = before
        elif x0 is not None:
            p_mean, p_lv = x0.mean, x0.logvar
        else:
            one = torch.ones(B, self.xdim, device=self._blob.device)
            p_mean, p_lv = one * torch.atleast_2d(self.mean), one * torch.atleast_2d(self.logvar)
        state_var = float(self.transition.logvar.exp()) if state_var is None else float(state_var)
        obs_var = float(self.likelihood.logvar.exp()) if obs_var is None else float(obs_var)
        return self.transition._ekf(self.decoder, y, u, p_mean, p_lv, p_cov, state_var, obs_var, observed, return_cov)

    def laplace_filter(self, y: Tensor, u: Tensor = None, *, x0: Gaussian = None, before: Tuple[Tensor, Tensor] = None,
                       state_var: float = None, observed: Tensor = None, n_iter: int = 8,
                       return_cov: bool = False) -> LaplaceFilterResult:
        """The filter of the learned generative model with count observations over a record as ONE C-ABI call (vjf_laplace_filter;
        the contract is stated in include/vjf_hip.h): the mean map and its Jacobian, the state noise, the linear decoder
        eta = C x + b and y ~ Poisson(exp(eta)) -- no recognition network, and no clamp on eta.  Per row the posterior is the Laplace
        approximation at the mode, found by `n_iter` Newton steps with a per-trial step control, and loglik is the Laplace evidence
        of the row; rows that were not observed are stepped over.  `ekf` is the same for a Gaussian model.
        :param y: (T, B, ydim) of counts (y >= 0; integers are not required); (T, ydim) is one trial
        :param u: (T, B, udim): u[t] drives the transition INTO row t, as in `filter`; row 0 is predicted from the prior with u[0]
        :param x0: the prior of the row before row 0: None (the model's `prior`) or a Gaussian of (B, xdim)
        :param before: (mean (B, xdim), cov (B, xdim, xdim)) in x0's place, such as a previous result's `head`: rows [0, k) first and
            rows [k, T) with before = that head second give the bits of one call.  Giving both x0 and before is a ValueError
        :param state_var: the scalar state-noise variance, default exp(transition.logvar).  Reading the default copies one scalar to
            the host, which synchronises the stream; pass a float to stay asynchronous
        :param observed: (T, B) of booleans or 0 / 1, None: every row.  A row that is not observed is predicted only (its loglik and
            grad_norm are 0) and its y is never used: it may hold NaN
        :param n_iter: Newton steps per row, 1 .. 64; `grad_norm` of the result tells whether they were enough
        :param return_cov: also return the full covariances of every row
        :return: LaplaceFilterResult(mean, var (T, B, xdim), cov (T, B, xdim, xdim) or None, loglik, grad_norm (T, B),
            head = (mean[-1], cov of the last row)); `.gaussian()` is the diagonal posterior `smooth` takes, `.log_likelihood()` the
            evidence per trial.  A trial with a non-finite or negative observed y, a non-finite u or prior at some row, a prior
            covariance that is not positive definite or rates that overflow at the prediction has NaN from that row on.
        Every xdim <= 16 with n_rbf <= 256 and udim <= 8 is accepted whatever ydim is; xdim <= 24 is accepted where the shape fits
        one workgroup's LDS, and xdim > 24 never.  What does not fit raises NotImplementedError naming the limit before anything is
        launched.  Under the Gaussian likelihood this raises NotImplementedError: `ekf` is that model's filter.
        Reads the model's state and writes none; no scratch."""
        if not isinstance(self.likelihood, PoissonLikelihood):
            raise NotImplementedError("laplace_filter needs the Poisson likelihood: ekf is the filter of a Gaussian model")
        if x0 is not None and before is not None:
            raise ValueError("give x0 (a diagonal Gaussian) or before (mean, cov), not both")
        y = dev32(y, ndim2=False)
        B = 1 if y.ndim == 2 else y.shape[1]
        p_mean = p_lv = p_cov = None
        if before is not None:
            p_mean, p_cov = before
        elif x0 is not None:
            p_mean, p_lv = x0.mean, x0.logvar
        else:
            one = torch.ones(B, self.xdim, device=self._blob.device)
            p_mean, p_lv = one * torch.atleast_2d(self.mean), one * torch.atleast_2d(self.logvar)
        state_var = float(self.transition.logvar.exp()) if state_var is None else float(state_var)
        return self.transition._laplace_filter(self.decoder, y, u, p_mean, p_lv, p_cov, state_var, observed, n_iter, return_cov)

    def sample_posterior(self, q: Union[Gaussian, Tuple[Tensor, Tensor]], u: Tensor = None, n_sample: int = 16, *,
                         state_var: float = None, noise: Tensor = None, after: Tensor = None) -> PosteriorSamples:
        """`n_sample` joint draws per trial from the smoothed posterior of a filtered sequence -- whole trajectories, each row
        conditioned on the draw behind it -- in one native call (RBFDS.sample_posterior has the arguments); `model.decoder(res.x)`
        gives draws of the observations' means."""
        return self.transition.sample_posterior(q, u, n_sample, state_var=state_var, noise=noise, after=after)

    def score_forecast(self, q: Union[Gaussian, Tuple[Tensor, Tensor], Tensor], y: Tensor = None, u: Tensor = None, n_step: int = 8, *,
                       return_pred: bool = False) -> ForecastScore:
        """How good the learned dynamics are: the k-step-ahead prediction error over a filtered record -- what `filter_sequence` /
        `fit` returned -- in one native call (RBFDS.score_forecast has the arguments and the contract).
        :param q: the filtered posterior: a Gaussian, a (mu, logvar) pair of tensors (tuple or list) or the means themselves, (T, B, xdim);
            (T, xdim) is one trial
        :param y: (T, B, ydim), the observations: the predictions are also decoded on chip and scored against them, by squared error
            under the Gaussian likelihood and by the Poisson negative log-likelihood (without log y!) under the Poisson one
        :return: ForecastScore; `.r2_x()`, `.r2_y()`, `.skill_x()`, `.skill_y()`, `.mse_x()`, `.mse_y()` reduce it per horizon."""
        mu = q.mean if isinstance(q, Gaussian) else (q[0] if isinstance(q, (tuple, list)) and len(q) == 2 and isinstance(q[0], Tensor) else q)
        kind = "poisson" if isinstance(self.likelihood, PoissonLikelihood) else "gaussian"
        return self.transition._score_forecast(self.decoder, kind, mu, y, u, n_step, return_pred)
