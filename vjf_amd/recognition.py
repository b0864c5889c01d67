"""vjf.recognition on the GPU   (mirror of vjf/recognition.py)."""
import ctypes
from typing import Sequence, Union

import torch
from torch import Tensor
from torch import nn
from torch.nn import Linear, Module, Sequential, Tanh

from . import _native as N
from .distribution import Gaussian
from .util import dev32, stream_ptr

__all__ = ['Recognition', 'activation_code', 'SUPPORTED_ACTIVATIONS']

SUPPORTED_ACTIVATIONS = ("Tanh, ReLU, LeakyReLU(negative_slope >= 0), ELU(alpha > 0), Softplus(beta > 0, threshold >= 20), Sigmoid, "
                         "Hardtanh(min_val < max_val), ReLU6")


def activation_code(module: Module):
    """(kind, p0, p1) of the C ABI's vjf_activation for an activation module, matched by its exact type.  The supported set is the
    activations whose derivative follows from the layer's output (the HIP routes keep no pre-activation); anything else raises
    NotImplementedError naming that set."""
    t = type(module)
    if t is nn.Tanh:
        return N.ACT_TANH, 0.0, 0.0
    if t is nn.ReLU:
        return N.ACT_RELU, 0.0, 0.0
    if t is nn.Sigmoid:
        return N.ACT_SIGMOID, 0.0, 0.0
    if t is nn.ReLU6:
        return N.ACT_HARDTANH, 0.0, 6.0
    if t is nn.LeakyReLU and float(module.negative_slope) >= 0.0:
        return N.ACT_LEAKY_RELU, float(module.negative_slope), 0.0
    if t is nn.ELU and float(module.alpha) > 0.0:
        return N.ACT_ELU, float(module.alpha), 0.0
    if t is nn.Softplus and float(module.beta) > 0.0 and float(module.threshold) >= 20.0:
        return N.ACT_SOFTPLUS, float(module.beta), float(module.threshold)
    if t is nn.Hardtanh and float(module.min_val) < float(module.max_val):
        return N.ACT_HARDTANH, float(module.min_val), float(module.max_val)
    raise NotImplementedError(f"activation {module!r} is not supported by the HIP recognition kernels; supported: {SUPPORTED_ACTIVATIONS}")


class Recognition(Module):
    """MLP on [y, u, mean, logvar] -> Gaussian(mean head without bias, logvar head with bias)
    (vjf/recognition.py:16-42).  Layers are torch Linear modules so that a seed gives the
    reference's initial weights and state_dict keys; their forward is never used -- the forward
    pass is the HIP operator.  `activation` is called once per layer, as the reference does (a class, a
    functools.partial or a lambda); every layer must get the same supported activation (activation_code)."""
    def __init__(self, ydim: int, xdim: int, udim: int, hidden_sizes: Sequence[int], activation=Tanh):
        super().__init__()
        self.ydim, self.xdim, self.udim = ydim, xdim, udim
        self.hidden_sizes = [int(h) for h in hidden_sizes]
        layers = [Linear(ydim + udim + 2 * xdim, hidden_sizes[0]), activation()]
        for k in range(len(hidden_sizes) - 1):
            layers.append(Linear(hidden_sizes[k], hidden_sizes[k + 1]))
            layers.append(activation())
        codes = {activation_code(m) for m in layers[1::2]}
        if len(codes) != 1:
            raise NotImplementedError("the HIP recognition kernels apply one activation to every layer")
        self.act_code = codes.pop()                        # (kind, p0, p1): model structure, like hidden_sizes (not in the state)
        self.add_module('mlp', Sequential(*layers))
        self.add_module('mean', Linear(hidden_sizes[-1], xdim, bias=False))
        self.add_module('logvar', Linear(hidden_sizes[-1], xdim, bias=True))
        for p in self.parameters():
            p.requires_grad_(False)
            p.data = dev32(p.data, ndim2=False)

    def activation(self) -> "N.VjfActivation":
        """The layers' activation as the C ABI's vjf_activation."""
        kind, p0, p1 = self.act_code
        return N.VjfActivation(kind, p0, p1)

    def linears(self):
        return [m for m in self.mlp if isinstance(m, Linear)]

    def forward(self, y: Tensor, xs: Union[Tensor, Gaussian], u: Tensor = None) -> Gaussian:
        if isinstance(xs, Tensor):
            raise NotImplementedError("Recognition on a point state is not used by VJF (model.py:116 passes a Gaussian)")
        elif not isinstance(xs, Gaussian):
            raise TypeError
        y = dev32(y)
        mu_s, lv_s = dev32(xs.mean), dev32(xs.logvar)
        u = None if (u is None or self.udim == 0) else dev32(u)
        B = y.shape[0]
        lins = self.linears()
        L = len(lins)
        Wp = (ctypes.c_void_p * L)(*[l.weight.data_ptr() for l in lins])
        bp = (ctypes.c_void_p * L)(*[l.bias.data_ptr() for l in lins])
        hid = (ctypes.c_int32 * L)(*self.hidden_sizes)
        mu_t = torch.empty(B, self.xdim, device=y.device, dtype=torch.float32)
        lv_t = torch.empty(B, self.xdim, device=y.device, dtype=torch.float32)
        args = (N.ptr(y), N.ptr(u), N.ptr(mu_s), N.ptr(lv_s), Wp, bp, N.ptr(self.mean.weight), N.ptr(self.logvar.weight),
                N.ptr(self.logvar.bias), N.ptr(mu_t), N.ptr(lv_t), B, self.ydim, self.udim, self.xdim, L, hid)
        if self.act_code[0] == N.ACT_TANH:
            N.check(N.lib().vjf_recognition_forward(*args, stream_ptr()), "vjf_recognition_forward")
        else:
            N.check(N.lib().vjf_recognition_forward_act(*args, ctypes.byref(self.activation()), stream_ptr()),
                    "vjf_recognition_forward_act")
        return Gaussian(mu_t, lv_t)
