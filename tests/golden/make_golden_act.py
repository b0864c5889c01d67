#!/usr/bin/env python3
"""Golden vectors of the recognition network with other activations than Tanh, from the imported reference (catniplab/vjf).

Run ONLY where the reference exists (as make_golden.py; VJF_REFERENCE names its checkout), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_act.py

The reference builds `Recognition(..., activation=X)` and calls X() once per layer (vjf/recognition.py:17-24); make_model takes no
activation, so the models are built here from their parts.  Files are named g9_act_* (never g5_*: tests/goldenio.traj_names globs
g5_*.npz and runs those as Tanh models).  Each file records the activation (`act`: its torch class name, `act_params`: its two
parameters in the order of the C ABI's vjf_activation p0, p1).  Only numpy arrays are written.
"""
import functools
import os
import sys

import numpy as np
import torch
from torch import nn

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, EpsFeeder, export_state, npy   # noqa: E402  (puts the reference on sys.path)

import vjf.model as ref_model            # noqa: E402
from vjf.distribution import Gaussian    # noqa: E402
from vjf.likelihood import GaussianLikelihood, PoissonLikelihood   # noqa: E402
from vjf.model import RBFDS, VJF         # noqa: E402
from vjf.recognition import Recognition  # noqa: E402

# tag -> (class name, p0, p1, the `activation` argument given to the reference)
ACTS = {
    "relu": ("ReLU", 0.0, 0.0, nn.ReLU),
    "leaky0.2": ("LeakyReLU", 0.2, 0.0, functools.partial(nn.LeakyReLU, 0.2)),
    "elu0.5": ("ELU", 0.5, 0.0, functools.partial(nn.ELU, 0.5)),
    "softplus2": ("Softplus", 2.0, 20.0, functools.partial(nn.Softplus, beta=2)),
    "sigmoid": ("Sigmoid", 0.0, 0.0, nn.Sigmoid),
    "hardtanh": ("Hardtanh", -2.0, 0.5, functools.partial(nn.Hardtanh, -2.0, 0.5)),
    "relu6": ("ReLU6", 0.0, 6.0, nn.ReLU6),
}


def act_record(tag):
    name, p0, p1, _ = ACTS[tag]
    return {"act": np.asarray(name), "act_params": np.asarray([p0, p1], np.float64)}


def traj_act(name, tag, *, dtype, lik, B, dz, dy, du, n, hidden, T, warm_up, lr, seed=0, y_scale=1.0):
    """One trajectory of VJF.filter (sgd, update, warm_up as given): the layout of make_golden.traj plus the activation."""
    torch.set_default_dtype(dtype)
    torch.manual_seed(seed)
    likelihood = PoissonLikelihood() if lik == "poisson" else GaussianLikelihood()   # (make_model's order of construction)
    m = VJF(dy, dz, likelihood, RBFDS(n, dz, du), Recognition(dy, dz, du, hidden, activation=ACTS[tag][3]), lr=lr)
    g = torch.Generator().manual_seed(1000 + seed)
    if lik == "poisson":
        y = torch.poisson(torch.exp(0.5 * torch.randn(T, B, dy, generator=g) - 0.5), generator=g)
    else:
        y = torch.randn(T, B, dy, generator=g) * y_scale
    u = torch.randn(T, B, du, generator=g) if du > 0 else None
    eps = torch.randn(T, 2, B, dz, generator=g)
    rec = {"y": npy(y), "eps": npy(eps)}
    if u is not None:
        rec["u"] = npy(u)
    rec["meta"] = np.asarray([B, dz, dy, du, n, T, int(warm_up)] + list(hidden))
    rec["lik"] = np.asarray(lik)
    rec.update(act_record(tag))
    rec.update(export_state(m, "s0"))
    feeder = EpsFeeder([eps[t, k] for t in range(T) for k in range(2)])
    orig = ref_model.reparametrize
    ref_model.reparametrize = feeder
    try:
        q = None
        per = {k: [] for k in ("mu", "lv", "loss", "rho", "sigma")}
        for t in range(T):
            ut = None if u is None else u[t]
            q, loss, *el = m.filter(y[t], ut, q, sgd=True, update=True, verbose=True, warm_up=warm_up)
            per["mu"].append(npy(q.mean))
            per["lv"].append(npy(q.logvar))
            per["loss"].append([float(loss)] + [float(e) for e in el])
            per["rho"].append(float(m.likelihood.logvar) if hasattr(m.likelihood, "logvar") else 0.0)
            per["sigma"].append(float(m.transition.logvar))
    finally:
        ref_model.reparametrize = orig
    for k, v in per.items():
        rec[f"out.{k}"] = np.asarray(v)
    rec.update(export_state(m, "sT"))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
    print(name, "loss", per["loss"][0][0], "->", per["loss"][-1][0])


def recognition_act():
    """Recognition.forward once per activation (fp64): weights, inputs and outputs."""
    torch.set_default_dtype(torch.float64)
    rec = {}
    tags = list(ACTS)
    for i, tag in enumerate(tags):
        dy, dz, du, hid, B = (10, 3, 2, [16, 8], 16)
        torch.manual_seed(60 + i)
        r = Recognition(dy, dz, du, hid, activation=ACTS[tag][3])
        g = torch.Generator().manual_seed(70 + i)
        y = torch.randn(B, dy, generator=g) * 2
        u = torch.randn(B, du, generator=g)
        mu, lv = torch.randn(B, dz, generator=g), torch.randn(B, dz, generator=g)
        out = r(y, Gaussian(mu, lv), u)
        lins = [l for l in r.mlp if isinstance(l, torch.nn.Linear)]
        rec[f"{i}.meta"] = np.asarray([dy, dz, du, B] + hid)
        for k, v in act_record(tag).items():
            rec[f"{i}.{k}"] = v
        for k, l in enumerate(lins):
            rec[f"{i}.rec_W{k}"], rec[f"{i}.rec_b{k}"] = npy(l.weight), npy(l.bias)
        rec[f"{i}.mean_W"], rec[f"{i}.lv_W"], rec[f"{i}.lv_b"] = npy(r.mean.weight), npy(r.logvar.weight), npy(r.logvar.bias)
        rec[f"{i}.y"], rec[f"{i}.u"], rec[f"{i}.mu"], rec[f"{i}.lv"] = npy(y), npy(u), npy(mu), npy(lv)
        rec[f"{i}.out_mu"], rec[f"{i}.out_lv"] = npy(out.mean), npy(out.logvar)
    rec["count"] = np.asarray(len(tags))
    np.savez_compressed(os.path.join(OUT, "g9_act_recognition.npz"), **rec)


def main():
    recognition_act()
    small = dict(B=16, dz=3, dy=10, n=16, T=8)
    for dt, dtag in ((torch.float64, "f64"), (torch.float32, "f32")):
        for tag in ACTS:
            # SGD visibly moves the recognition weights through the derivative: two hidden layers, lr 1e-2
            traj_act(f"g9_act_{tag}_gaussian_{dtag}", tag, dtype=dt, lik="gaussian", du=0, hidden=[8, 8], warm_up=False, lr=1e-2, **small)
            if tag != "relu6":
                traj_act(f"g9_act_{tag}_poisson_du2_wu1_{dtag}", tag, dtype=dt, lik="poisson", du=2, hidden=[8], warm_up=True, lr=1e-3,
                         **small)
    torch.set_default_dtype(torch.float32)
    files = [f for f in os.listdir(OUT) if f.startswith("g9_act_")]
    print("g9 files:", len(files), "bytes:", sum(os.path.getsize(os.path.join(OUT, f)) for f in files),
          "largest:", max(os.path.getsize(os.path.join(OUT, f)) for f in files))


if __name__ == "__main__":
    main()
