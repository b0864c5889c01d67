#!/usr/bin/env python3
"""Golden gradients of VJF.filter from the imported reference (catniplab/vjf): every parameter's `.grad` BEFORE the clip.

Run ONLY where the reference exists (as make_golden.py; VJF_REFERENCE names its checkout), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grads.py

The reference's step calls `nn.utils.clip_grad_value_(self.parameters(), 1.)` between `loss.backward()` and `optimizer.step()`
(vjf/model.py:209-211).  Here that function is wrapped for the length of a trajectory: the wrapper copies every parameter's `.grad`,
then calls the original; nothing else of the reference changes.  For the Poisson case whose eta straddles the clamp at 10
(vjf/likelihood.py:60) `VJF.make_model` is wrapped as well, to scale the freshly drawn decoder before the first step.

One file, tests/golden/g11_grads.npz, holds several numbered cases in fp64 -- `count`, then per case i: `i.meta`
[B, dz, dy, du, n, warm_up, hidden...], `i.lik`, `i.<state tensor>` (what the forward pass reads: no w_precision / w_pchol), `i.y`,
`i.u`, `i.eps` (2, B, dz), `i.mu_s` / `i.lv_s` where the step starts from a posterior, and `i.grad.<tensor>` named as
tests/helpers.model_arrays names the tensors.  Only numpy arrays are written.
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, npy, traj        # noqa: E402  (puts the reference on sys.path)

from vjf.model import VJF                     # noqa: E402

TMP = "_g11_tmp"
FORWARD_STATE = ("prior_mean", "prior_logvar", "lik_logvar", "tr_logvar", "centroid", "logwidth", "w_mean", "w_chol",
                 "mean_W", "lv_W", "lv_b", "dec_W", "dec_b")


def fixture_name(param_name):
    """reference parameter name -> fixture key (tests/golden/make_golden.export_state)"""
    p = param_name.split(".")
    if param_name == "likelihood.logvar":
        return "lik_logvar"
    if p[:2] == ["recognition", "mlp"]:
        return ("rec_W" if p[3] == "weight" else "rec_b") + str(int(p[2]) // 2)
    return {"recognition.mean.weight": "mean_W", "recognition.logvar.weight": "lv_W", "recognition.logvar.bias": "lv_b",
            "decoder.decode.weight": "dec_W", "decoder.decode.bias": "dec_b"}.get(param_name)


class recording_grads:
    """Within the block every call of nn.utils.clip_grad_value_ first appends [grad or None per parameter] to `self.steps`."""
    def __enter__(self):
        self.steps = []
        self.orig = orig = torch.nn.utils.clip_grad_value_
        steps = self.steps

        def clip_grad_value_(parameters, clip_value, *a, **k):
            parameters = list(parameters)
            steps.append([None if p.grad is None else npy(p.grad) for p in parameters])
            return orig(parameters, clip_value, *a, **k)
        torch.nn.utils.clip_grad_value_ = clip_grad_value_
        return self

    def __exit__(self, *exc):
        torch.nn.utils.clip_grad_value_ = self.orig


class scaled_decoder:
    """Within the block VJF.make_model returns a model whose decoder is  W <- scale W,  b <- b + shift."""
    def __init__(self, scale, shift):
        self.scale, self.shift = scale, shift

    def __enter__(self):
        self.orig = orig = VJF.__dict__["make_model"]
        scale, shift = self.scale, self.shift

        def make_model(cls, *a, **k):
            m = orig.__func__(cls, *a, **k)
            with torch.no_grad():
                m.decoder.decode.weight.mul_(scale)
                m.decoder.decode.bias.add_(shift)
            return m
        VJF.make_model = classmethod(make_model)

    def __exit__(self, *exc):
        VJF.make_model = self.orig


def run(*, lik, B, dz, dy, du, n, hidden, T, warm_up, seed):
    """[case dict per step] of a T-step fp64 trajectory of make_golden.traj."""
    torch.set_default_dtype(torch.float64)
    names = [k for k, _ in VJF.make_model(dy, dz, du, n, hidden, likelihood=lik).named_parameters()]
    with recording_grads() as rec:
        traj(TMP, dtype=torch.float64, lik=lik, B=B, dz=dz, dy=dy, du=du, n=n, hidden=hidden, T=T, warm_up=warm_up, seed=seed,
             keep_states=tuple(range(1, T)))
    path = os.path.join(OUT, TMP + ".npz")
    with np.load(path) as z:
        z = {k: z[k] for k in z.files}
    os.remove(path)
    assert len(rec.steps) == T and all(len(g) == len(names) for g in rec.steps)
    cases = []
    for t in range(T):
        c = {"meta": np.asarray([B, dz, dy, du, n, int(warm_up)] + list(hidden)), "lik": np.asarray(lik),
             "y": z["y"][t], "eps": z["eps"][t]}
        if du:
            c["u"] = z["u"][t]
        if t > 0:
            c["mu_s"], c["lv_s"] = z["out.mu"][t - 1], z["out.lv"][t - 1]
        keys = FORWARD_STATE + tuple(f"rec_{w}{k}" for k in range(len(hidden)) for w in "Wb")
        for k in keys:
            if f"s{t}.{k}" in z:
                c[k] = z[f"s{t}.{k}"]
        for name, g in zip(names, rec.steps[t]):
            key = fixture_name(name)
            if key is not None:
                assert g is not None, name
                c["grad." + key] = g
        cases.append(c)
    return cases


def main():
    mega = dict(lik="gaussian", dy=10, dz=3, du=2, n=40, hidden=[8])            # tests/lifetime.FAMILIES["mega"]
    mega_p = dict(lik="poisson", dy=12, dz=5, du=0, n=100, hidden=[20, 12])     # ... ["mega_p"]
    cases = run(B=37, T=2, warm_up=False, seed=3, **mega)                       # 0: from the prior; 1: from the posterior, after an RLS update
    cases += run(B=33, T=1, warm_up=True, seed=4, **mega)                       # 2: warm_up
    with scaled_decoder(8.0, 6.0):
        cases += run(B=40, T=1, warm_up=False, seed=5, **mega_p)                # 3: Poisson, eta on both sides of 10
    rec = {"count": np.asarray(len(cases))}
    for i, c in enumerate(cases):
        rec.update({f"{i}.{k}": np.asarray(v) for k, v in c.items()})
    assert all(v.dtype.kind in "fiU" for v in rec.values())
    path = os.path.join(OUT, "g11_grads.npz")
    np.savez_compressed(path, **rec)
    torch.set_default_dtype(torch.float32)
    print("g11_grads.npz:", len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
