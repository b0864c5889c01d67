"""Cost of the recognition layers' activation on the one-launch route (vjf_mega_act_kernel against vjf_mega_kernel).

    python tools/act_bench.py [--steps 200] [--reps 5]

At configs[1] (B = 4096 trials, d_z = 10, d_y = 50, RBF(200), hidden [128], Gaussian) it times `filter_sequence` over --steps steps,
warmed up, alternating a Tanh model and a model with the activation in the same process (the median of --reps pairs), and prints
one JSON line per activation: us/step, M trial-timesteps/s and the ratio to Tanh.
"""
import argparse
import functools
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACTS = {
    "ReLU": nn.ReLU,
    "LeakyReLU(0.2)": functools.partial(nn.LeakyReLU, 0.2),
    "ELU": nn.ELU,
    "Softplus": nn.Softplus,
    "Sigmoid": nn.Sigmoid,
    "Hardtanh": nn.Hardtanh,
}


def model(act, cfg):
    import vjf_amd
    from vjf_amd.likelihood import GaussianLikelihood
    from vjf_amd.model import RBFDS
    from vjf_amd.recognition import Recognition
    torch.manual_seed(0)
    return vjf_amd.VJF(cfg["dy"], cfg["dz"], GaussianLikelihood(), RBFDS(cfg["n"], cfg["dz"], 0),
                       Recognition(cfg["dy"], cfg["dz"], 0, cfg["hidden"], activation=act), lr=1e-3)


def time_seq(m, y, eps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    m.filter_sequence(y, eps=eps)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / y.shape[0]          # us per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    cfg = dict(B=4096, dz=10, dy=50, n=200, hidden=[128])
    g = torch.Generator().manual_seed(1)
    y = torch.randn(args.steps, cfg["B"], cfg["dy"], generator=g).cuda()
    eps = torch.randn(args.steps, 2, cfg["B"], cfg["dz"], generator=g).cuda()
    for name, act in ACTS.items():
        mt, ma = model(nn.Tanh, cfg), model(act, cfg)
        for m in (mt, ma):                                   # warm-up: contexts, first launches
            m.filter_sequence(y[:8], eps=eps[:8])
            m.filter_sequence(y, eps=eps)
        assert mt.route() == "one-launch" and ma.route() == "one-launch", (mt.route(), ma.route())
        tt, ta = [], []
        for _ in range(args.reps):
            tt.append(time_seq(mt, y, eps))
            ta.append(time_seq(ma, y, eps))
        assert mt.status() == 0 and ma.status() == 0
        t_tanh, t_act = statistics.median(tt), statistics.median(ta)
        print(json.dumps({"activation": name, "config": "configs[1]", "steps": args.steps, "us_per_step": round(t_act, 2),
                          "M_trial_timesteps_per_s": round(cfg["B"] / t_act, 1), "tanh_us_per_step": round(t_tanh, 2),
                          "ratio_to_tanh": round(t_act / t_tanh, 4)}), flush=True)
        del mt, ma


if __name__ == "__main__":
    main()
