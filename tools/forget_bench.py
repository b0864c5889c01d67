"""Cost of the forgetting factor of the RLS update on the one-launch route (`transition.shrink`, VJF_SC_SHRINK).

    python tools/forget_bench.py [--steps 200] [--reps 5] [--out profiles/forget_bench.json]

At configs[1] (B = 4096 trials, d_z = 10, d_y = 50, RBF(200), hidden [128], Gaussian) it times `filter_sequence` over --steps steps,
warmed up, alternating a model with shrink = 1 and one with shrink = 0.98 in the same process (the median of --reps pairs).  The
factor is a launch constant read from the state: both models run the same kernel, so the ratio measures what multiplying by a value
other than 1 changes -- nothing is expected.  One JSON line, printed and written to --out: us/step and M trial-timesteps/s of both
and the ratio.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAM = 0.98


def model(cfg, shrink):
    import vjf_amd
    torch.manual_seed(0)
    return vjf_amd.VJF.make_model(cfg["dy"], cfg["dz"], 0, cfg["n"], cfg["hidden"], likelihood="gaussian", lr=1e-3, shrink=shrink)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forget_bench.json"))
    args = ap.parse_args()
    cfg = dict(B=4096, dz=10, dy=50, n=200, hidden=[128])
    g = torch.Generator().manual_seed(1)
    y = torch.randn(args.steps, cfg["B"], cfg["dy"], generator=g).cuda()
    eps = torch.randn(args.steps, 2, cfg["B"], cfg["dz"], generator=g).cuda()
    m1, mf = model(cfg, 1.0), model(cfg, LAM)
    for m in (m1, mf):                                       # warm-up: contexts, first launches
        m.filter_sequence(y[:8], eps=eps[:8])
        m.filter_sequence(y, eps=eps)
    assert m1.route() == "one-launch" and mf.route() == "one-launch", (m1.route(), mf.route())
    t1, tf = [], []
    for _ in range(args.reps):
        t1.append(time_seq(m1, y, eps))
        tf.append(time_seq(mf, y, eps))
    assert m1.status() == 0 and mf.status() == 0
    a, b = statistics.median(t1), statistics.median(tf)
    # what the factor is for: the size of P (the weight of the past against one new step) stays bounded
    p1 = float(m1.transition.velocity.w_precision.diagonal().max())
    pf = float(mf.transition.velocity.w_precision.diagonal().max())
    line = json.dumps({"config": "configs[1]", "route": "one-launch", "steps": args.steps, "reps": args.reps,
                       "shrink_1": {"us_per_step": round(a, 2), "M_trial_timesteps_per_s": round(cfg["B"] / a, 1), "max_diag_P": p1},
                       f"shrink_{LAM}": {"us_per_step": round(b, 2), "M_trial_timesteps_per_s": round(cfg["B"] / b, 1), "max_diag_P": pf},
                       "ratio": round(b / a, 4)})
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
