"""`lyapunov` (one native call per horizon: vjf_tangent_rollout) against the loop a user writes without it: per step, torch on the GPU
for the features and the mean step, the analytic J Q as einsums over the shared matrices, and a batched `torch.linalg.qr` with the
signs fixed every `qr_every` steps.

    python tools/tangent_bench.py [--reps 5] [--region 0.3] [--loop-budget 5] [--out profiles/tangent_bench.json]

Shapes: one Lorenz trial (configs[0]'s dimensions: B = 1, d_z = 3, RBF(100)), m = 3, 10 000 steps, qr_every 1 and 8; configs[1]'s
dimensions (B = 4096, d_z = 10, RBF(200)), m = 10 and m = 2, 200 steps, qr_every 1 and 8.  The baseline is the torch loop, never the
code under test.  The two variants alternate in one process, each timed over a region of whole calls that lasts at least --region
seconds (sized in the warm-up) and ends in a device synchronise.  Per shape one JSON line: the median and the spread (min .. max) of
--reps regions per variant in us per step, the ratio of the medians, whether every native region is shorter than every region of the
loop, and the largest difference of the exponents.  For the split of the native step, each line also has the native call with one
interval for the whole horizon (`native_one_interval`: the Gram-Schmidt passes but one taken out) and `forecast_sequence` of the same
horizon without noise (`rollout_only`: the features and the x step with a weights kernel in front, no tangent products).
The loop does the same work at every step (a QR every `qr_every` steps), and at 4096 trials a call of it over 200 steps takes over a minute
(the batched `torch.linalg.qr` is what takes them): where one call of the loop over the whole horizon would take more than --loop-budget seconds (estimated from a probe of a few intervals), the loop is timed over a shorter horizon, a
multiple of `qr_every` -- `torch_loop_steps` in the line -- and reported per step like the rest; the native calls always run the whole
horizon.  No ratio is promised: the exit code is 0 whatever the outcome, the `faster_beyond_spread` field says it.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RUNS = [dict(shape="configs[0]", B=1, dz=3, dy=10, n=100, hidden=[20], m=3, T=10000),
        dict(shape="configs[1]", B=4096, dz=10, dy=50, n=200, hidden=[128], m=10, T=200),
        dict(shape="configs[1]", B=4096, dz=10, dy=50, n=200, hidden=[128], m=2, T=200)]


def model(cfg):
    """A model whose roll-out stays among its centroids and whose map is not the identity: weights of 0.3 N(0, 1)."""
    import vjf_amd
    torch.manual_seed(0)
    m = vjf_amd.VJF.make_model(cfg["dy"], cfg["dz"], 0, cfg["n"], cfg["hidden"], likelihood="gaussian", noise="device")
    m.transition.velocity.w_mean.copy_(0.3 * torch.randn(cfg["n"], cfg["dz"], generator=torch.Generator().manual_seed(1)))
    return m


def torch_loop(vel, x0, m, T, qr):
    """The loop a user writes today: exponents (B, m), x, Q."""
    c, W = vel.feature.centroid, vel.w_mean
    iw2 = torch.exp(-2. * vel.feature.logwidth)
    B, xdim = x0.shape
    cx = c[:, :xdim]
    x, Q = x0, torch.eye(xdim, m, device=x0.device).expand(B, xdim, m).contiguous()
    lsum = torch.zeros(B, m, device=x0.device)
    for t in range(T):
        phi = torch.exp(-.5 * ((x[:, None, :] - c[None]) ** 2).sum(-1) * iw2)
        s = (phi * iw2)[:, :, None] * (torch.einsum("bj,bjv->bv", x, Q)[:, None, :] - torch.einsum("kj,bjv->bkv", cx, Q))
        Q = Q - torch.einsum("ki,bkv->biv", W, s)
        x = x + phi @ W
        if (t + 1) % qr == 0 or t + 1 == T:
            Q, R = torch.linalg.qr(Q)
            d = torch.diagonal(R, dim1=-2, dim2=-1)
            Q = Q * torch.sign(d)[:, None, :]
            lsum = lsum + torch.log(d.abs())
    return lsum / T, x, Q


def region(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--region", type=float, default=0.3, help="least length of a timed region, seconds")
    ap.add_argument("--loop-budget", type=float, default=5., help="most seconds one call of the torch loop may take")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tangent_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tangent_bench needs a GPU"
    lines = []
    with torch.no_grad():
        for cfg in RUNS:
            mdl = model(cfg)
            tr, T, m = mdl.transition, cfg["T"], cfg["m"]
            x0 = torch.randn(cfg["B"], cfg["dz"], generator=torch.Generator().manual_seed(2)).cuda()
            zeros = torch.zeros(T, cfg["n"], cfg["dz"], device="cuda")
            for qr in (1, 8):
                # the loop's horizon: the whole one where a call fits the budget (a probe of eight intervals says)
                probe = min(T, 8 * qr)
                torch_loop(tr.velocity, x0, m, probe, qr)
                per_step = region(lambda: torch_loop(tr.velocity, x0, m, probe, qr), 1) / probe
                Tl = T if per_step * T <= a.loop_budget else max(probe, int(a.loop_budget / per_step) // qr * qr)
                variants = {"torch_loop": lambda: torch_loop(tr.velocity, x0, m, Tl, qr),
                            "native": lambda: tr.lyapunov(x0, None, T, n_exponent=m, qr_every=qr),
                            "native_one_interval": lambda: tr.lyapunov(x0, None, T, n_exponent=m, qr_every=T),
                            "rollout_only": lambda: tr.forecast_sequence(x0, None, T, w_noise=zeros)}
                steps = {k: Tl if k == "torch_loop" else T for k in variants}
                ea, eb = variants["torch_loop"]()[0], tr.lyapunov(x0, None, Tl, n_exponent=m, qr_every=qr).exponents
                diff = float((ea - eb).abs().max())
                assert math.isfinite(diff) and float(eb.abs().max()) < 10
                calls = {}
                for k, fn in variants.items():                               # warm-up, and the size of a region
                    fn()
                    calls[k] = max(1, math.ceil(1.3 * a.region / max(region(fn, 1), 1e-6)))
                times = {k: [] for k in variants}
                for _ in range(a.reps):
                    for k, fn in variants.items():                           # alternating
                        times[k].append(region(fn, calls[k]) / (calls[k] * steps[k]) * 1e6)
                med = {k: statistics.median(v) for k, v in times.items()}
                line = {"bench": "tangent", "shape": cfg["shape"], "B": cfg["B"], "d_z": cfg["dz"], "n_rbf": cfg["n"], "m": m, "n_step": T,
                        "qr_every": qr, "torch_loop_steps": Tl, "unit": "us per step", "reps": a.reps,
                        **{k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3), "calls_per_region": calls[k],
                               "region_s": round(med[k] * calls[k] * steps[k] * 1e-6, 3)} for k, v in times.items()},
                        "speedup": round(med["torch_loop"] / med["native"], 2),
                        "faster_beyond_spread": max(times["native"]) < min(times["torch_loop"]),
                        "exponent_range": [round(float(eb.min()), 5), round(float(eb.max()), 5)],
                        "max_abs_diff_exponents": diff}
                print(json.dumps(line), flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
