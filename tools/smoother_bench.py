"""`smooth` (one native call: vjf_smooth) against the loop a user writes without it: backwards over the rows, per row one
`model.jacobian` call, the mean step in torch on the GPU, `torch.linalg.cholesky` / `cholesky_solve` for the gain and the two products
of the textbook covariance update.

    python tools/smoother_bench.py [--reps 5] [--region 0.3] [--loop-rows 1000] [--out profiles/smoother_bench.json]

Shapes: one Lorenz-sized trial (configs[0]'s dimensions: d_z = 3, RBF(100)) over 10 000 rows, and 4096 trials of configs[1]'s dimensions
(d_z = 10, RBF(200)) over 200 rows; the filtered means are the model's own trajectory plus 0.05 N(0, 1), the log-variances
U(log 1e-3, log 1e-1), the state-noise variance 0.01.  The baseline is the torch loop, never the code under test; where the record is
longer than --loop-rows the loop is timed over its last --loop-rows rows only and `loop_rows` says so (its cost per row does not depend
on the row).  The variants alternate in one process, each timed over a region of whole calls that lasts at least --region seconds
(sized in the warm-up) and ends in a device synchronise.  Per shape one JSON line: the median and the spread (min .. max) of --reps
regions per variant in microseconds per row, the ratios of the medians, whether every native region is shorter than every region of the
loop, and the largest difference between the two results relative to scale.  What the ratio measures is the loop's launch count (a
dozen small kernels per row) against one launch; it says nothing about how close the kernel is to the hardware's limits.  No ratio is
promised: the exit code is 0 whatever the outcome, the `faster_beyond_spread` field says it.
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

RUNS = [dict(shape="configs[0]", B=1, T=10000, dz=3, dy=10, n=100, hidden=[20]),
        dict(shape="configs[1]", B=4096, T=200, dz=10, dy=50, n=200, hidden=[128])]
Q = 0.01


def features(vel, x):
    c = vel.feature.centroid
    return torch.exp(-.5 * ((x[:, None, :] - c[None]) ** 2).sum(-1) * torch.exp(-2. * vel.feature.logwidth))


def model(cfg):
    import vjf_amd
    torch.manual_seed(0)
    m = vjf_amd.VJF.make_model(cfg["dy"], cfg["dz"], 0, cfg["n"], cfg["hidden"], likelihood="gaussian", noise="device")
    g = torch.Generator().manual_seed(1)
    m.transition.velocity.w_mean.copy_(0.1 * torch.randn(cfg["n"], cfg["dz"], generator=g))
    return m


def sequence(mdl, cfg):
    """(mu, lv) (T, B, d_z): the mean map's own trajectory plus 0.05 N(0, 1); lv ~ U(log 1e-3, log 1e-1)."""
    g = torch.Generator().manual_seed(2)
    T, B, d = cfg["T"], cfg["B"], cfg["dz"]
    x = mdl.transition.forecast_sequence(torch.randn(B, d, generator=g).cuda(), None, T - 1)
    mu = x + 0.05 * torch.randn(T, B, d, generator=g).cuda()
    lv = math.log(1e-3) + (math.log(1e-1) - math.log(1e-3)) * torch.rand(T, B, d, generator=g).cuda()
    return mu.contiguous(), lv.contiguous()


def torch_loop(mdl, mu, lv, with_cov):
    """The loop a user writes today, textbook form.  -> (mean, var, cov or None) of the rows given."""
    vel = mdl.transition.velocity
    T, B, d = mu.shape
    eye = torch.eye(d, device=mu.device)
    mean, var = torch.empty_like(mu), torch.empty_like(mu)
    cov = torch.empty(T, B, d, d, device=mu.device) if with_cov else None
    ms, Ps = mu[-1], torch.diag_embed(lv[-1].exp())
    mean[-1], var[-1] = ms, lv[-1].exp()
    if with_cov:
        cov[-1] = Ps
    for t in range(T - 2, -1, -1):
        J = mdl.jacobian(mu[t])
        mp = mu[t] + features(vel, mu[t]) @ vel.w_mean
        D = lv[t].exp()
        JD = J * D[:, None, :]
        Pp = JD @ J.transpose(1, 2) + Q * eye
        G = torch.cholesky_solve(JD, torch.linalg.cholesky(Pp)).transpose(1, 2)
        ms = mu[t] + (G @ (ms - mp)[:, :, None])[:, :, 0]
        Ps = torch.diag_embed(D) + G @ (Ps - Pp) @ G.transpose(1, 2)
        mean[t], var[t] = ms, torch.diagonal(Ps, dim1=1, dim2=2)
        if with_cov:
            cov[t] = Ps
    return mean, var, cov


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
    ap.add_argument("--loop-rows", type=int, default=1000, help="rows the torch loop is timed over at most")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "smoother_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "smoother_bench needs a GPU"
    lines = []
    with torch.no_grad():
        for cfg in RUNS:
            mdl = model(cfg)
            mu, lv = sequence(mdl, cfg)
            T = cfg["T"]
            lr = min(T, a.loop_rows)
            rows = {"torch_loop": lr, "torch_loop_cov": lr, "native": T, "native_cov": T}
            variants = {"torch_loop": lambda: torch_loop(mdl, mu[T - lr:], lv[T - lr:], False),
                        "torch_loop_cov": lambda: torch_loop(mdl, mu[T - lr:], lv[T - lr:], True),
                        "native": lambda: mdl.smooth((mu, lv), state_var=Q),
                        "native_cov": lambda: mdl.smooth((mu, lv), state_var=Q, return_cov=True)}
            ref, got = variants["torch_loop_cov"](), variants["native_cov"]()
            diff = {"mean": float((got.mean[T - lr:] - ref[0]).abs().max() / ref[0].abs().max().clamp(min=1.)),
                    "cov": float((got.cov[T - lr:] - ref[2]).abs().max() / ref[2].abs().max())}
            calls = {}
            for k, fn in variants.items():                               # warm-up, and the size of a region
                fn()
                calls[k] = max(1, math.ceil(1.3 * a.region / max(region(fn, 1), 1e-6)))
            times = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():                           # alternating
                    times[k].append(region(fn, calls[k]) / calls[k] / rows[k] * 1e6)
            med = {k: statistics.median(v) for k, v in times.items()}
            line = {"bench": "smooth", "shape": cfg["shape"], "trials": cfg["B"], "rows": T, "loop_rows": lr, "d_z": cfg["dz"], "n_rbf": cfg["n"],
                    "state_var": Q, "unit": "us per row", "reps": a.reps,
                    **{k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3), "calls_per_region": calls[k],
                           "region_s": round(med[k] * calls[k] * rows[k] * 1e-6, 3)} for k, v in times.items()},
                    "speedup": round(med["torch_loop"] / med["native"], 2), "speedup_cov": round(med["torch_loop_cov"] / med["native_cov"], 2),
                    "faster_beyond_spread": max(times["native"]) < min(times["torch_loop"]) and max(times["native_cov"]) < min(times["torch_loop_cov"]),
                    "largest_difference_over_scale": {k: float(f"{v:.3g}") for k, v in diff.items()}}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
