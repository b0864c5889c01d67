"""`ekf` (one native call: vjf_ekf) against the loop a user writes without it: forwards over the rows, per row one `model.jacobian`
call, the mean step in torch on the GPU, `torch.linalg.cholesky` / `cholesky_solve` of the innovation covariance for the gain and the
evidence, and the products of the textbook update.

    python tools/ekf_bench.py [--reps 5] [--region 0.3] [--loop-rows 1000] [--out profiles/ekf_bench.json]

Shapes: one Lorenz-sized trial (configs[0]'s dimensions: d_z = 3, RBF(100), d_y = 10) over 10 000 rows, and 4096 trials of configs[1]'s
dimensions (d_z = 10, RBF(200), d_y = 50) over 200 rows; y is decoded from the model's own trajectory plus sqrt(r) N(0, 1), r = 0.1, the
state-noise variance 0.01, the prior N(x0, 0.05 I).  The baseline is the torch loop, never the code under test; where the record is
longer than --loop-rows the loop is timed over its first --loop-rows rows only and `loop_rows` says so (its cost per row does not depend
on the row).  The variants alternate in one process, each timed over a region of whole calls that lasts at least --region seconds
(sized in the warm-up) and ends in a device synchronise.  Per shape one JSON line: the median and the spread (min .. max) of --reps
regions per variant in microseconds per row, the ratios of the medians, whether every native region is shorter than every region of the
loop, and the largest difference between the two results relative to scale.  What the ratio measures is the loop's launch count (some
twenty small kernels per row) against one launch; it says nothing about how close the kernel is to the hardware's limits: no kernel
trace and no LDS-traffic count is taken here, so the kernel's own speed of light is not established.  No ratio is promised: the exit
code is 0 whatever the outcome, the `faster_beyond_spread` field says it.
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
Q, R, P0 = 0.01, 0.1, 0.05


def features(vel, x):
    c = vel.feature.centroid
    return torch.exp(-.5 * ((x[:, None, :] - c[None]) ** 2).sum(-1) * torch.exp(-2. * vel.feature.logwidth))


def model(cfg):
    import vjf_amd
    torch.manual_seed(0)
    m = vjf_amd.VJF.make_model(cfg["dy"], cfg["dz"], 0, cfg["n"], cfg["hidden"], likelihood="gaussian", noise="device")
    g = torch.Generator().manual_seed(1)
    m.transition.velocity.w_mean.copy_(0.1 * torch.randn(cfg["n"], cfg["dz"], generator=g))
    m.decoder.decode.weight.copy_(0.5 * torch.randn(cfg["dy"], cfg["dz"], generator=g))
    m.decoder.decode.bias.copy_(0.1 * torch.randn(cfg["dy"], generator=g))
    return m


def record(mdl, cfg):
    """(y (T, B, d_y), x0 (B, d_z)): the decoder's image of the mean map's own trajectory from x0, plus sqrt(R) N(0, 1)."""
    g = torch.Generator().manual_seed(2)
    T, B, d = cfg["T"], cfg["B"], cfg["dz"]
    x0 = torch.randn(B, d, generator=g).cuda()
    x = mdl.transition.forecast_sequence(x0, None, T)[1:]
    y = mdl.decoder(x) + math.sqrt(R) * torch.randn(T, B, cfg["dy"], generator=g).cuda()
    return y.contiguous(), x0


def torch_loop(mdl, y, x0, with_cov):
    """The loop a user writes today, textbook form.  -> (mean, var, cov or None, loglik) of the rows given."""
    vel = mdl.transition.velocity
    C, b = mdl.decoder.decode.weight, mdl.decoder.decode.bias
    T, B, dy = y.shape
    d = x0.shape[1]
    eye, eyey = torch.eye(d, device=y.device), torch.eye(dy, device=y.device)
    mean, var = torch.empty(T, B, d, device=y.device), torch.empty(T, B, d, device=y.device)
    cov = torch.empty(T, B, d, d, device=y.device) if with_cov else None
    ll = torch.empty(T, B, device=y.device)
    m, P = x0, P0 * eye.expand(B, d, d)
    const = dy * math.log(2 * math.pi)
    for t in range(T):
        J = mdl.jacobian(m)
        m = m + features(vel, m) @ vel.w_mean
        P = J @ P @ J.transpose(1, 2) + Q * eye
        CP = C @ P                                           # (B, dy, d)
        S = CP @ C.T + R * eyey
        Ls = torch.linalg.cholesky(S)
        v = y[t] - b - m @ C.T
        K = torch.cholesky_solve(CP, Ls).transpose(1, 2)     # P C^T S^-1
        w = torch.cholesky_solve(v[:, :, None], Ls)[:, :, 0]
        ll[t] = -0.5 * (const + 2 * torch.diagonal(Ls, dim1=1, dim2=2).log().sum(1) + (v * w).sum(1))
        m = m + (K @ v[:, :, None])[:, :, 0]
        P = P - K @ CP
        mean[t], var[t] = m, torch.diagonal(P, dim1=1, dim2=2)
        if with_cov:
            cov[t] = P
    return mean, var, cov, ll


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ekf_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ekf_bench needs a GPU"
    import vjf_amd
    lines = []
    with torch.no_grad():
        for cfg in RUNS:
            mdl = model(cfg)
            y, x0 = record(mdl, cfg)
            T = cfg["T"]
            lr = min(T, a.loop_rows)
            prior = vjf_amd.Gaussian(x0, torch.full_like(x0, math.log(P0)))
            rows = {"torch_loop": lr, "torch_loop_cov": lr, "native": T, "native_cov": T}
            variants = {"torch_loop": lambda: torch_loop(mdl, y[:lr], x0, False),
                        "torch_loop_cov": lambda: torch_loop(mdl, y[:lr], x0, True),
                        "native": lambda: mdl.ekf(y, x0=prior, state_var=Q, obs_var=R),
                        "native_cov": lambda: mdl.ekf(y, x0=prior, state_var=Q, obs_var=R, return_cov=True)}
            ref, got = variants["torch_loop_cov"](), variants["native_cov"]()
            diff = {"mean": float((got.mean[:lr] - ref[0]).abs().max() / ref[0].abs().max().clamp(min=1.)),
                    "cov": float((got.cov[:lr] - ref[2]).abs().max() / ref[2].abs().max()),
                    "loglik": float((got.loglik[:lr] - ref[3]).abs().max() / ref[3].abs().max())}
            calls = {}
            for k, fn in variants.items():                               # warm-up, and the size of a region
                fn()
                calls[k] = max(1, math.ceil(1.3 * a.region / max(region(fn, 1), 1e-6)))
            times = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():                           # alternating
                    times[k].append(region(fn, calls[k]) / calls[k] / rows[k] * 1e6)
            med = {k: statistics.median(v) for k, v in times.items()}
            line = {"bench": "ekf", "shape": cfg["shape"], "trials": cfg["B"], "rows": T, "loop_rows": lr, "d_z": cfg["dz"], "d_y": cfg["dy"],
                    "n_rbf": cfg["n"], "state_var": Q, "obs_var": R, "unit": "us per row", "reps": a.reps,
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
