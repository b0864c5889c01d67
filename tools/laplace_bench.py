"""`laplace_filter` (one native call: vjf_laplace_filter) against the loop a user writes without it: forwards over the rows, per row one
`model.jacobian` call, the mean step in torch on the GPU, and the same Newton iteration in whitened coordinates (the contract of
include/vjf_hip.h, statement for statement) with `torch.linalg.cholesky` and triangular solves.

    python tools/laplace_bench.py [--reps 5] [--region 0.3] [--loop-rows 200] [--out profiles/laplace_bench.json]

Shapes: one Lorenz-sized trial (configs[0]'s dimensions: d_z = 3, RBF(100), d_y = 10) over 10 000 rows, and 4096 trials of configs[2]'s
dimensions (d_z = 10, RBF(200), d_y = 200) over 200 rows; the counts are drawn Poisson(exp(min(eta, 8))) from the decoder's image of the
mean map's own trajectory, the state-noise variance is 0.01 and the prior N(x0, 0.05 I).  The baseline is the torch loop, never the code
under test; where the record is longer than --loop-rows the loop is timed over its first --loop-rows rows only and `loop_rows` says so
(its cost per row does not depend on the row).  The variants alternate in one process, each timed over a region of whole calls that
lasts at least --region seconds (sized in the warm-up) and ends in a device synchronise.  Per shape one JSON line: the median and the
spread (min .. max) of --reps regions per variant in microseconds per row, and
    speedup            torch loop over native, both at n_iter = 8: what it measures is the loop's launch count (some forty small kernels
                       per Newton iteration) against one launch, not how close the kernel is to the hardware's limits;
    iter8_over_iter1   native at n_iter = 8 over native at n_iter = 1 on the same inputs: nine E / D pairs against two beside the same
                       prediction, so the share of a row's time the iteration takes.
No kernel trace and no counter is taken here: every time is wall-clock around whole calls, so the kernel's own time is not separated
from the launch.  No ratio is promised: the exit code is 0 whatever the outcome, the `faster_beyond_spread` field says it.
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
        dict(shape="configs[2]", B=4096, T=200, dz=10, dy=200, n=200, hidden=[128])]
Q, P0, N_ITER = 0.01, 0.05, 8


def features(vel, x):
    c = vel.feature.centroid
    return torch.exp(-.5 * ((x[:, None, :] - c[None]) ** 2).sum(-1) * torch.exp(-2. * vel.feature.logwidth))


def model(cfg):
    import vjf_amd
    torch.manual_seed(0)
    m = vjf_amd.VJF.make_model(cfg["dy"], cfg["dz"], 0, cfg["n"], cfg["hidden"], likelihood="poisson", noise="device")
    g = torch.Generator().manual_seed(1)
    m.transition.velocity.w_mean.copy_(0.1 * torch.randn(cfg["n"], cfg["dz"], generator=g))
    m.decoder.decode.weight.copy_(0.25 * torch.randn(cfg["dy"], cfg["dz"], generator=g))
    m.decoder.decode.bias.copy_(0.5 + 0.1 * torch.randn(cfg["dy"], generator=g))
    return m


def record(mdl, cfg):
    """(y (T, B, d_y) of counts, x0 (B, d_z)): Poisson draws at the decoder's image of the mean map's own trajectory from x0."""
    g = torch.Generator().manual_seed(2)
    T, B, d = cfg["T"], cfg["B"], cfg["dz"]
    x0 = torch.randn(B, d, generator=g).cuda()
    x = mdl.transition.forecast_sequence(x0, None, T)[1:]
    y = torch.poisson(mdl.decoder(x).clamp(max=8.0).exp().cpu(), generator=g).cuda()
    return y.contiguous(), x0


def torch_loop(mdl, y, x0, n_iter):
    """The loop a user writes today: the contract in torch.  -> (mean, var, loglik, grad_norm) of the rows given."""
    vel = mdl.transition.velocity
    C, b = mdl.decoder.decode.weight, mdl.decoder.decode.bias
    T, B, dy = y.shape
    d = x0.shape[1]
    eye = torch.eye(d, device=y.device)
    mean, var = torch.empty(T, B, d, device=y.device), torch.empty(T, B, d, device=y.device)
    ll, gnorm = torch.empty(T, B, device=y.device), torch.empty(T, B, device=y.device)
    m, P = x0, P0 * eye.expand(B, d, d)

    def E(mp, Lp, yt, z):
        eta = (mp + (Lp @ z[:, :, None])[:, :, 0]) @ C.T + b
        lam = eta.exp()
        return lam, (lam - yt * eta).sum(1) + 0.5 * (z * z).sum(1)

    def D(Lp, yt, z, lam):
        H = torch.einsum("bj,ji,jp->bip", lam, C, C)
        Lm = torch.linalg.cholesky(eye + Lp.transpose(1, 2) @ H @ Lp)
        grad = z - (Lp.transpose(1, 2) @ ((yt - lam) @ C)[:, :, None])[:, :, 0]
        return Lm, grad, -torch.cholesky_solve(grad[:, :, None], Lm)[:, :, 0]

    for t in range(T):
        J = mdl.jacobian(m)
        mp = m + features(vel, m) @ vel.w_mean
        Lp = torch.linalg.cholesky(J @ P @ J.transpose(1, 2) + Q * eye)
        z = torch.zeros_like(mp)
        lam, phi = E(mp, Lp, y[t], z)
        Lm, grad, dz = D(Lp, y[t], z, lam)
        alpha = torch.ones(B, device=y.device)
        for _ in range(n_iter):
            zc = z + alpha[:, None] * dz
            lamc, phic = E(mp, Lp, y[t], zc)
            acc = (phic <= phi) & torch.isfinite(phic)
            z, lam, phi = torch.where(acc[:, None], zc, z), torch.where(acc[:, None], lamc, lam), torch.where(acc, phic, phi)
            Lm, grad, dn = D(Lp, y[t], z, lam)
            dz = torch.where(acc[:, None], dn, dz)
            alpha = torch.where(acc, torch.ones_like(alpha), alpha / 4)
        m = mp + (Lp @ z[:, :, None])[:, :, 0]
        Y = torch.linalg.solve_triangular(Lm, Lp.transpose(1, 2), upper=False)
        P = Y.transpose(1, 2) @ Y
        ll[t] = -(phi + torch.lgamma(y[t] + 1).sum(1) + torch.diagonal(Lm, dim1=1, dim2=2).log().sum(1))
        gnorm[t] = grad.norm(dim=1)
        mean[t], var[t] = m, torch.diagonal(P, dim1=1, dim2=2)
    return mean, var, ll, gnorm


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
    ap.add_argument("--loop-rows", type=int, default=200, help="rows the torch loop is timed over at most")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "laplace_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "laplace_bench needs a GPU"
    import vjf_amd
    lines = []
    with torch.no_grad():
        for cfg in RUNS:
            mdl = model(cfg)
            y, x0 = record(mdl, cfg)
            T = cfg["T"]
            lr = min(T, a.loop_rows)
            prior = vjf_amd.Gaussian(x0, torch.full_like(x0, math.log(P0)))
            rows = {"torch_loop": lr, "native": T, "native_iter1": T}
            variants = {"torch_loop": lambda: torch_loop(mdl, y[:lr], x0, N_ITER),
                        "native": lambda: mdl.laplace_filter(y, x0=prior, state_var=Q, n_iter=N_ITER),
                        "native_iter1": lambda: mdl.laplace_filter(y, x0=prior, state_var=Q, n_iter=1)}
            ref, got = variants["torch_loop"](), variants["native"]()
            diff = {"mean": float((got.mean[:lr] - ref[0]).abs().max() / ref[0].abs().max().clamp(min=1.)),
                    "var": float((got.var[:lr] - ref[1]).abs().max() / ref[1].abs().max()),
                    "loglik": float((got.loglik[:lr] - ref[2]).abs().max() / ref[2].abs().max())}
            calls = {}
            for k, fn in variants.items():                               # warm-up, and the size of a region
                fn()
                calls[k] = max(1, math.ceil(1.3 * a.region / max(region(fn, 1), 1e-6)))
            times = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():                           # alternating
                    times[k].append(region(fn, calls[k]) / calls[k] / rows[k] * 1e6)
            med = {k: statistics.median(v) for k, v in times.items()}
            line = {"bench": "laplace_filter", "shape": cfg["shape"], "trials": cfg["B"], "rows": T, "loop_rows": lr, "d_z": cfg["dz"],
                    "d_y": cfg["dy"], "n_rbf": cfg["n"], "state_var": Q, "n_iter": N_ITER, "mean_count": round(float(y.mean()), 3),
                    "unit": "us per row", "reps": a.reps,
                    **{k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3), "calls_per_region": calls[k],
                           "region_s": round(med[k] * calls[k] * rows[k] * 1e-6, 3)} for k, v in times.items()},
                    "speedup": round(med["torch_loop"] / med["native"], 2),
                    "iter8_over_iter1": round(med["native"] / med["native_iter1"], 2),
                    "faster_beyond_spread": max(times["native"]) < min(times["torch_loop"]),
                    "largest_grad_norm": float(f"{float(got.grad_norm.max()):.3g}"), "kernel_trace": False,
                    "largest_difference_over_scale": {k: float(f"{v:.3g}") for k, v in diff.items()}}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
