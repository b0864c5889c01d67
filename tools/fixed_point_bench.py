"""`fixed_points` (one native call: vjf_fixed_points) against the loop a user writes without it: a plain Newton iteration, per step
one `model.jacobian` call, torch on the GPU for the features and g, `torch.linalg.solve`, and a host check of the residual that
decides when to stop.

    python tools/fixed_point_bench.py [--reps 5] [--region 0.3] [--out profiles/fixed_point_bench.json]

Shapes: one Lorenz-sized model (configs[0]'s dimensions: d_z = 3, RBF(100)) with 64 starts, and configs[1]'s dimensions (d_z = 10,
RBF(200)) with 4096 starts.  Both searches run to tol = 1e-5 with at most 64 iterations from the same starts: roots are planted in the
model (as tests/fixed_point_cases.py plants them) and a start is a root plus 0.3 N(0, 1).  The baseline is the torch loop, never the
code under test.  The two variants alternate in one process, each timed over a region of whole calls that lasts at least --region
seconds (sized in the warm-up) and ends in a device synchronise.  Per shape one JSON line: the median and the spread (min .. max) of
--reps regions per variant in ms per call, the ratio of the medians, whether every native region is shorter than every region of the
loop, the iterations each took (the loop: until every start is within tol or the cap; native: the largest and the mean n_iter) and the
share of starts each converges -- in all, and to a point among the centroids (|x|_inf <= 2.5: far from them g vanishes, and a search
that ends on that plateau is within tol without a fixed point being there).  No ratio is promised: the exit code is 0 whatever the outcome, the `faster_beyond_spread` field says it.
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

RUNS = [dict(shape="configs[0]", B=64, dz=3, dy=10, n=100, hidden=[20]),
        dict(shape="configs[1]", B=4096, dz=10, dy=50, n=200, hidden=[128])]
TOL, MAX_ITER, N_ROOTS, PERT = 1e-5, 64, 6, 0.3


def features(vel, x):
    c = vel.feature.centroid
    return torch.exp(-.5 * ((x[:, None, :] - c[None]) ** 2).sum(-1) * torch.exp(-2. * vel.feature.logwidth))


def model(cfg):
    """Weights of 0.5 N(0, 1) with N_ROOTS roots planted: w <- w - Phi*^T (Phi* Phi*^T)^-1 Phi* w in fp64.  -> (model, roots)"""
    import vjf_amd
    torch.manual_seed(0)
    m = vjf_amd.VJF.make_model(cfg["dy"], cfg["dz"], 0, cfg["n"], cfg["hidden"], likelihood="gaussian", noise="device")
    g = torch.Generator().manual_seed(1)
    vel = m.transition.velocity
    w = (0.5 * torch.randn(cfg["n"], cfg["dz"], generator=g)).double()
    roots = (3. * torch.rand(N_ROOTS, cfg["dz"], generator=g) - 1.5).cuda()
    P = features(vel, roots).double().cpu()
    vel.w_mean.copy_((w - P.T @ torch.linalg.solve(P @ P.T, P @ w)).float())
    return m, roots


def torch_loop(mdl, x0):
    """The loop a user writes today: plain Newton on g = 0.  -> (x, residual (B,), iterations)"""
    vel = mdl.transition.velocity
    eye = torch.eye(x0.shape[1], device=x0.device)
    x, it = x0, 0
    while True:
        g = features(vel, x) @ vel.w_mean
        res = g.norm(dim=1)
        if it == MAX_ITER or not bool((res > TOL).any()):            # (the host decides: one round trip per iteration)
            return x, res, it
        A = mdl.jacobian(x) - eye
        # (solve_ex: torch.linalg.solve without its check, which raises once a diverging start has left the centroids and A = 0 there)
        x = x - torch.linalg.solve_ex(A, g[:, :, None])[0][:, :, 0]
        it += 1


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fixed_point_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fixed_point_bench needs a GPU"
    lines = []
    with torch.no_grad():
        for cfg in RUNS:
            mdl, roots = model(cfg)
            B = cfg["B"]
            x0 = (roots[torch.arange(B) % N_ROOTS] + PERT * torch.randn(B, cfg["dz"], generator=torch.Generator().manual_seed(2)).cuda()).contiguous()
            variants = {"torch_loop": lambda: torch_loop(mdl, x0),
                        "native": lambda: mdl.fixed_points(x0, max_iter=MAX_ITER, tol=TOL),
                        "native_no_jacobian": lambda: mdl.fixed_points(x0, max_iter=MAX_ITER, tol=TOL, return_jacobian=False)}
            xl, resl, itl = variants["torch_loop"]()
            fp = variants["native"]()
            okl = torch.isfinite(resl) & (resl <= TOL)
            inside = lambda x: x.abs().amax(dim=1) <= 2.5                # noqa: E731
            calls = {}
            for k, fn in variants.items():                               # warm-up, and the size of a region
                fn()
                calls[k] = max(1, math.ceil(1.3 * a.region / max(region(fn, 1), 1e-6)))
            times = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():                           # alternating
                    times[k].append(region(fn, calls[k]) / calls[k] * 1e3)
            med = {k: statistics.median(v) for k, v in times.items()}
            line = {"bench": "fixed_points", "shape": cfg["shape"], "starts": B, "d_z": cfg["dz"], "n_rbf": cfg["n"], "tol": TOL, "max_iter": MAX_ITER,
                    "start_perturbation": PERT, "unit": "ms per call", "reps": a.reps,
                    **{k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4), "calls_per_region": calls[k],
                           "region_s": round(med[k] * calls[k] * 1e-3, 3)} for k, v in times.items()},
                    "speedup": round(med["torch_loop"] / med["native"], 2),
                    "faster_beyond_spread": max(times["native"]) < min(times["torch_loop"]),
                    "iterations": {"torch_loop": itl, "native_max": int(fp.n_iter.max()), "native_mean": round(float(fp.n_iter.float().mean()), 2)},
                    "converged_share": {"torch_loop": round(float(okl.float().mean()), 4), "native": round(float(fp.converged.float().mean()), 4)},
                    # g vanishes far from the centroids (they lie in [-2, 2]): a search that ends out there is within tol of a plateau
                    "converged_among_centroids_share": {"torch_loop": round(float((okl & inside(xl)).float().mean()), 4),
                                                        "native": round(float((fp.converged & inside(fp.x)).float().mean()), 4)}}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
