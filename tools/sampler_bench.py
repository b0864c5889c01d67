"""`sample_posterior` (one native call: vjf_smooth_sample) against the loop a user writes without it: backwards over the rows, per row
one `model.jacobian` call, the mean step in torch on the GPU, `torch.linalg.cholesky` of the predicted covariance and of the conditional
one, `cholesky_solve` for the gain, and the batched products that move all S members -- and against `smooth` on the same inputs.

    python tools/sampler_bench.py [--reps 5] [--region 0.3] [--loop-rows 1000] [--out profiles/sampler_bench.json]

Shapes: one Lorenz-sized trial (configs[0]'s dimensions: d_z = 3, RBF(100)) with S = 64 over 10 000 rows, and 4096 trials of configs[1]'s
dimensions (d_z = 10, RBF(200)) with S = 16 over 200 rows; inputs as tools/smoother_bench.py's (its model and its sequence), the noise
one torch.randn(S, T, B, d_z) drawn once outside the timed regions.  The baseline is the torch loop, never the code under test; where
the record is longer than --loop-rows the loop is timed over its last --loop-rows rows only and `loop_rows` says so.  The variants
alternate in one process, each timed over a region of whole calls that lasts at least --region seconds (sized in the warm-up) and ends
in a device synchronise.  Per shape one JSON line: the median and the spread (min .. max) of --reps regions per variant in microseconds
per row, the ratios of the medians, whether every native region is shorter than every region of the loop, and how far the loop's draws
lie from the native ones relative to scale (the loop factors the conditional covariance itself, another factor than L^-T, so the
same noise gives other draws: the comparison is made at zero noise, where both give the smoothed mean).
What `speedup` measures is the loop's launch count against one launch; `draws_over_smooth` is the cost of S joint draws in units of
one smoothing pass (the claim to check: of the order of one, not S); neither says how close the kernel is to the hardware's limits.
No ratio is promised: the exit code is 0 whatever the outcome.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.smoother_bench import Q, RUNS, features, model, region, sequence      # noqa: E402

MEMBERS = {"configs[0]": 64, "configs[1]": 16}


def torch_loop(mdl, mu, lv, z):
    """The loop a user writes today, textbook form.  z (S, T, B, d) -> x (S, T, B, d)."""
    vel = mdl.transition.velocity
    T, B, d = mu.shape
    eye = torch.eye(d, device=mu.device)
    x = torch.empty_like(z)
    cur = mu[-1] + (0.5 * lv[-1]).exp() * z[:, -1]
    x[:, -1] = cur
    for t in range(T - 2, -1, -1):
        J = mdl.jacobian(mu[t])
        mp = mu[t] + features(vel, mu[t]) @ vel.w_mean
        D = lv[t].exp()
        JD = J * D[:, None, :]
        Pp = JD @ J.transpose(1, 2) + Q * eye
        G = torch.cholesky_solve(JD, torch.linalg.cholesky(Pp)).transpose(1, 2)
        C = torch.diag_embed(D) - G @ JD
        Lc = torch.linalg.cholesky(0.5 * (C + C.transpose(1, 2)))
        cur = mu[t] + torch.einsum("bij,sbj->sbi", G, cur - mp) + torch.einsum("bij,sbj->sbi", Lc, z[:, t])
        x[:, t] = cur
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--region", type=float, default=0.3, help="least length of a timed region, seconds")
    ap.add_argument("--loop-rows", type=int, default=1000, help="rows the torch loop is timed over at most")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sampler_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sampler_bench needs a GPU"
    from vjf_amd import _native as N
    lines = []
    with torch.no_grad():
        for cfg in RUNS:
            mdl = model(cfg)
            mu, lv = sequence(mdl, cfg)
            T, B, d, S = cfg["T"], cfg["B"], cfg["dz"], MEMBERS[cfg["shape"]]
            lr = min(T, a.loop_rows)
            z = torch.randn(S, T, B, d, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
            rows = {"torch_loop": lr, "smooth": T, "native": T}
            variants = {"torch_loop": lambda: torch_loop(mdl, mu[T - lr:], lv[T - lr:], z[:, T - lr:]),
                        "smooth": lambda: mdl.smooth((mu, lv), state_var=Q),
                        "native": lambda: mdl.sample_posterior((mu, lv), None, S, state_var=Q, noise=z)}
            z0 = torch.zeros(2, lr, B, d, device="cuda")
            ref = torch_loop(mdl, mu[T - lr:], lv[T - lr:], z0)
            got = mdl.sample_posterior((mu[T - lr:], lv[T - lr:]), None, 2, state_var=Q, noise=z0).x
            diff = float((got - ref).abs().max() / ref.abs().max().clamp(min=1.))
            lds_members = {}
            sc, lds = ctypes.c_int32(), ctypes.c_int64()
            if N.lib().vjf_smooth_sample_plan(cfg["n"], d, d, S, ctypes.byref(sc), ctypes.byref(lds)) == 0:
                lds_members = {"members_per_workgroup": sc.value, "lds_bytes": lds.value}
            calls = {}
            for k, fn in variants.items():                               # warm-up, and the size of a region
                fn()
                calls[k] = max(1, math.ceil(1.3 * a.region / max(region(fn, 1), 1e-6)))
            times = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():                           # alternating
                    times[k].append(region(fn, calls[k]) / calls[k] / rows[k] * 1e6)
            med = {k: statistics.median(v) for k, v in times.items()}
            line = {"bench": "sample_posterior", "shape": cfg["shape"], "trials": B, "members": S, "rows": T, "loop_rows": lr, "d_z": d,
                    "n_rbf": cfg["n"], "state_var": Q, "unit": "us per row", "reps": a.reps, **lds_members,
                    **{k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3), "calls_per_region": calls[k],
                           "region_s": round(med[k] * calls[k] * rows[k] * 1e-6, 3)} for k, v in times.items()},
                    "speedup": round(med["torch_loop"] / med["native"], 2), "draws_over_smooth": round(med["native"] / med["smooth"], 2),
                    "faster_beyond_spread": max(times["native"]) < min(times["torch_loop"]),
                    "zero_noise_difference_over_scale": float(f"{diff:.3g}")}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
