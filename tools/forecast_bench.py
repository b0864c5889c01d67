"""`forecast` (one Python iteration, two host round trips and several launches per step) against `forecast_sequence` (one native
call per horizon: vjf_forecast_seq).

    python tools/forecast_bench.py [--steps 200] [--reps 5] [--region 0.3] [--out profiles/forecast_bench.json]

Shapes: configs[0] (B = 1, d_z = 3, RBF(100)) and configs[1] (B = 4096, d_z = 10, RBF(200)), a horizon of --steps steps, state noise
off and on.  Three variants alternate in one process, each timed over a region of whole calls that lasts at least --region seconds
(sized in the warm-up) and ends in a device synchronise, decoding included:
    forecast              the per-step loop, noise="reference" (the CPU generator): the baseline
    forecast_sequence     the same model, the same draws on the CPU generator
    forecast_sequence_dev a model with noise="device": both noise tensors drawn on the GPU, one call each
Per shape and noise setting one JSON line: the median and the spread (min .. max) of --reps regions per variant in us per step,
the ratios of the medians, and the largest difference between the two drop-in variants' roll-outs under one seed.  Exit code 1 (and
a line on stderr) when a `forecast_sequence` variant is not faster than `forecast` by more than the spread: every one of its regions
shorter than every region of `forecast`.
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

SHAPES = {"configs[0]": dict(B=1, dz=3, dy=10, n=100, hidden=[20]),
          "configs[1]": dict(B=4096, dz=10, dy=50, n=200, hidden=[128])}


def model(cfg, noise):
    """A model whose roll-out stays among its centroids: small weights with a small spread (a fitted model's, not the constructor's
    identity covariance)."""
    import vjf_amd
    torch.manual_seed(0)
    m = vjf_amd.VJF.make_model(cfg["dy"], cfg["dz"], 0, cfg["n"], cfg["hidden"], likelihood="gaussian", noise=noise)
    vel = m.transition.velocity
    g = torch.Generator().manual_seed(1)
    vel.w_mean.copy_(0.05 * torch.randn(cfg["n"], cfg["dz"], generator=g))
    vel.w_chol.copy_(0.05 * torch.eye(cfg["n"]))
    m.transition.logvar.fill_(math.log(0.01))
    return m


def region(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--region", type=float, default=0.3, help="least length of a timed region, seconds")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "forecast_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "forecast_bench needs a GPU"
    T, lines = a.steps, []
    for name, cfg in SHAPES.items():
        ref, dev = model(cfg, "reference"), model(cfg, "device")
        x0 = torch.randn(cfg["B"], cfg["dz"], generator=torch.Generator().manual_seed(2)).cuda()
        for noise in (False, True):
            variants = {"forecast": lambda: ref.forecast(x0, None, T, noise=noise),
                        "forecast_sequence": lambda: ref.forecast_sequence(x0, None, T, noise=noise),
                        "forecast_sequence_dev": lambda: dev.forecast_sequence(x0, None, T, noise=noise)}
            torch.manual_seed(3)
            xa, ya = variants["forecast"]()
            torch.manual_seed(3)
            xb, yb = variants["forecast_sequence"]()
            diff = max(float((xa - xb).abs().max()), float((ya - yb).abs().max()))
            assert math.isfinite(diff) and float(xa.abs().max()) < 100
            calls = {}
            for k, fn in variants.items():                               # warm-up, and the size of a region
                fn()
                calls[k] = max(1, math.ceil(1.3 * a.region / max(region(fn, 2) / 2, 1e-6)))   # (a margin: later calls run faster)
            times = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():                           # alternating
                    times[k].append(region(fn, calls[k]) / (calls[k] * T) * 1e6)
            med = {k: statistics.median(v) for k, v in times.items()}
            line = {"bench": "forecast", "shape": name, "B": cfg["B"], "d_z": cfg["dz"], "n_rbf": cfg["n"], "n_step": T, "noise": noise,
                    "unit": "us per step (decoding included)", "reps": a.reps,
                    **{k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3), "calls_per_region": calls[k],
                           "region_s": round(med[k] * calls[k] * T * 1e-6, 3)} for k, v in times.items()},
                    "speedup_sequence": round(med["forecast"] / med["forecast_sequence"], 2),
                    "speedup_sequence_dev": round(med["forecast"] / med["forecast_sequence_dev"], 2),
                    "faster_beyond_spread": max(times["forecast_sequence"]) < min(times["forecast"]),
                    "dev_faster_beyond_spread": max(times["forecast_sequence_dev"]) < min(times["forecast"]),
                    "max_abs_diff_same_seed": diff}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    slow = [(ln["shape"], ln["noise"], k) for ln in lines for k in ("faster_beyond_spread", "dev_faster_beyond_spread") if not ln[k]]
    if slow:                                                                 # the one hard requirement: never pass silently
        print("FAILED: forecast_sequence is NOT faster than forecast beyond the measured spread at", slow, file=sys.stderr, flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
