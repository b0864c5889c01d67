"""S `forecast_sequence` calls, a stack and `torch.var_mean` (what a user writes without it) against one `forecast_ensemble` call
(vjf_forecast_ens).

    python tools/ensemble_bench.py [--steps 200] [--reps 5] [--region 0.3] [--out profiles/ensemble_bench.json]

Shapes: configs[0] with B = 1 and S = 64 (one Lorenz trial, the example's case) and configs[1] with B = 4096 and S = 16, a horizon of
--steps steps, noise="device" (weight and state noise drawn on the GPU).  Two variants alternate in one process, each warmed up and
timed over regions of whole ensembles that last at least --region seconds (sized in the warm-up) and end in a device synchronise:
    loop                S forecast_sequence calls on one model, torch.stack, torch.var_mean over the members of x and of the decoded y
    forecast_ensemble   one call
Per shape one JSON line: the median and the spread (min .. max) of --reps regions per variant in ms per ensemble, and the ratio of
the medians.  Exit code 1 (and a line on stderr) unless every region of the ensemble call is shorter than every region of the loop at
B = 1, and no region of it is longer than the loop's longest at B = 4096.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from forecast_bench import SHAPES, model, region    # noqa: E402

MEMBERS = {"configs[0]": 64, "configs[1]": 16}


def loop(m, x0, T, S):
    xs, ys = zip(*[m.forecast_sequence(x0, None, T, noise=True) for _ in range(S)])
    xv, xm = torch.var_mean(torch.stack(xs), 0, unbiased=False)
    yv, ym = torch.var_mean(torch.stack(ys), 0, unbiased=False)
    return xm, xv, ym, yv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--region", type=float, default=0.3, help="least length of a timed region, seconds")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ensemble_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ensemble_bench needs a GPU"
    T, lines = a.steps, []
    for name, cfg in SHAPES.items():
        S = MEMBERS[name]
        m = model(cfg, "device")
        x0 = torch.randn(cfg["B"], cfg["dz"], generator=torch.Generator().manual_seed(2)).cuda()
        variants = {"loop": lambda: loop(m, x0, T, S),
                    "forecast_ensemble": lambda: m.forecast_ensemble(x0, None, T, S, noise=True)[:4]}
        # both estimate the same moments from independent draws: finite, and of one magnitude
        ra, rb = variants["loop"](), variants["forecast_ensemble"]()
        for p, q in zip(ra, rb):
            assert p.shape == q.shape and torch.isfinite(p).all() and torch.isfinite(q).all()
        assert float(ra[0].abs().max()) < 100 and float(rb[0].abs().max()) < 100
        del ra, rb
        calls = {}
        for k, fn in variants.items():                               # warm-up, and the size of a region
            fn()
            calls[k] = max(1, math.ceil(1.3 * a.region / max(region(fn, 2) / 2, 1e-6)))   # (a margin: later calls run faster)
        times = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, fn in variants.items():                           # alternating
                times[k].append(region(fn, calls[k]) / calls[k] * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        line = {"bench": "forecast_ensemble", "shape": name, "B": cfg["B"], "d_z": cfg["dz"], "d_y": cfg["dy"], "n_rbf": cfg["n"], "n_step": T,
                "n_sample": S, "noise": "device", "unit": "ms per ensemble (draws, decoding and moments included)", "reps": a.reps,
                **{k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3), "calls_per_region": calls[k],
                       "region_s": round(med[k] * calls[k] * 1e-3, 3)} for k, v in times.items()},
                "speedup": round(med["loop"] / med["forecast_ensemble"], 2),
                "every_region_shorter": max(times["forecast_ensemble"]) < min(times["loop"]),
                "no_region_longer_than_the_loops_longest": max(times["forecast_ensemble"]) <= max(times["loop"])}
        line["criterion"] = "every_region_shorter" if cfg["B"] == 1 else "no_region_longer_than_the_loops_longest"
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    slow = [ln["shape"] for ln in lines if not ln[ln["criterion"]]]
    if slow:                                                                 # the hard requirement: never pass silently
        print("FAILED: forecast_ensemble misses its criterion against the loop of forecast_sequence calls at", slow, file=sys.stderr, flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
