"""`score_forecast` (one native call: vjf_kstep_score) against the loop a user writes without it: the record flattened to starts,
`forecast_sequence` from them with zero weight noise, the decoder on every state, the subtraction, the square and the masked sum in
torch, chunked over origins where memory demands.

    python tools/kstep_bench.py [--reps 5] [--region 0.3] [--out profiles/kstep_bench.json]

Shapes: one Lorenz-sized trial (configs[0]'s dimensions: d_z = 3, RBF(100)) over 10 000 rows with K = 32, and 4096 trials of
configs[1]'s dimensions (d_z = 10, d_y = 50, RBF(200)) over 200 rows with K = 16; the model and the sequence are
tools/smoother_bench.py's, y = decoder(mu) + 0.1 N(0, 1).  The baseline is the torch loop, never the code under test.  The variants
alternate in one process, each timed over a region of whole calls that lasts at least --region seconds (sized in the warm-up) and
ends in a device synchronise.  Per shape one JSON line: the median and the spread (min .. max) of --reps regions per variant in
milliseconds per call, the ratio of the medians, whether every native region is shorter than every region of the loop, and how far
the loop's sums lie from the native ones relative to their size.
What `speedup` measures is the loop's launch count and the traffic it forms ((K + 1) x starts x (d_z + d_y) floats) against one
pass that forms neither; it does not say how close the kernel is to the hardware's limits.  No ratio is promised: the exit code is 0
whatever the outcome.
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
from tools.smoother_bench import RUNS, model, region, sequence      # noqa: E402

HORIZON = {"configs[0]": 32, "configs[1]": 16}
LOOP_FLOATS = 1 << 28                      # the loop's states and decoded states of a chunk of origins stay below this many floats


def torch_loop(mdl, mu, y, K):
    """The loop a user writes today.  -> (sse_x (K+1, d), base_x, sse_y (K+1, dy), base_y) float64."""
    T, B, d = mu.shape
    dy = y.shape[-1]
    n = mdl.transition.velocity.w_mean.shape[0]
    zeros = torch.zeros(K, n, d, device=mu.device)
    out = [torch.zeros(K + 1, d, dtype=torch.float64, device=mu.device), torch.zeros(K + 1, d, dtype=torch.float64, device=mu.device),
           torch.zeros(K + 1, dy, dtype=torch.float64, device=mu.device), torch.zeros(K + 1, dy, dtype=torch.float64, device=mu.device)]
    per = max(1, LOOP_FLOATS // ((K + 1) * B * (d + dy)))
    hs = torch.arange(K + 1, device=mu.device)
    for t0 in range(0, T, per):
        t1 = min(T, t0 + per)
        x0 = mu[t0:t1].reshape(-1, d)
        x = mdl.transition.forecast_sequence(x0, None, K, w_noise=zeros).reshape(K + 1, t1 - t0, B, d)
        yh = mdl.decoder(x)
        idx = (torch.arange(t0, t1, device=mu.device)[None, :] + hs[:, None])          # (K+1, origins): the target rows
        ok = (idx <= T - 1)[:, :, None, None]
        idx = idx.clamp(max=T - 1)
        tx, ty = mu[idx], y[idx]
        out[0] += torch.where(ok, (x - tx) ** 2, 0.).sum((1, 2), dtype=torch.float64)
        out[1] += torch.where(ok, (x[:1] - tx) ** 2, 0.).sum((1, 2), dtype=torch.float64)
        out[2] += torch.where(ok, (yh - ty) ** 2, 0.).sum((1, 2), dtype=torch.float64)
        out[3] += torch.where(ok, (yh[:1] - ty) ** 2, 0.).sum((1, 2), dtype=torch.float64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--region", type=float, default=0.3, help="least length of a timed region, seconds")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kstep_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kstep_bench needs a GPU"
    from vjf_amd import _native as N
    lines = []
    with torch.no_grad():
        for cfg in RUNS:
            mdl = model(cfg)
            mu, _ = sequence(mdl, cfg)
            T, B, d, dy, K = cfg["T"], cfg["B"], cfg["dz"], cfg["dy"], HORIZON[cfg["shape"]]
            y = (mdl.decoder(mu) + 0.1 * torch.randn(T, B, dy, device="cuda", generator=torch.Generator("cuda").manual_seed(3))).contiguous()
            variants = {"torch_loop": lambda: torch_loop(mdl, mu, y, K), "native": lambda: mdl.score_forecast(mu, y, None, K)}
            ref, got = variants["torch_loop"](), variants["native"]()
            diff = max(float(((g - r).abs().max() / r.abs().max().clamp(min=1.))) for g, r in zip((got.sse_x, got.base_x, got.sse_y, got.base_y), ref))
            plan = {}
            lds, tiles, per, forms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
            if N.lib().vjf_kstep_score_plan(T, B, K, cfg["n"], d, d, dy, ctypes.byref(lds), ctypes.byref(tiles), ctypes.byref(per), ctypes.byref(forms)) == 0:
                plan = {"lds_bytes": lds.value, "tiles": tiles.value, "tiles_per_chunk": per.value, "forms": forms.value}
            calls = {}
            for k, fn in variants.items():                               # warm-up, and the size of a region
                fn()
                calls[k] = max(1, math.ceil(1.3 * a.region / max(region(fn, 1), 1e-6)))
            times = {k: [] for k in variants}
            for _ in range(a.reps):
                for k, fn in variants.items():                           # alternating
                    times[k].append(region(fn, calls[k]) / calls[k] * 1e3)
            med = {k: statistics.median(v) for k, v in times.items()}
            line = {"bench": "score_forecast", "shape": cfg["shape"], "trials": B, "rows": T, "n_step": K, "d_z": d, "d_y": dy, "n_rbf": cfg["n"],
                    "unit": "ms per call", "reps": a.reps, **plan,
                    "loop_floats_never_formed": (K + 1) * T * B * (d + dy),
                    **{k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4), "calls_per_region": calls[k],
                           "region_s": round(med[k] * calls[k] * 1e-3, 3)} for k, v in times.items()},
                    "speedup": round(med["torch_loop"] / med["native"], 2),
                    "faster_beyond_spread": max(times["native"]) < min(times["torch_loop"]),
                    "difference_over_scale": float(f"{diff:.3g}")}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
