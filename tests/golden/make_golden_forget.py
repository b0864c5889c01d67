#!/usr/bin/env python3
"""Golden trajectories of VJF.filter with a forgetting factor in the RLS update, from the imported reference (catniplab/vjf).

Run ONLY where the reference exists (as make_golden.py; VJF_REFERENCE names its checkout), from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_forget.py

The reference's `LinearRegression.rls` takes `shrink` (vjf/module.py:80-96) but its step passes 1 (vjf/model.py:371).  Here the
method is wrapped for the length of a trajectory so that the step's call runs with SHRINK; nothing else of the reference changes.
Files are named g10_forget* (never g5_*: tests/goldenio.traj_names globs g5_*.npz and runs those without forgetting) and have the
layout of make_golden.traj, plus `shrink`.  Only numpy arrays are written.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, traj        # noqa: E402  (puts the reference on sys.path)

from vjf.module import LinearRegression  # noqa: E402

SHRINK = 0.9


class forgetting:
    """Within the block every call of LinearRegression.rls runs with shrink=`lam`, whatever the caller passes."""
    def __init__(self, lam):
        self.lam = lam

    def __enter__(self):
        self.orig = orig = LinearRegression.rls
        lam = self.lam

        @functools.wraps(orig)
        def rls(module, x, target, v, shrink=1.):
            return orig(module, x, target, v, shrink=lam)
        LinearRegression.rls = rls

    def __exit__(self, *exc):
        LinearRegression.rls = self.orig


def main():
    # the shapes of the g5_gaussian_du2_wu0_* pair (make_golden.main)
    small = dict(B=32, dz=3, dy=10, n=16, hidden=[8], T=8)
    for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        name = f"g10_forget{SHRINK}_{tag}"
        with forgetting(SHRINK):
            traj(name, dtype=dt, lik="gaussian", du=2, warm_up=False, **small)
        path = os.path.join(OUT, name + ".npz")
        with np.load(path) as z:
            rec = {k: z[k] for k in z.files}
        rec["shrink"] = np.asarray(SHRINK, np.float64)
        np.savez_compressed(path, **rec)
    torch.set_default_dtype(torch.float32)
    files = [f for f in os.listdir(OUT) if f.startswith("g10_forget")]
    print("g10 files:", files, "bytes:", [os.path.getsize(os.path.join(OUT, f)) for f in files])


if __name__ == "__main__":
    main()
