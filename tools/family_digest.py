"""Digests of what the kernels that walk a tile of 16 trials over the learned flow return -- `fixed_points` (with the Jacobian), `smooth`
(with return_cov), `sample_posterior` and `ekf` -- for comparing two builds of the library byte for byte:

    VJF_LIB=NAME python tools/family_digest.py > FILE      (vjf_amd/libvjf_hip_NAME.so; once per build and setting, then diff the files)

One line per output array: `name shape dtype sha256 n_nonfinite`.  Inputs: every case of tests/fixed_point_cases.py (near and far
starts), tests/smoother_cases.py (its three kinds), tests/sampler_cases.py (the same kinds) and tests/ekf_cases.py (its three regimes,
and the typical one with the gap pattern) -- a ragged last tile, a control input, two output tiles, n > 256, xdim 24 and xdim 1 -- and
per entry point one input in which every element of a single trial's row is NaN.  The overrides a build reads (VJF_FC_CENTROID_LDS,
VJF_EKF_DECODER_LDS, VJF_SMS_MEMBERS) are the caller's to set: one process per setting.  It searches nothing and judges nothing.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POISONED = "ragged3"                     # the case whose trial 1 is poisoned


def emit(name, t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    bad = int((~np.isfinite(a)).sum()) if a.dtype.kind == "f" else 0
    print(name, "x".join(map(str, a.shape)) or "scalar", a.dtype, hashlib.sha256(a.tobytes()).hexdigest(), bad, flush=True)


def emit_fields(name, res, fields):
    for k in fields:
        v = getattr(res, k)
        if k == "head":
            emit(f"{name}.head_mean", v[0])
            emit(f"{name}.head_cov", v[1])
        elif v is not None:
            emit(f"{name}.{k}", v)


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def poisoned(a, *index):
    a = a.copy()
    a[index] = np.nan
    return a


def main():
    assert torch.cuda.is_available(), "family_digest needs a GPU"
    import vjf_amd
    from tests import ekf_cases as ec
    from tests import fixed_point_cases as fpc
    from tests import sampler_cases as pc
    from tests import smoother_cases as sc
    with torch.no_grad():
        for name in fpc.CASES:
            m = fpc.make_model(vjf_amd, name)
            runs = [(kind, fpc.inputs(name, kind)) for kind in fpc.PERT]
            if name == POISONED:
                runs.append(("nan", dict(runs[0][1], x0=poisoned(runs[0][1]["x0"], 1))))
            for kind, a in runs:
                out = m.fixed_points(dev(a["x0"]), dev(a["u"]), max_iter=fpc.MAX_ITER, tol=fpc.TOL, return_jacobian=True)
                emit_fields(f"fixed_points/{name}/{kind}", out, ("x", "residual", "converged", "n_iter", "jacobian"))
        for name in sc.CASES:
            m = sc.make_model(vjf_amd, name)
            T = sc.CASES[name][5]
            runs = [(kind, sc.inputs(name, kind)) for kind in sc.KINDS]
            if name == POISONED:
                runs.append(("nan", dict(runs[0][1], mu=poisoned(runs[0][1]["mu"], T // 2, 1))))
            z = pc.noise(name)
            for kind, a in runs:
                q = (dev(a["mu"]), dev(a["lv"]))
                emit_fields(f"smooth/{name}/{kind}", m.smooth(q, dev(a["u"]), state_var=sc.Q, return_cov=True), ("mean", "var", "cov", "head"))
                emit(f"sample_posterior/{name}/{kind}.x", m.sample_posterior(q, dev(a["u"]), z.shape[0], state_var=pc.Q, noise=dev(z)).x)
        for name in ec.CASES:
            m = ec.make_model(vjf_amd, name)
            T = ec.CASES[name][5]
            runs = [(regime, ec.inputs(name, regime), None) for regime in ec.REGIMES]
            runs.append(("typical-gaps", runs[0][1], ec.observed(name)))
            if name == POISONED:
                runs.append(("nan", dict(runs[0][1], y=poisoned(runs[0][1]["y"], T // 2, 1)), None))
            for regime, a, obs in runs:
                out = m.ekf(dev(a["y"]), dev(a["u"]), x0=vjf_amd.Gaussian(dev(a["x0"]), dev(a["lv0"])), state_var=a["q"], obs_var=a["r"],
                            observed=dev(obs), return_cov=True)
                emit_fields(f"ekf/{name}/{regime}", out, ("mean", "var", "cov", "loglik", "head"))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
