"""Shared by tests/test_shape_range_ref.py and tests/test_gpu_shape_range.py: the shape classes the planners of `fixed_points`, `smooth`,
`sample_posterior` and `ekf` admit and the family tests (seven shapes, xdim in {1, 3, 5, 10, 17, 24}, udim <= 2, n >= 9) never run.

The shapes are registered with smoother_cases (EXTRA: served by its helpers and by ekf_cases' and sampler_cases', kept out of the CASES
the family tests parametrise over), so states, filtered sequences, records, noise and references are built exactly as the families'
are, with seeds of their own; the seven family cases keep theirs (test_shape_range_ref.py holds their digests).  B = 17: a full tile
and a tile of one trial.

The rule is the families':  max|got - ref64| <= F * max(E, 8 eps_fp32 scale),  E = max|ref32 - ref64|, with the families' bound()
and its conditions (E <= 1e-4 scale, max|mean| < 100, max|draw| < 1000)."""
import numpy as np

from tests import fixed_point_cases as fpc
from tests import sampler_cases as pc
from tests import smoother_cases as sc

FP, SM, SP, EKF = "fp", "smooth", "sample", "ekf"
ALL, NO_EKF = (FP, SM, SP, EKF), (FP, SM, SP)
# name: ((xdim, udim, n_rbf, ydim, B, T), seed index, ops, the class it is there for)
SHAPES = {
    "x2n1": ((2, 0, 1, 3, 17, 4), 400, ALL, "n = 1"),
    "n3u1": ((5, 1, 3, 3, 17, 4), 401, ALL, "n < 4 with a control input"),
    "x17n5": ((17, 0, 5, 3, 17, 4), 402, ALL, "two output tiles, two wavefronts with an empty share of K"),
    "x15": ((15, 0, 24, 5, 17, 4), 301, ALL, "one clamped lane"),
    "x16u8": ((16, 8, 24, 5, 17, 4), 303, ALL, "the last NO = 1, udim = 8"),
    "x23u2": ((23, 2, 24, 5, 17, 4), 304, ALL, "inside 18-23"),
    "x25": ((25, 0, 24, 5, 17, 4), 305, ALL, "the first shape beyond 24"),
    "x27u8": ((27, 8, 24, 5, 17, 4), 307, ALL, "the EKF's largest xdim, udim = 8"),
    "x30u8": ((30, 8, 20, 5, 17, 4), 310, NO_EKF, "vg = 2, cl = false by plan"),
    "x31": ((31, 0, 20, 5, 17, 4), 309, NO_EKF, "the smoother at vg = 1"),
    "corner": ((24, 8, 256, 5, 17, 3), 315, ALL, "the guaranteed corner"),
    # the largest n the planners admit at these xdim (test_shape_range_ref.py finds them through the plan entry points)
    "sm24max": ((24, 0, 753, 5, 17, 3), 311, (SM, SP), "LDS edge"),
    "sm30max": ((30, 0, 141, 5, 17, 3), 312, (SM, SP), "LDS edge"),
    "ekf24max": ((24, 0, 461, 5, 17, 3), 314, (EKF,), "LDS edge"),
    "ekf27max": ((27, 0, 96, 5, 17, 3), 313, (EKF,), "LDS edge"),
    # (fixed points only: no sequence, so no T; its seed index is this module's choice)
    "fp32max": ((32, 0, 410, 9, 17, 1), 316, (FP,), "LDS edge at VJF_FP_MAXDOUT"),
}
MAX_ROWS = ("sm24max", "sm30max", "ekf24max", "ekf27max", "fp32max")
MEMBERS = {name: 17 if name in ("x30u8", "corner") else 3 for name, v in SHAPES.items() if SP in v[2]}
for _name, (_shape, _index, _ops, _why) in SHAPES.items():
    assert _name not in sc.CASES
    sc.EXTRA[_name] = (_shape, _index)
pc.EXTRA_MEMBERS.update(MEMBERS)

KINDS = ("typical", "mixed")                                                  # the smoother's and the sampler's
REGIMES = (("typical", True), ("sharp", False), ("vague", True))              # the EKF's (regime, gaps)
# The committed factors of the rule, one per op: start at 4, at most twice the worst ratio achieved on the MI355X, never above 16
# (profiles/shape_range_margins.json has every comparison), and never above the op's family factor (1.5, 1.3, 0.78, 3.3): no shape
# class here is further from fp64 than the family's worst.  Achieved on an MI355X, the worst three per op:
#   fixed points   0.686 (x30u8, x behind one step), 0.611 (x25, x), 0.607 (fp32max, x); residuals and Jacobians under 0.07
#   smooth         0.639 (x31, typical: var and cov), 0.609 (x15, typical: var and cov), 0.498 (sm24max: var and cov)
#   sample         0.330 (x15, mixed), 0.234 (corner, mixed), 0.207 (x17n5, mixed)
#   ekf            1.876 (corner, sharp: loglik), 1.804 (x17n5, sharp: mean), 1.782 (x25, sharp: mean); then 1.519 (ekf27max: var, cov)
F = {FP: 1.3, SM: 1.2, SP: 0.66, EKF: 3.3}


def names(op):
    return [name for name, v in SHAPES.items() if op in v[2]]


def shape(name):
    return SHAPES[name][0]


def kinds(name):
    """The *max rows run `typical` only: their numpy references are the slow part."""
    return KINDS[:1] if name in MAX_ROWS else KINDS


def regimes(name):
    return REGIMES[:1] if name in MAX_ROWS else REGIMES


def smooth_cases():
    return [(name, kind) for name in names(SM) for kind in kinds(name)]


def sample_cases():
    return [(name, kind) for name in names(SP) for kind in kinds(name)]


def ekf_cases():
    return [(name, regime, gaps) for name in names(EKF) for regime, gaps in regimes(name)]


# ---- fixed points: the shape's state as the smoother has it (no planted roots), one damped step from a start of its own
def fp_inputs(name):
    """float32 x0 (B, xdim) ~ U(-1.5, 1.5) and u (B, udim) ~ N(0, 1) or None."""
    xdim, udim, n, ydim, B, T = shape(name)
    r = np.random.default_rng(5000 + sc.case_index(name))
    x0 = r.uniform(-1.5, 1.5, (B, xdim)).astype(np.float32)
    return {"x0": x0, "u": r.standard_normal((B, udim)).astype(np.float32) if udim else None}


_FP = {}


def fp_references(name):
    """{"x" | "residual" | "jacobian": (ref64, ref32)} and "n_iter" of one damped step (max_iter = 1, damping = 1): once per process."""
    if name not in _FP:
        from tests import fixed_point_ref as fr
        a, s64 = fp_inputs(name), sc.state(name)
        r64, r32 = fpc.references(s64, a["x0"], a["u"], max_iter=1, tol=fpc.TOL, lam0=1.0)
        c = lambda v, dt: None if v is None else np.asarray(v, dt)          # noqa: E731
        _FP[name] = {"x": (r64[0], r32[0]), "residual": (r64[1], r32[1]), "n_iter": r64[2],
                     "jacobian": (fr.jacobian(s64, r64[0], c(a["u"], np.float64)),
                                  fr.jacobian(s64.cast(np.float32), r32[0], c(a["u"], np.float32)))}
    return _FP[name]


# ---- the planners, through the real library's plan entry points (host-only code)
def plan(op, n, d, dout, dy=5, S=3):
    """(return code, lds, members per workgroup) of the op's plan entry point."""
    import ctypes as C
    from vjf_amd import _native as N
    L, lds, members = N.lib(), C.c_int64(-1), C.c_int32(-1)
    if op == SM:
        r = L.vjf_smooth_plan(n, d, dout, C.byref(lds))
    elif op == SP:
        r = L.vjf_smooth_sample_plan(n, d, dout, S, C.byref(members), C.byref(lds))
    elif op == EKF:
        r = L.vjf_ekf_plan(n, d, dout, dy, C.byref(lds))
    else:
        r = L.vjf_fixed_points_plan(n, d, dout, C.byref(lds))
    return r, lds.value, members.value


def form_of(op, name):
    """(vg, cl) of the plan the library makes for the shape, recovered from the LDS it asks for (tests/tile_layouts.py); the EKF's
    (vg, cl, dl), the sampler's (vg, cl, sc)."""
    from tests import tile_layouts as tl
    xdim, udim, n, ydim, B, T = shape(name)
    d = xdim + udim
    r, lds, members = plan(op, n, d, xdim, ydim, MEMBERS.get(name, 3))
    assert r == 0 and 0 < lds <= tl.BUDGET, (op, name, r, lds)
    floats = {SM: lambda vg, cl: tl.smooth(n, d, xdim, vg, cl), FP: lambda vg, cl: tl.fixed_points(n, d, xdim, vg, cl),
              SP: lambda vg, cl: tl.sample(n, d, xdim, vg, members, cl), EKF: lambda vg, cl, dl: tl.ekf(n, d, xdim, ydim, vg, cl, dl)}[op]
    found = tl.forms(lds, xdim, floats, flags=2 if op == EKF else 1)
    assert len(found) == 1, (op, name, lds, found)          # (no two forms of these shapes ask for the same LDS)
    return found[0] + ((members,) if op == SP else ())


# ---- an indefinite covariance whose Cholesky factorisation fails at pivot j exactly
def indefinite(cov, j):
    """L D L^T in fp64 rounded to fp32: L the Cholesky factor of `cov` (dout, dout), D the identity with D[j, j] = -1.  Its leading
    j x j block is that of `cov`; pivot j of its factorisation is -L[j, j]^2."""
    L = np.linalg.cholesky(np.asarray(cov, np.float64))
    D = np.ones(L.shape[0])
    D[j] = -1.0
    return ((L * D) @ L.T).astype(np.float32)


def valid_cov(dout, seed):
    """A covariance of the size the kernels carry (variances near 0.05, moderate correlations), fp64."""
    r = np.random.default_rng(seed)
    A = r.standard_normal((dout, dout)) / np.sqrt(dout)
    return 0.05 * (np.eye(dout) + 0.5 * A @ A.T)


# trial (both tiles of B = 17 are hit) -> pivot, per shape
PIVOTS = {"x27u8": {16: 15, 9: 16, 13: 26}, "x16u8": {16: 15}}
