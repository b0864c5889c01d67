"""The shape classes of tests/shape_range_cases.py on the CPU: the yardstick's conditions at every shape, op and kind; the planners'
edges and the (cl, vg) class of every shape, through the real library's plan entry points (host-only code); the indefinite covariance
the GPU test poisons a trial with; and the seven family cases' values, which registering the new shapes must not move."""
import hashlib

import numpy as np
import pytest

from tests import ekf_cases as ec
from tests import fixed_point_cases as fpc
from tests import sampler_cases as pc
from tests import shape_range_cases as rc
from tests import smoother_cases as sc
from vjf_amd import _native as N


# ------------------------------------------------------------------ the family cases keep their seeds and values
def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            a = np.ascontiguousarray(a)
            h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()[:16]


# sha256 of what the seeds alone decide (the state, the decoder, lv, u, x0, the noise, the gap pattern), taken before EXTRA existed
DRAWS = {"ragged3": "ae49225d63ac129d", "control": "560ed551da9896ae", "wide": "0474903d2e2db17f", "configB": "7824c512bc7e6232",
         "beyond256": "802069b22e1b5766", "x24": "9e899625b50bd984", "scalar": "6f1d3b9ba8190376"}


def _family_values(name):
    s = sc.state(name)
    a, e = sc.inputs(name, "mixed"), ec.inputs(name, "sharp")
    drawn = (s.centroid, s.logwidth, s.w_mean, *ec.decoder(name), a["lv"], a["u"], e["x0"], e["lv0"], ec.observed(name), pc.noise(name))
    return _digest(*drawn), _digest(a["mu"], e["y"])


def test_the_family_cases_keep_their_seeds_and_values(monkeypatch):
    assert list(sc.CASES) == list(DRAWS) and set(pc.MEMBERS) == set(DRAWS) and not set(sc.EXTRA) & set(DRAWS)
    assert [sc.case_index(k) for k in DRAWS] == [2, 1, 3, 0, 100, 200, 201]
    with_extra = {name: _family_values(name) for name in DRAWS}
    # the same with nothing registered and nothing cached: the trajectories and records (numpy's exp is in them) bit for bit
    for mod, attr in ((sc, "EXTRA"), (sc, "_SEQ"), (ec, "_IN"), (pc, "EXTRA_MEMBERS")):
        monkeypatch.setattr(mod, attr, {})
    for name, want in DRAWS.items():
        assert _family_values(name) == with_extra[name], name
        assert with_extra[name][0] == want, (name, with_extra[name][0])


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name,kind", rc.smooth_cases())
def test_yardstick_smoother_and_sampler(name, kind):
    ref = sc.references(name, kind)
    for what in ("mean", "var", "cov"):
        sc.bound(what, *ref[what])
    pc.bound(*pc.references(name, kind))
    xdim, udim, n, ydim, B, T = rc.shape(name)
    assert pc.references(name, kind)[0].shape == (rc.MEMBERS[name], T, B, xdim)


@pytest.mark.parametrize("name,regime,gaps", rc.ekf_cases())
def test_yardstick_ekf(name, regime, gaps):
    ref = ec.references(name, regime, gaps)
    for what in ec.TENSORS:
        ec.bound(what, *ref[what])


@pytest.mark.parametrize("name", rc.names(rc.FP))
def test_yardstick_fixed_points(name):
    ref = rc.fp_references(name)
    assert np.abs(ref["x"][0] - rc.fp_inputs(name)["x0"]).max() > 1e-2          # (a step was taken)
    for what in ("x", "residual", "jacobian"):
        fpc.bound(*ref[what])


def test_the_table_of_shapes():
    assert rc.smooth_cases() == rc.sample_cases() and len(rc.smooth_cases()) == 2 * 11 + 2 and len(rc.ekf_cases()) == 3 * 9 + 2
    assert len(rc.names(rc.FP)) == 12
    for name, (shape, index, ops, why) in rc.SHAPES.items():
        assert shape[4] == 17 and shape[5] <= 4 and sc.shape(name) == shape and sc.case_index(name) == index
    assert len({v[1] for v in rc.SHAPES.values()}) == len(rc.SHAPES)


# ------------------------------------------------------------------ the planners, through the real library
@pytest.fixture(autouse=True)
def _free_plans(monkeypatch):
    for k in ("VJF_FC_CENTROID_LDS", "VJF_EKF_DECODER_LDS", "VJF_SMS_MEMBERS"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("op,name", [(rc.SM, "sm24max"), (rc.SM, "sm30max"), (rc.SP, "sm24max"), (rc.SP, "sm30max"), (rc.EKF, "ekf24max"),
                                     (rc.EKF, "ekf27max"), (rc.FP, "fp32max")])
def test_the_largest_n_the_planner_admits(op, name):
    """n is accepted, n + 1 is refused for LDS, and so is every n up to 64 beyond it (the budget is monotone in n)."""
    xdim, udim, n, ydim, B, T = rc.shape(name)
    assert rc.plan(op, n, xdim + udim, xdim, ydim)[0] == 0
    for more in range(1, 65):
        assert rc.plan(op, n + more, xdim + udim, xdim, ydim)[0] == -11, (op, name, n + more)
        assert b"LDS" in N.lib().vjf_last_error()
    vg, cl = rc.form_of(op, name)[:2]
    if op != rc.SP:                          # (the sampler is refused where the smoother is; its own buffers are smaller)
        assert (vg, cl) == (1, False)


def test_the_table_of_the_largest_n():
    """The limits the documents state: udim = 0 and udim = 8 at each xdim beyond 24."""
    def largest(op, dout, udim):
        n = 0
        while rc.plan(op, n + 1, dout + udim, dout)[0] == 0:
            n += 1
        return n
    got = {(op, dout, udim): largest(op, dout, udim) for op, douts in ((rc.SM, (24, 25, 27, 28, 30, 31, 32)), (rc.EKF, (24, 25, 27, 28)),
                                                                      (rc.FP, (24, 32))) for dout in douts for udim in (0, 8)}
    print(got)
    assert [got[rc.SM, k, 0] for k in (24, 25, 27, 28, 30, 31, 32)] == [753, 660, 463, 360, 141, 27, 0]
    assert [got[rc.SM, k, 8] for k in (24, 27, 30, 31)] == [746, 456, 134, 20]
    assert [got[rc.EKF, k, 0] for k in (24, 25, 27, 28)] == [461, 344, 96, 0]
    assert [got[rc.EKF, k, 8] for k in (24, 27)] == [454, 89]
    assert (got[rc.FP, 32, 0], got[rc.FP, 32, 8], got[rc.FP, 24, 0]) == (410, 402, 1043)
    for dout in (24, 25, 27, 30, 31):        # the sampler admits exactly what the smoother does
        n = got[rc.SM, dout, 0]
        assert rc.plan(rc.SP, n, dout, dout)[0] == 0 and rc.plan(rc.SP, n + 1, dout, dout)[0] == -11


def test_every_shape_lands_in_its_class():
    form = {(op, name): rc.form_of(op, name) for name, v in rc.SHAPES.items() for op in v[2]}
    print(form)
    # one live accumulator of the four in flow_evaluate
    for key in ((rc.SM, "sm24max"), (rc.SM, "sm30max"), (rc.SM, "x31"), (rc.EKF, "ekf24max"), (rc.EKF, "ekf27max"), (rc.FP, "fp32max")):
        assert form[key][0] == 1, (key, form[key])
    # cl = false by the plan itself
    for key in ((rc.SM, "x30u8"), (rc.SM, "x31"), (rc.SM, "corner"), (rc.EKF, "x27u8"), (rc.EKF, "corner")):
        assert form[key][1] is False, (key, form[key])
    assert form[rc.SM, "x30u8"][0] == 2
    # a last group that is not whole: fewer columns per pass than dout, and not a multiple of VJF_FLOW_MV
    for op in rc.ALL:
        assert any(f[0] < rc.shape(name)[0] and f[0] % 4 for (o, name), f in form.items() if o == op), op
    # everything in LDS, every column in one pass
    for name in ("x15", "x16u8", "x2n1", "n3u1"):
        for op in rc.ALL:
            assert form[op, name][:2] == (rc.shape(name)[0], True), (op, name, form[op, name])
    # the members go in several chunks where the table says so
    for name, S in rc.MEMBERS.items():
        assert 1 <= form[rc.SP, name][2] <= S and (S != 17 or form[rc.SP, name][2] < S), (name, form[rc.SP, name])


# ------------------------------------------------------------------ the indefinite covariance
@pytest.mark.parametrize("dout,j", [(27, 15), (27, 16), (27, 26), (16, 15)])
def test_the_indefinite_covariance_fails_at_its_pivot(dout, j):
    P = rc.valid_cov(dout, 900 + dout)
    np.linalg.cholesky(P.astype(np.float32))
    bad = rc.indefinite(P, j)
    assert bad.dtype == np.float32 and np.array_equal(bad, bad.T) and np.isfinite(bad).all()
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(bad)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(bad.astype(np.float64))
    np.linalg.cholesky(bad[:j, :j])                                    # every pivot before j is positive ...
    with pytest.raises(np.linalg.LinAlgError):                         # ... and pivot j is the one that is not
        np.linalg.cholesky(bad[:j + 1, :j + 1])
    # the leading block is the valid covariance's, and the fp32 pivot is -L[j, j]^2 far beyond rounding
    assert np.abs(bad[:j, :j] - P[:j, :j]).max() <= 2 ** -23 * np.abs(P).max()
    Lj = np.linalg.cholesky(P)[j]
    s = np.linalg.solve(np.linalg.cholesky(bad[:j, :j].astype(np.float64)), bad[:j, j].astype(np.float64))
    assert bad[j, j] - s @ s < -0.5 * Lj[j] ** 2 < 0
