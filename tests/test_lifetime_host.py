"""CPU side of the lifetime tests (tests/lifetime.py): the nine-call script through the host mirror on the oracle-backed stand-in
for the C ABI (tests/fake_backend.py) -- what `vjf_amd.VJF` itself owns across calls: the context and its growth, the blob, the
learning rates and the freeze flag in the scalars slot, the state round trip -- and, on the oracle alone, the conditions that keep the
GPU test (tests/test_gpu_lifetime.py) honest for every family."""
import warnings

import numpy as np
import pytest
import torch

from tests import fake_backend
from tests import lifetime as life
from tests.helpers import load_oracle_state
from vjf_amd import _native as N

cpu_only = pytest.mark.skipif(torch.cuda.is_available(), reason="the stand-in backend works on CPU tensors")


@pytest.fixture
def fake():
    undo = fake_backend.install()
    yield N._lib
    undo()


@cpu_only
@pytest.mark.parametrize("fam", ["mega", "mega_p", "serial"])
def test_script_through_the_host_mirror(fake, fam):
    """The script on a model whose C ABI is the stand-in, against the oracle stepped directly.  The stand-in computes in fp64 but
    keeps the state and the outputs where the device keeps them, in fp32 tensors (rounded after every step), so the bounds are the
    fp32 ones of the GPU test -- it is closer to the fp64 oracle than any fp32 arithmetic.  Along the way, what the host mirror owns:
    growth re-creates the context and keeps the blob; the halved learning rates and the freeze flag are in the scalars slot when call
    6 enters the library (and not before); `set_state(get_state())` changes nothing but SC_TRI_CLEAN and the status word, which it
    clears; `close()` followed by a call makes a new context."""
    import vjf_amd
    m = life.make_model(vjf_amd, fam)
    s64 = load_oracle_state(m, np.float64)
    s0 = s64.clone()
    blob_ptr = m._blob.data_ptr()
    seen = {}                                                  # call -> (scalars at entry into the library, context object)
    now = {}
    inner_seq, inner_step = fake.vjf_filter_seq, fake.vjf_filter_step

    def spy(inner):
        def f(ctx, *a):
            seen.setdefault(now["k"], (m._scalars.clone(), fake.ctxs[ctx.value]))
            return inner(ctx, *a)
        return f
    fake.vjf_filter_seq, fake.vjf_filter_step = spy(inner_seq), spy(inner_step)

    def pre(k, call, B):
        now["k"] = k
        if k == 7:
            # the round trip by hand first (the script's own follows): an identity but for the two words it clears
            m._scalars[N.SC_TRI_CLEAN] = 1.0
            st = m.get_state()
            m._scalars[N.SC_STATUS] = float(N.STATUS_RLS_FAILED)
            before = m._blob.clone()
            m.set_state(st)
            changed = (m._blob != before).nonzero().flatten().tolist()
            base = m._scalars.data_ptr() - m._blob.data_ptr()
            assert changed == [base // 4 + N.SC_STATUS, base // 4 + N.SC_TRI_CLEAN], changed
            assert float(m._scalars[N.SC_STATUS]) == 0.0 and float(m._scalars[N.SC_TRI_CLEAN]) == 0.0
            assert [g["lr"] for g in m.optimizer.param_groups] == [life.LR * 0.5] * 4

    ctx_batches = []
    for step in life.drive(fam, m, (s64,), pre=pre):
        life.compare_outputs(f"host[{fam}]", step, step.refs[0])
        assert m.check_status() == 0
        assert m._blob.data_ptr() == blob_ptr                  # one blob for the whole life
        ctx_batches.append(m._ctx_batch)
        assert len(fake.ctxs) == 1
    life.compare_state(f"host[{fam}]", m, s64, s64)
    assert (m._get_counter("lik"), m._get_counter("tr")) == life.expected_counters(fam)

    # growth: contexts for 64 trials, then (call 5) for 150; the smaller batches behind it are served by the grown one
    assert ctx_batches == [64, 64, 64, 64, 150, 150, 150, 150, 150]
    assert all(seen[k][1] is seen[1][1] for k in (2, 3, 4)) and all(seen[k][1] is seen[5][1] for k in (6, 7, 8, 9))
    assert seen[5][1] is not seen[1][1]
    assert seen[5][1].cfg.max_batch == 150 and seen[1][1].cfg.max_batch == 64
    assert seen[5][1].blob.ctypes.data == blob_ptr and seen[1][1].blob.ctypes.data == blob_ptr
    # the learning rates and the freeze flag, as the library found them on entry
    lr = slice(N.SC_LR_LIK, N.SC_LR_LIK + 4)
    for k in range(1, 10):
        want = life.LR * (0.5 if k >= 6 else 1.0)
        assert seen[k][0][lr].tolist() == [float(np.float32(want))] * 4, k
        assert float(seen[k][0][N.SC_FREEZE_DEC]) == (1.0 if k >= 6 else 0.0), k
    assert s64.lr == [life.LR * 0.5] * 4 and s64.freeze_decoder and not s0.freeze_decoder

    # close(): no context left; the next call makes a new one for its own batch, on the same blob
    m.close()
    assert m._ctx is None and m._ctx_batch == 0 and len(fake.ctxs) == 0 and m.route() == "unsized"
    y, u, eps = life.inputs(fam)[2]
    now["k"] = 10
    m.filter_sequence(y, u, None, eps=eps, **life.INFER)
    assert m._ctx is not None and m._ctx_batch == 37 and len(fake.ctxs) == 1
    assert seen[10][1] is not seen[9][1] and seen[10][1].blob.ctypes.data == blob_ptr


@pytest.mark.parametrize("fam", list(life.FAMILIES))
def test_script_keeps_the_gpu_test_honest(fam):
    """On the oracle alone, from the real initial state (`make_model` on the CPU, `load_oracle_state`): the fp32 oracle -- the
    reference's own arithmetic -- stays within the GPU test's fixed tolerances for posterior and losses over the whole script, so a
    correct fp32 device can; the script really trains (the RLS weights grow to >= 0.1, the recognition weights move by > 1e-4:
    a comparison of tensors that never left their initial value would be vacuous); the sample counters advance as the
    running-variance recurrence says."""
    import vjf_amd
    m = life.make_model(vjf_amd, fam)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr = life.reference(fam, m)
    for k, (r64, r32) in enumerate(zip(tr.refs64, tr.refs32), 1):
        np.testing.assert_allclose(r32[0], r64[0], err_msg=f"call {k} mean", **life.POST)
        np.testing.assert_allclose(r32[1], r64[1], err_msg=f"call {k} logvar", **life.POST)
        np.testing.assert_allclose(r32[2], r64[2], err_msg=f"call {k} losses", **life.LOSS)
    assert np.abs(tr.s64.w_mean).max() >= 0.1
    assert np.abs(tr.s64.mean_W - tr.s0.mean_W).max() > 1e-4
    assert (tr.s64.n_lik, tr.s64.n_tr) == life.expected_counters(fam)
    assert tr.s0.n_lik == 0 and tr.s0.n_tr == 0 and tr.s64.n_tr > 0
    # the frozen decoder: unchanged from call 6 on is not observable here, but the flag and the rates reached both oracles
    assert tr.s64.freeze_decoder and tr.s32.freeze_decoder and tr.s64.lr == [life.LR * 0.5] * 4
    # every RLS tensor of the fp32 oracle is finite (an RLS update that broke down would make the yardstick meaningless)
    for nm in ("w_mean", "w_chol", "w_precision", "w_pchol"):
        assert np.isfinite(getattr(tr.s32, nm)).all(), nm
