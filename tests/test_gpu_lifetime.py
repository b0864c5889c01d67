"""One native context across its life (tests/lifetime.py): batch size, flags, entry point and route changing from call to call, as
`fit()` and an online filter use it.  Everything the library carries from one call to the next -- the workspace sized by `max_batch`,
the two alternating counter blocks of the one-launch route, the parameter image and the transposed copies, SC_TRI_CLEAN, the epoch
and hand-off counts, the lazily created extra streams -- is exercised by nine calls on one model:

  (a) against the fp64 oracle carried through the whole script, at the tolerances of the single-call parity tests;
  (b) history must not matter: a twin that gets a FRESH context and workspace before every call computes the same bits;
  (c) `max_batch` must not matter: a context for 600 trials computes the same bits as one for the 37 it serves;
  (d) the overlap setting (route) switched before every call, one call on a side stream, against the oracle;
  (e) a batch beyond `max_batch` through the C ABI is refused and leaves the context as it was.

All tests need a real MI355X:  pytest -m gpu."""
import ctypes

import pytest
import torch

from tests import lifetime as life

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vjf():
    import vjf_amd
    assert torch.cuda.is_available()
    return vjf_amd


def _same_bits(what, k, live, twin, a, b):
    for name, x, y in zip(("mean", "logvar", "losses"), a, b):
        assert torch.equal(x, y), f"{what}: call {k}: {name} differs by {float((x.double() - y.double()).abs().max()):.3e}"
    assert torch.equal(live._blob, twin._blob), f"{what}: state after call {k}: {life.blob_diff(live, twin)}"


# ------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fam", list(life.FAMILIES))
def test_life_against_the_oracle(vjf, fam):
    """Every call's posterior and loss rows (rtol = atol = 2e-6 / 2e-5, test_filter_vs_oracle's) and a clean status word; after the
    last call the whole state (non-RLS tensors rtol 1e-5, atol 1e-6; the RLS tensors at 5e-3 / 5e-5 or, noted, within 3 x the fp32
    oracle's own distance from fp64) and the two sample counters exactly."""
    m = life.make_model(vjf, fam)
    tr = life.reference(fam, m)
    for step, ref in zip(life.drive(fam, m), tr.refs64):
        life.compare_outputs(f"life[{fam}]", step, ref)
        assert m.check_status() == 0, f"call {step.k}"
    notes = life.compare_state(f"life[{fam}]", m, tr.s64, tr.s32)
    for n in notes:
        print("note:", n)


# ------------------------------------------------------------------ (b)
@pytest.mark.parametrize("fam", list(life.FAMILIES))
def test_history_does_not_matter(vjf, fam):
    """A twin follows the script from the same initial state, but before every call its context is destroyed and created anew (a
    fresh workspace, fresh counters and streams, the same `max_batch` as the live one has by then): all three outputs of every call
    and the state blob after it are bit-identical, and both report the same route -- for the one-launch families "one-launch" on
    every call but 8 (an RLS update without SGD is served per step)."""
    live, twin = life.make_model(vjf, fam), life.make_model(vjf, fam)
    assert torch.equal(live._blob, twin._blob)

    def fresh(k, call, B):
        torch.cuda.synchronize()
        twin.close()
        twin._ensure_ctx(max(live._ctx_batch, B))

    for a, b in zip(life.drive(fam, live), life.drive(fam, twin, pre=fresh)):
        assert live._ctx_batch == twin._ctx_batch
        _same_bits(f"history[{fam}]", a.k, live, twin, a.out, b.out)
        assert live.check_status() == 0 and twin.check_status() == 0, f"call {a.k}"
        route = live.route(**a.call.flags)
        assert route == twin.route(**a.call.flags), f"call {a.k}"
        if fam in ("mega", "mega_p"):
            assert route == ("per-step" if a.k == 8 else "one-launch"), f"call {a.k}: {route}"


# ------------------------------------------------------------------ (c)
@pytest.mark.parametrize("fam", ["mega", "rlsb", "wide"])
def test_max_batch_does_not_matter(vjf, fam):
    """Two fresh models; one gets a context for 600 trials first (the Gram slabs, the E / ACT / DEL rows, the partials are carved
    for 600, and split_for(600) != split_for(37)).  Both run a training sequence of 3 steps on 37 trials from the prior: same bits."""
    f = life.FAMILIES[fam]
    a, b = life.make_model(vjf, fam), life.make_model(vjf, fam)
    b._ensure_ctx(600)
    g = torch.Generator().manual_seed(life.DATA_SEED + 1)
    T, B = 3, 37
    y = torch.randn(T, B, f["dy"], generator=g)
    u = torch.randn(T, B, f["du"], generator=g) if f["du"] else None
    eps = torch.randn(T, 2, B, f["dz"], generator=g)
    oa = a.filter_sequence(y, u, None, eps=eps, **life.TR)
    ob = b.filter_sequence(y, u, None, eps=eps, **life.TR)
    assert (a._ctx_batch, b._ctx_batch) == (37, 600)
    _same_bits(f"max_batch[{fam}]", 1, a, b, oa, ob)
    assert a.check_status() == 0 and b.check_status() == 0
    assert a.route() == b.route()


# ------------------------------------------------------------------ (d)
@pytest.mark.parametrize("fam", ["mega", "rlsb"])
def test_routes_switched_on_a_live_context(vjf, fam):
    """Before call k the overlap setting changes ([1, 0, 3][k % 3] on the one-launch family: one-launch, one-stream order, three
    streams; [1, 0][k % 2] on the multi-launch RLS family: two-stream, one-stream order), and call 4 runs under a side stream
    (`vjf_set_stream` on a context that owns internal streams and events by then).  Compared with the oracle exactly as in (a) -- no
    bitwise claim, the routes differ by summation order.  After every call `route()` is what `vjf_route` reports for the setting
    `vjf_set_overlap` returned, and what the route table says for it."""
    from vjf_amd import _native as N
    cycle = [1, 0, 3] if fam == "mega" else [1, 0]
    m = life.make_model(vjf, fam)
    tr = life.reference(fam, m)
    side = torch.cuda.Stream()

    def pre(k, call, B):
        m.set_overlap(cycle[k % len(cycle)])

    def around(k, thunk):
        if k != 4:
            return thunk()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            out = thunk()
        torch.cuda.synchronize()
        return out

    L = N.lib()
    for step, ref in zip(life.drive(fam, m, pre=pre, around=around), tr.refs64):
        k, want = step.k, cycle[step.k % len(cycle)]
        life.compare_outputs(f"routes[{fam}]", step, ref)
        assert m.check_status() == 0, f"call {k}"
        setting = L.vjf_set_overlap(m._ctx, want)                       # (again: it returns the resulting setting)
        assert setting == want, f"call {k}"
        code = L.vjf_route(m._ctx, life.flag_bits(step.call.flags))
        assert code >= 0
        route = m.route(**step.call.flags)
        assert route == life.ROUTE_NAME[code], f"call {k}"
        assert route == life.expected_route(fam, setting, step.call.flags), f"call {k}: setting {setting}, {step.call.flags}: {route}"
    notes = life.compare_state(f"routes[{fam}]", m, tr.s64, tr.s32)
    for n in notes:
        print("note:", n)


# ------------------------------------------------------------------ (e)
def test_batch_beyond_max_batch_is_refused_and_harmless(vjf):
    """`vjf_filter_step` with B = 65 (and buffers of 65 rows) on a context of max_batch = 64: a negative return whose message names
    max_batch, nothing launched -- the blob bit-identical, the output buffers untouched, the status word 0 -- and the next ordinary
    call of the context matches a twin that never made the bad call."""
    from vjf_amd import _native as N
    fam = "mega"
    f = life.FAMILIES[fam]
    m, twin = life.make_model(vjf, fam), life.make_model(vjf, fam)
    (y1, u1, e1), (y2, u2, e2) = life.inputs(fam)[:2]
    for mod in (m, twin):
        mod.filter_sequence(y1, u1, None, eps=e1, **life.WARM)
    assert m._ctx_batch == 64 and m.check_status() == 0
    B, dev = 65, m._blob.device
    g = torch.Generator().manual_seed(life.DATA_SEED + 2)
    y, u = torch.randn(B, f["dy"], generator=g).to(dev), torch.randn(B, f["du"], generator=g).to(dev)
    es, et = torch.randn(B, f["dz"], generator=g).to(dev), torch.randn(B, f["dz"], generator=g).to(dev)
    mu, lv, loss4 = torch.full((B, f["dz"]), 7.0, device=dev), torch.full((B, f["dz"]), 7.0, device=dev), torch.full((4,), 7.0, device=dev)
    before = m._blob.clone()
    torch.cuda.synchronize()
    L = N.lib()
    rc = L.vjf_filter_step(m._ctx, B, N.ptr(y), N.ptr(u), None, None, N.ptr(es), N.ptr(et), N.ptr(mu), N.ptr(lv), N.ptr(loss4),
                           N.FLAG_SGD | N.FLAG_UPDATE)
    assert rc < 0 and b"max_batch" in L.vjf_last_error(), (rc, L.vjf_last_error())
    # (the sequence entry point checks the same bound: one step of the same buffers, the two draws side by side)
    eps = torch.stack([es, et])[None].contiguous()
    rc = L.vjf_filter_seq(m._ctx, 1, B, N.ptr(y), N.ptr(u), N.ptr(eps), None, None, N.ptr(mu), N.ptr(lv), N.ptr(loss4),
                          N.FLAG_SGD | N.FLAG_UPDATE)
    assert rc < 0 and b"max_batch" in L.vjf_last_error(), (rc, L.vjf_last_error())
    torch.cuda.synchronize()
    assert torch.equal(m._blob, before)
    assert bool((mu == 7.0).all()) and bool((lv == 7.0).all()) and bool((loss4 == 7.0).all())
    s = ctypes.c_uint32(99)
    assert L.vjf_get_status(m._ctx, ctypes.byref(s)) == 0 and s.value == 0
    oa = m.filter_sequence(y2, u2, None, eps=e2, **life.TR)
    ob = twin.filter_sequence(y2, u2, None, eps=e2, **life.TR)
    _same_bits("abi bound", 2, m, twin, oa, ob)
    assert m.check_status() == 0 and twin.check_status() == 0 and m.route() == "one-launch"
