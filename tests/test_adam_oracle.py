"""The grid Adam step (csrc/adam.hip) against adam_cases.step32 bit for bit -- and through it (test_adam_host.py, no GPU)
against float64 -- at its edge values, in every form of the step and on the trips of its loops that nothing else runs.

Tried against three wrong adam_one builds (MI355X): `+ eps` moved inside the division by bc2_sqrt, contract(off)
dropped, sqrtf replaced by __builtin_amdgcn_sqrtf.  Each fails test_every_form_gives_step32_bits (first assertion: the
bits of p against step32, in check_step), test_device_table_rows (the same assertion), both second-trip tests (the bits
of p against step32) -- the eps build in 13 of the 20 hyper x step cases of a form (where bc2_sqrt = 1 the two agree),
the contracting build in 16 (all but the four of the beta1 = 0 set), the approximate square root in 19.
test_nan_guard_on_edge_state does not and cannot fail under them: a guarded step runs none of adam_one."""
import functools

import numpy as np
import pytest
import torch

import adam_cases as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORMS = ("dense", "dense_views", "dense_param_view", "scan", "touched", "mixed")
CANARY = np.float32(-1234.5)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def view_of(a):
    """``a`` on the device as the [1:-1] view of a storage two floats longer: four bytes past a 16-byte boundary, a
    canary float in front of it and one behind.  -> (view, storage)"""
    st = torch.full((a.size + 2,), float(CANARY), device=DEV)
    assert st.data_ptr() % 16 == 0
    st[1:-1].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return st[1:-1], st


@functools.lru_cache(maxsize=None)
def _layout(n, rot, dense):
    return A.layout(n, rot, dense)


@functools.lru_cache(maxsize=None)
def _expected(n, rot, dense, hyper, step):
    L = _layout(n, rot, dense)
    sc = A.scalars_of(*hyper, step)
    return L.expect(sc, dense), L.bound(sc)


class State:
    """One layout's arrays on the device, in the shape a form wants them."""

    def __init__(self, L, views=()):
        self.L = L
        self.storage = {}
        for k in "pgmv":
            if k in views:
                t, self.storage[k] = view_of(getattr(L, k))
            else:
                t = dev(getattr(L, k))
                assert t.data_ptr() % 16 == 0
            setattr(self, k, t)
        self.active = dev(L.active)
        self.touched = dev(L.nonzero.astype(np.uint8))

    def row(self, zero, touched):
        return (self.p, self.g, self.m, self.v, self.active, zero) + ((self.touched,) if touched else ())


def run_form(form, rot, zero, when, guard=None):
    """One step of ``form`` over the layout(s) of rotation ``rot`` -> [(State, dense?, touched?)].  when: the five
    arguments (step, lr, beta1, beta2, eps) or an AdamWhen."""
    from miso_amd import ops
    if form.startswith("dense"):
        views = {"dense": "", "dense_views": "pgmv", "dense_param_view": "p"}[form]
        s = State(_layout(A.N_DENSE, rot, True), views)
        assert guard is None
        ops.adam_dense_(s.p, s.g, s.m, s.v, *when, zero_grad=zero)
        return [(s, True, False)]
    if form == "mixed":                        # one block, one launch: a tensor by its gradient and one by its flags
        a, b = State(_layout(A.N_ACTIVE, rot, False)), State(_layout(A.N_ACTIVE, rot + 5, False))
        rows = [a.row(zero, False), b.row(not zero, True)]
        out = [(a, False, False, zero), (b, False, True, not zero)]
    else:
        a = State(_layout(A.N_ACTIVE, rot, False))
        rows = [a.row(zero, form == "touched")]
        out = [(a, False, form == "touched", zero)]
    ops.adam_step_(ops.adam_tensors(rows), ops.adam_when(*when) if isinstance(when, tuple) else when, guard)
    return out


def _zero_of(entry, zero):
    return entry[3] if len(entry) > 3 else zero


def check_step(entry, zero, hyper, step, what):
    """The arrays of one stepped State against step32 (bits, NaN by class), step64's bound, and the flag rules."""
    s, dense, touched = entry[:3]
    zero = _zero_of(entry, zero)
    L = s.L
    want, (val, err, ok) = _expected(L.n, L.rot, dense, hyper, step)
    for name, t, w, v64, e in zip("pmv", (s.p, s.m, s.v), want, val, err):
        got = host(t)
        same = A.same_by_class(got, w)
        bad = np.flatnonzero(~same)
        assert bad.size == 0, (what, name, L.rot, bad[:4], got[bad[:4]], w[bad[:4]],
                               L.p[bad[:4]], L.g[bad[:4]], L.m[bad[:4]], L.v[bad[:4]])
        moved = ok if dense else ok & L.stepped_el
        assert (np.abs(got[moved].astype(np.float64) - v64[moved]) <= e[moved]).all(), (what, name, "float64 bound")
    g = A.bits(host(s.g))
    cleared = np.ones(L.n, dtype=bool) if dense else L.stepped_el
    if zero:
        assert (g[cleared] == 0).all(), (what, "a stepped chunk's gradient is not +0")
        assert np.array_equal(g[~cleared], A.bits(L.g)[~cleared]), (what, "a sleeping chunk's gradient changed")
    else:
        assert np.array_equal(g, A.bits(L.g)), (what, "gradient changed without zero_grad")
    if not dense:
        assert np.array_equal(host(s.active), L.stepped.astype(np.uint8)), (what, "active")
        assert int(host(s.touched).sum()) == (0 if touched else int(L.nonzero.sum())), (what, "touched")
    for k, st in s.storage.items():
        ends = host(st[[0, -1]])
        assert np.array_equal(A.bits(ends), A.bits(np.array([CANARY, CANARY]))), (what, k, "canary", ends)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("step", [1, 2, 1000, 1000000])
@pytest.mark.parametrize("hyper", A.HYPERS, ids=lambda h: "lr%g-b%g-%g-eps%g" % h)
def test_every_form_gives_step32_bits(hyper, step, form):
    """One step from the planted state over the form's layouts of EDGE (every rotation, with and without zero_grad):
    p, m, v equal step32 bit for bit -- a NaN for a NaN, the same infinity, bits elsewhere -- and lie within step64's
    bound wherever the step stays finite; `active` = the chunk holds a gradient whose bits are not +-0, or was active; a
    chunk woken by ONE subnormal gradient steps, a chunk whose only gradient is -0 sleeps with its bits unchanged; with
    zero_grad the gradient is +0 in every stepped chunk and untouched elsewhere; `touched` ends cleared; the unaligned
    dense form leaves the float in front of and behind every array alone."""
    for rot in range(A.N_ROT):
        for zero in (False, True):
            for entry in run_form(form, rot, zero, (step,) + hyper):
                check_step(entry, zero, hyper, step, (form, rot, zero))


@pytest.mark.parametrize("hyper", [A.HYPERS[0], A.HYPERS[2]], ids=["default", "beta1-0"])
def test_device_table_rows(hyper):
    """Scalars from the device table (AdamDeviceStep.when) in every form of miso_adam_step: the count set to 0,
    rows - 1 and rows + 5, then bumped, gives the bits of the host-scalar step -- and of step32 -- at numbers 1, rows and
    rows + 6; the last is the clamp min(step, table_len) together with the rule that the table ends on the constant
    row.  A count of -3 under a NaN guard is not bumped, and the launch, clamped to row 0, changes nothing."""
    from miso_amd import ops
    ds = ops.AdamDeviceStep(*hyper, DEV)
    rows = ds.rows
    assert rows == ops.adam_table_rows(hyper[1], hyper[2]) and tuple(ds.table.shape) == (rows, 6)
    fine = torch.tensor([0.5], device=DEV)
    for count, number in ((0, 1), (rows - 1, rows), (rows + 5, rows + 6)):
        for i, form in enumerate(("scan", "touched", "mixed")):
            ds.set_count(count)
            ds.bump(fine if i else None)
            assert int(ds.step[0]) == count + 1
            rot, zero = 3 * i + count % 5, bool(i % 2)
            got = run_form(form, rot, zero, ds.when, fine)
            ref = run_form(form, rot, zero, (number,) + hyper)
            for a, b in zip(got, ref):
                check_step(a, zero, hyper, number, ("table", form, count))
                for k in ("p", "g", "m", "v", "active", "touched"):
                    x, y = getattr(a[0], k), getattr(b[0], k)
                    assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                       y.view(torch.int32) if y.dtype == torch.float32 else y), (form, count, k)
    nan = torch.tensor([float("nan")], device=DEV)
    for form in ("scan", "touched", "mixed"):
        ds.set_count(-3)
        ds.bump(nan)
        assert int(ds.step[0]) == -3
        for entry in run_form(form, 1, True, ds.when, nan):
            check_guarded(entry, True, ("table", form))


def check_guarded(entry, zero, what):
    """A step under a NaN guard: p, m, v, active keep their bits; zero_grad clears the chunks that hold a non-zero
    gradient (+0 exactly), leaves the chunks that were never stepped alone, and whatever it does to the others (stepped
    before, gradients +-0) leaves them zero."""
    s, dense, touched = entry[:3]
    zero = _zero_of(entry, zero)
    L = s.L
    for k in "pmv":
        assert np.array_equal(A.bits(host(getattr(s, k))), A.bits(getattr(L, k))), (what, k)
    assert np.array_equal(host(s.active), L.active), (what, "active")
    g = host(s.g)
    if zero:
        assert (A.bits(g)[L.nonzero_el] == 0).all(), (what, "consumed gradients not cleared")
        asleep = ~L.stepped_el
        assert np.array_equal(A.bits(g)[asleep], A.bits(L.g)[asleep]), (what, "sleeping chunk")
        assert (g[~L.nonzero_el] == 0).all()
    else:
        assert np.array_equal(A.bits(g), A.bits(L.g)), (what, "gradient")
    if touched:
        assert int(host(s.touched).sum()) == 0, (what, "touched")


@pytest.mark.parametrize("form", ["scan", "touched", "mixed"])
def test_nan_guard_on_edge_state(form):
    """With a NaN guard every guarded form (the dense entry takes no guard) leaves p, m, v and `active` bit-identical
    on the EDGE layouts, NaN and inf gradients included, and zero_grad still clears exactly the chunks that hold a
    non-zero gradient."""
    nan = torch.tensor([float("nan")], device=DEV)
    for rot in range(A.N_ROT):
        for zero in (False, True):
            for entry in run_form(form, rot, zero, (7,) + A.HYPERS[rot % len(A.HYPERS)], nan):
                check_guarded(entry, zero, (form, rot, zero))


def _tile_edge(arrs, start, count):
    idx = np.arange(count) % A.EDGE.size
    for k, a in zip("pgmv", arrs):
        a[start:start + count] = A.EDGE[k][idx]


def test_dense_grid_stride_second_trip():
    """adam_kernel's grid-stride loop takes a second trip above 4 096 x 256 float4s: n = 4 x 1 048 576 + 4 x 300 + 3.
    EDGE at the start, across the 4 194 304 boundary (where the second trip begins) and in the tail, randn x 1e-2
    elsewhere; every element has step32's bits and the gradient is cleared."""
    from miso_amd import ops
    n = 4 * 1048576 + 4 * 300 + 3
    rng = np.random.default_rng(5)
    p, g = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32) * np.float32(1e-2)
    m = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-2)
    v = np.square(rng.standard_normal(n, dtype=np.float32) * np.float32(1e-2))
    E = A.EDGE.size
    for start, count in ((0, 2 * E), (4 * 1048576 - E, 2 * E), (n - E - 3, E + 3)):
        _tile_edge((p, g, m, v), start, count)
    hyper, step = A.HYPERS[0], 3
    want = A.step32(p, g, m, v, A.scalars_of(*hyper, step))
    dp, dg, dm, dv = dev(p), dev(g), dev(m), dev(v)
    ops.adam_dense_(dp, dg, dm, dv, step, *hyper, zero_grad=True)
    for name, t, w in zip("pmv", (dp, dm, dv), want):
        bad = np.flatnonzero(~A.same_by_class(host(t), w))
        assert bad.size == 0, (name, bad[:8], bad.size)
    assert int(dg.view(torch.int32).count_nonzero()) == 0


def test_gradient_scan_second_trip():
    """adam_active_body's slab loop takes a second trip above 4 096 x 4 x 4 slabs: n = 16 777 216 + 256 x 5 + 64 x 2 + 7
    by gradient, 67 MB an array.  One chunk in sixteen holds a gradient, and so do the chunk behind the boundary and
    those of the ragged end; two steps, the second with other chunks and zero_grad.  Everything equals adam_dense_ on a
    copy bit for bit (moments start at zero, where a dense step of a sleeping chunk changes nothing); on the host only
    the slices around the boundary and at the end are compared with step32: the full-length numpy reference takes
    seconds."""
    from miso_amd import ops
    n0 = 16777216
    n = n0 + A.N_ACTIVE
    nch = (n + A.CHUNK - 1) // A.CHUNK
    gen = torch.Generator(device=DEV).manual_seed(11)
    p0 = torch.randn(n, device=DEV, generator=gen)
    c = torch.arange(nch, device=DEV)
    first = n0 // A.CHUNK
    wakes = []
    for lanes, extra in (((15,), (first, nch - 2, nch - 1)), ((15, 3), (first + 1, nch - 3))):
        on = torch.zeros(nch, dtype=torch.bool, device=DEV)
        for r in lanes:
            on |= c % 16 == r
        on[list(extra)] = True
        wakes.append(on)
    assert bool(wakes[0][first - 1]) and bool(wakes[0][first]) and bool(wakes[0][nch - 1])
    grads = [torch.randn(n, device=DEV, generator=gen) * 1e-2 * on.repeat_interleave(A.CHUNK)[:n] for on in wakes]
    hyper = A.HYPERS[0]
    slices = (slice(n0 - 320, n0 + 576), slice(n - A.N_ACTIVE + 1024, n))
    res = {}
    for kind in ("dense", "scan"):
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        act = ops.adam_active_flags(p)
        for t, gr in enumerate(grads):
            g = gr.clone()
            if kind == "dense":
                ops.adam_dense_(p, g, m, v, t + 1, *hyper, zero_grad=t == 1)
            else:
                ops.adam_active_(p, g, m, v, act, t + 1, *hyper, zero_grad=t == 1)
        res[kind] = (p, m, v, g, act)
    for k, a, b in zip("pmv", res["dense"], res["scan"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    p, m, v, g, act = res["scan"]
    assert torch.equal(act.bool(), wakes[0] | wakes[1])
    woken = (wakes[0] | wakes[1]).repeat_interleave(A.CHUNK)[:n]
    assert int(g[woken].view(torch.int32).count_nonzero()) == 0 and torch.equal(g[~woken], grads[1][~woken])
    for sl in slices:
        hp, hm, hv = host(p0[sl]), np.zeros(sl.stop - sl.start, np.float32), np.zeros(sl.stop - sl.start, np.float32)
        for t, gr in enumerate(grads):
            hp, hm, hv = A.step32(hp, host(gr[sl]), hm, hv, A.scalars_of(*hyper, t + 1))
        for name, got, want in zip("pmv", (p, m, v), (hp, hm, hv)):
            assert np.array_equal(A.bits(host(got[sl])), A.bits(want)), (name, sl)
