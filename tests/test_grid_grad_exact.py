"""The grid gradient, bit for bit, at every vertex, on every path that forms it.

tests/grid_grad_cases.py builds batches on which every weight, every product and every partial sum of the gradient is
representable in fp32 whatever the order (dyadic coordinates, cotangents m 2**e, a 24-bit window per vertex that the
helper asserts).  The float64 numpy scatter there is then THE answer: the atomic scatters, the vector pulls with and
without their slice queue, the matrix-core pull with its epochs, the matrix-core push and the scatters inside the fused
backward and training kernels must reproduce it as int32 bit patterns (-0 == +0), including exact zeros at the vertices
no sample touches, samples that sit on cell / tile / brick faces and on the faces of the bound, and vertices whose
gradient is seven decades below the level's largest entry -- none of which a max-norm comparison can see.
"""
import dataclasses

import numpy as np
import pytest
import torch

import grid_grad_cases as gc
from oracle import ref_torch as R

DEV = "cuda:0"
CASES = ["A", "B", "C", "D", "E"]
CLUSTERED = [n for n in CASES if gc.SPECS[n]["cluster"]]


def _features(case, dtype):
    return [torch.zeros(1, case.C, *lv, dtype=dtype, requires_grad=True) for lv in case.levels]


def _autograd_grads(case, dtype):
    feats = _features(case, dtype)
    out = R.encode_stock(feats, torch.tensor(case.bound, dtype=dtype), torch.tensor(case.x).to(dtype))
    return torch.autograd.grad(out, feats, torch.tensor(case.dfeat).to(dtype))


def _same_bits(got32: np.ndarray, want32: np.ndarray) -> np.ndarray:
    return (got32.view(np.int32) == want32.view(np.int32)) | ((got32 == 0) & (want32 == 0))


# --------------------------------------------------------------------------- #
# CPU: the premise
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", CASES)
def test_numpy_reference_equals_float64_autograd_and_the_fp32_oracle(name):
    """Three independent evaluations -- the numpy scatter, float64 autograd through the oracle's encode, and the same in
    fp32 (ATen's own summation order) -- agree exactly: the inputs leave no room for rounding."""
    case = gc.case(name)
    g64 = _autograd_grads(case, torch.float64)
    g32 = _autograd_grads(case, torch.float32)
    for l, r in enumerate(case.ref):
        assert np.array_equal(g64[l][0].numpy(), r.G), (name, l)
        want = r.G.astype(np.float32)
        assert np.array_equal(want.astype(np.float64), r.G), (name, l)        # G itself is an fp32 number everywhere
        assert _same_bits(g32[l][0].numpy(), want).all(), (name, l)


@pytest.mark.parametrize("name", CASES + ["F"])
def test_budget_holds_with_and_without_prefill(name):
    case = gc.case(name)
    bits = gc.assert_budget(case.ref)
    pre = gc.assert_budget(case.ref, [gc.prefill_pattern(r.G.shape, 900 + l) for l, r in enumerate(case.ref)])
    print(f"case {name}: {bits:.1f} bits, prefilled {pre:.1f}")
    assert bits <= 24.0 and pre <= 24.0


def test_budget_assertion_refuses_an_inexact_case():
    """A later edit of the inputs cannot quietly turn the exact tests into lucky ones: non-dyadic cotangents are refused."""
    case = gc.case("C")
    d = case.dfeat * np.float32(1.0 / 3.0)
    with pytest.raises(AssertionError, match="depend on their order"):
        gc.assert_budget(gc.reference(case.levels, case.C, case.bound, case.x, d))


@pytest.mark.parametrize("name", CASES)
def test_cases_have_the_properties_the_exact_tests_exist_for(name):
    case = gc.case(name)
    for l, r in enumerate(case.ref):
        # (the coarsest level of a case has fewer vertices than the batch has samples: every one of them is reached)
        if l > 0:
            assert (r.M == 0).any(), (name, l)
        assert np.array_equal(r.G[:, r.M == 0], np.zeros_like(r.G[:, r.M == 0]))
    if name in CLUSTERED:
        assert case.ref[0].M.max() >= 1000, (name, int(case.ref[0].M.max()))
    mags = np.concatenate([np.abs(r.G[r.G != 0]) for r in case.ref])
    assert mags.max() / mags.min() >= 1e6, (name, mags.max(), mags.min())
    # pinned rows: on the bound's corners and faces, and three that must contribute nothing
    p = case.n - gc.PINNED
    assert np.isnan(case.x[p + 4]).all() and np.isinf(case.x[p + 5]).all() and (case.x[p + 6] == np.float32(1e30)).all()
    assert (case.dfeat[p + 4:, 0] != 0).all()
    lo, hi = np.array(case.bound)[:, 0], np.array(case.bound)[:, 1]
    assert np.array_equal(case.x[p], lo.astype(np.float32)) and np.array_equal(case.x[p + 1], hi.astype(np.float32))


# --------------------------------------------------------------------------- #
# GPU: d-feat rows handed in
# --------------------------------------------------------------------------- #
_DEVCACHE = {}


def _dev_case(name):
    """Device copies shared by the tests of a case: points, rows, the expected gradients, never written to."""
    if name not in _DEVCACHE:
        case = gc.case(name)
        want = [torch.from_numpy(r.G.astype(np.float32)).unsqueeze(0).to(DEV) for r in case.ref]
        _DEVCACHE[name] = dict(case=case, x=torch.tensor(case.x).to(DEV), d=torch.tensor(case.dfeat).to(DEV),
                               want=want, sorted={}, prefill=None)
    return _DEVCACHE[name]


def _sorted(name, tiles):
    from miso_amd import ops
    dc = _dev_case(name)
    if tiles not in dc["sorted"]:
        meta = ops.GridMeta.from_bound(dc["case"].bound)
        dc["sorted"][tiles] = ops.SortedBatch(dc["case"].n, DEV, tiles=tiles).sort(dc["x"], meta)
    return dc["sorted"][tiles]


def _prefill(name):
    """The accumulate-mode pattern per level and the expected prefill + G, budget asserted with the prefill's bits in."""
    dc = _dev_case(name)
    if dc["prefill"] is None:
        case = dc["case"]
        pre = [gc.prefill_pattern(r.G.shape, 900 + l) for l, r in enumerate(case.ref)]
        gc.assert_budget(case.ref, pre)
        tot = [(p.astype(np.float64) + r.G) for p, r in zip(pre, case.ref)]
        for t in tot:
            assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
        dc["prefill"] = ([torch.from_numpy(p).unsqueeze(0).to(DEV) for p in pre],
                         [torch.from_numpy(t.astype(np.float32)).unsqueeze(0).to(DEV) for t in tot])
    return dc["prefill"]


def _assert_exact(got, want, case, l, what):
    """got / want: (1,C,Z,Y,X) device tensors of any layout.  int32 patterns equal, -0 == +0."""
    same = (got.view(torch.int32) == want.view(torch.int32)) | ((got == 0) & (want == 0))
    if bool(same.all()):
        return
    bad = (~same).nonzero()
    _, c, z, y, x = (int(v) for v in bad[0])
    g, w = got[0, c, z, y, x], want[0, c, z, y, x]
    r = case.ref[l]
    raise AssertionError(
        f"{what}: level {l} {case.levels[l]}: {bad.shape[0]} of {same.numel()} entries differ; first at channel {c} vertex "
        f"(z,y,x)=({z},{y},{x}): got {g.item()!r} (0x{g.view(torch.int32).item() & 0xffffffff:08x}) want {w.item()!r} "
        f"(0x{w.view(torch.int32).item() & 0xffffffff:08x}); M={int(r.M[z, y, x])} S={r.S[c, z, y, x]!r} q={r.q[c, z, y, x]!r}")


def _layout(t, channels_last=True):
    return t.contiguous(memory_format=torch.channels_last_3d) if channels_last else t.contiguous()


def _grid(case, channels_last=True):
    return [_layout(torch.zeros(1, case.C, *lv, device=DEV), channels_last) for lv in case.levels]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["channels_last", "ncdhw", "sorted_batch", "no_lean"])
@pytest.mark.parametrize("name", CASES)
def test_atomic_scatter_is_exact(name, variant, monkeypatch):
    """miso_encode_bwd in both its forms (caller order, binned): float atomics in whatever order the hardware serves them.
    With a gradient buffer the launch is always the weight-form encode_bwd_kernel (launch_encode_bwd); MISO_ENCODE_NO_LEAN keeps
    grad_x in that kernel when it is asked for alone, so `no_lean` runs the scatter with grad_x formed beside it."""
    from miso_amd import ops
    dc = _dev_case(name)
    case = dc["case"]
    monkeypatch.setattr(ops, "ENCODE_PULL_MIN_POINTS", None)          # always atomics
    if variant == "no_lean":
        monkeypatch.setenv("MISO_ENCODE_NO_LEAN", "1")
    feats = _grid(case, channels_last=variant != "ncdhw")
    meta = ops.GridMeta.from_bound(case.bound)
    sb = _sorted(name, 16) if variant == "sorted_batch" else None
    _, grads = ops.encode_bwd_raw(dc["x"], feats, meta, dc["d"], variant == "no_lean", [True] * len(feats), sorted_batch=sb)
    for l, (g, w) in enumerate(zip(grads, dc["want"])):
        assert g.stride() == feats[l].stride()
        _assert_exact(g, w, case, l, f"atomic scatter ({variant}), case {name}")


# form -> (environment, cases).  (C is not for the matrix-core pull at 16 tiles: its level of 3 vertices on y has
# fewer than 2/3 of a vertex per tile, plan_grad's mc_reaches; as shipped it takes vector_drain's path.)  There is a query for the matrix-core pull (miso_grad_pull_on_matrix_cores) and for
# the levels a binning owns (miso_grad_pull_levels); between the vector kernels plan_grad decides by `block_ok`: an even
# cubic binning that divides every pulled level's size on every axis, at most three levels -> PULL_BLOCK (A, D: 16 | 16,
# 32, 64, 128), else PULL_WAVE (C: 16 divides none of 12, 20, 33, 3, 100).  MISO_MC_SMALL shrinks the matrix-core kernel's
# survivor table and pair pool at launch (launch_grad_pull_mc), so every block runs several epochs and halves ranges; the
# plan and its query do not change.  The slice queue: plan.drain = a queue is present and MISO_PULL_NO_SPLIT is not set;
# that slices were queued is read from the queue itself, which the library rewinds but does not clear.
PULL_FORMS = {
    "mc": (dict(), ["A", "B", "D", "E"]),
    "mc_small": (dict(MISO_MC_SMALL="1"), ["A", "B", "D", "E"]),
    "vector_drain": (dict(MISO_PULL_MC="0"), ["A", "D", "C"]),
    "vector_no_split": (dict(MISO_PULL_MC="0", MISO_PULL_NO_SPLIT="1"), ["A", "D", "C"]),
}
PULL_PARAMS = [(f, n) for f, (_, names) in PULL_FORMS.items() for n in names]
PITCH_PAD, PITCH_OFF = 8, 4


@pytest.mark.gpu
@pytest.mark.parametrize("cond", ["binned_rows", "caller_rows", "pitched_binned", "pitched_caller", "ignored_level"])
@pytest.mark.parametrize("overwrite", [True, False], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("form,name", PULL_PARAMS)
def test_pull_is_exact(form, name, overwrite, cond, monkeypatch):
    """ops.grad_pull_raw in every form plan_grad can choose, rows in binned or caller order, contiguous or as a 16-byte
    aligned view of a wider buffer (pitch F + 8, offset 4), one level ignored.  overwrite: the buffers hold NaN on entry
    and must hold exactly G afterwards -- exact zeros where no sample reaches (and all over an ignored level);
    accumulate: they hold 0.25 randint(-4, 4) and must hold exactly prefill + G (an ignored level: the prefill)."""
    from miso_amd import ops
    for k, v in PULL_FORMS[form][0].items():
        monkeypatch.setenv(k, v)
    tiles = gc.TILES_E if name == "E" else 16
    dc = _dev_case(name)
    case = dc["case"]
    L, F, n = len(case.levels), case.C * len(case.levels), case.n
    ignored = 1 if cond == "ignored_level" else None
    meta = ops.GridMeta.from_bound(case.bound, ignore_level=[l == ignored for l in range(L)])
    sb = _sorted(name, tiles)
    feats = _grid(case)
    pre, tot = _prefill(name)
    if overwrite:
        grads = [torch.full_like(f, float("nan")) for f in feats]
        want = [torch.zeros_like(w) if l == ignored else w for l, w in enumerate(dc["want"])]
    else:
        grads = [_layout(p.clone()) for p in pre]
        want = [pre[l] if l == ignored else t for l, t in enumerate(tot)]

    # which form runs, by the library's own account
    lib = ops._lib.load()
    gq = ops._fill_grid(feats, meta, grads, data=False)
    assert int(lib.miso_grad_pull_levels(ops.C.byref(gq), ops.pack_tiles(tiles))) == (1 << L) - 1
    caller = cond in ("caller_rows", "pitched_caller")
    rows = dc["d"] if caller else dc["d"][sb.perm.long()]
    if cond.startswith("pitched"):
        wide = torch.full((n, F + PITCH_PAD), float("nan"), device=DEV)
        wide[:, PITCH_OFF:PITCH_OFF + F] = rows
        rows = wide[:, PITCH_OFF:PITCH_OFF + F]
        assert rows.data_ptr() % 16 == 0 and rows.stride(0) == F + PITCH_PAD
    on_mc = int(lib.miso_grad_pull_on_matrix_cores(ops.C.byref(gq), ops.pack_tiles(tiles), n, rows.stride(0)))
    assert on_mc == (1 if form.startswith("mc") else 0)

    sb.pull_queue[4:].zero_()                                            # items of an earlier test (the header is 4 ints)
    ops.grad_pull_raw(feats, meta, sb, rows, grads, overwrite=overwrite, caller_order=caller)
    torch.cuda.synchronize()
    queued = int(sb.pull_queue[4:].abs().sum())
    assert int(sb.pull_queue[:4].abs().sum()) == 0                      # header rewound
    if form == "vector_drain" and name in CLUSTERED:
        assert queued > 0, "the cluster's tiles were to be cut into queued slices"
    if form != "vector_drain":
        assert queued == 0
    for l, (g, w) in enumerate(zip(grads, want)):
        _assert_exact(g, w, case, l, f"pull {form} {'overwrite' if overwrite else 'accumulate'} {cond}, case {name}")


# --------------------------------------------------------------------------- #
# GPU: the fused callers -- the d-feat rows come out of the decoder backward
# --------------------------------------------------------------------------- #
# An exact decoder: integer weights in {-1, 0, 1}, at most four non-zeros per row; b1 = 1 over grid values of order 1e-3
# and b2 above every row sum of |W2| keep every ReLU active at every sample, so the rows are g_i (W3 W2 W1): an integer
# vector times a dyadic scalar.  Each intermediate of the backward chain has at most eight significant bits -- one bf16
# piece in the split form, exact in the exact form.
FUSED = ["F", "G", "P"]
H = 64
TARGET = 1024.0      # |target|: far from any pred (|pred| <= 4 (b2 + row sum) < 40)
_FUSEDCACHE = {}


def _sparse_int(rs, rows, cols, nnz=4):
    w = np.zeros((rows, cols))
    for r in range(rows):
        idx = rs.choice(cols, size=min(nnz, cols), replace=False)
        w[r, idx] = rs.choice([-1.0, 1.0], size=idx.size)
    return w


def _fused_case(name):
    """Grid values, the exact decoder, d loss / d sdf with the regional scale and the sign an L1 loss against the far
    target gives, the expected rows and their float64 grid gradient (budget asserted)."""
    from miso_amd import ops
    if name in _FUSEDCACHE:
        return _FUSEDCACHE[name]
    dc = _dev_case(name)
    case = dc["case"]
    n, L, F = case.n, len(case.levels), case.C * len(case.levels)
    assert n & (n - 1) == 0, "the mean's 1/n must be a power of two"
    rs = np.random.RandomState(4000 + ord(name))
    W1, W2, W3 = _sparse_int(rs, H, F), _sparse_int(rs, H, H), _sparse_int(rs, 1, H)
    b1, b2, b3 = np.ones(H), np.abs(W2).sum(1) + 1.0, np.zeros(1)
    v = (W3 @ W2 @ W1).reshape(F)
    assert np.abs(W3 @ W2).max() < 256 and np.abs(v).max() < 256 and (v != 0).sum() >= F // 2
    tsign = rs.choice([-1.0, 1.0], size=n)                      # target = tsign * TARGET: pred - target has sign -tsign
    g = -tsign * case.scale                                     # d loss / d sdf of the backward tests; the training
    rows = g[:, None] * v[None, :]                              # kernels' is this / n
    ref = gc.reference(case.levels, case.C, case.bound, case.x, rows)
    gc.assert_budget(ref)
    dev = lambda a: torch.tensor(np.asarray(a, dtype=np.float32)).to(DEV)
    gen = torch.Generator().manual_seed(7)
    feats = [_layout((torch.randn(1, case.C, *lv, generator=gen) * 1e-3).to(DEV)) for lv in case.levels]
    pack = ops.DecoderPack([dev(W1), dev(W2), dev(W3)], [dev(b1), dev(b2), dev(b3)])
    aux = np.stack([tsign * TARGET, np.ones(n), np.zeros(n), case.scale], axis=1)      # {target, valid, sign, weight}
    fc = dict(case=case, dc=dc, feats=feats, pack=pack, v=v, g=dev(g).reshape(n, 1), rows=dev(rows), ref=ref,
              aux=dev(aux).contiguous(), tsign=tsign,
              want=[torch.tensor(r.G.astype(np.float32)).unsqueeze(0).to(DEV) for r in ref],
              want_mean=[torch.tensor((r.G / n).astype(np.float32)).unsqueeze(0).to(DEV) for r in ref])
    for r in ref:
        assert np.array_equal((r.G / n).astype(np.float32).astype(np.float64), r.G / n)
    _FUSEDCACHE[name] = fc
    return fc


def _check_grads(fc, grads, want, what):
    rc = dataclasses.replace(fc["case"], ref=fc["ref"])      # (_assert_exact reports M, S, q of the fused reference)
    for l, (g, w) in enumerate(zip(grads, want)):
        _assert_exact(g, w, rc, l, what)


def _meta(case, crowded=False):
    from miso_amd import ops
    return ops.GridMeta.from_bound(case.bound, flags=ops._lib.F_CROWDED if crowded else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact_fp32", "split_bf16"])
@pytest.mark.parametrize("name", FUSED)
def test_fused_rows_are_the_expected_rows_and_the_unsorted_scatter_is_exact(name, exact):
    """First the premise: miso_sdf_bwd_rows hands out exactly g_i (W3 W2 W1) -- if this fails the case is misbuilt and the
    decoder is not what is under test here.  Then the scatter inside sdf_bwd_kernel, in both of its forms (with the rows
    staged for the caller, and plain: ops.sdf_bwd_raw unsorted), adds those rows up to exactly the float64 gradient."""
    from miso_amd import ops
    fc = _fused_case(name)
    case, x, feats, pack = fc["case"], fc["dc"]["x"], fc["feats"], fc["pack"]
    meta = _meta(case)
    with ops.exact_fp32(exact):
        assert ops.sdf_fused_supported(feats, meta, pack)
        sdf, mask = ops.sdf_fwd_raw(x, feats, meta, pack, True)
        assert float(sdf.abs().max()) < 40.0
        _, grads, rows = ops.sdf_bwd_rows_raw(x, feats, meta, pack, fc["g"], mask, False, [True] * len(feats))
        assert bool((rows == fc["rows"]).all()), "misbuilt case: the decoder backward does not return g_i (W3 W2 W1)"
        _check_grads(fc, grads, fc["want"], f"sdf_bwd_rows scatter, case {name}")
        _, grads = ops.sdf_bwd_raw(x, feats, meta, pack, fc["g"], mask, False, [True] * len(feats))
        _check_grads(fc, grads, fc["want"], f"sdf_bwd unsorted scatter, case {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact_fp32", "split_bf16"])
@pytest.mark.parametrize("name,pulled,pushed", [("F", 0b111, 0), ("G", 0b01, 0), ("P", 0b11, 0b01)])
def test_sdf_bwd_sorted_is_exact(name, pulled, pushed, exact):
    """ops.sdf_bwd_raw over a batch binned at 16 tiles, overwrite mode over NaN: F -- every level through the matrix-core
    pull; G -- the coarse level pulled, the 144-wide one scattered by the kernel into the zero fill; P, with
    MISO_F_CROWDED -- the coarse level through grad_push_mfma_kernel, the fine one pulled."""
    from miso_amd import ops
    fc = _fused_case(name)
    case, x, feats, pack = fc["case"], fc["dc"]["x"], fc["feats"], fc["pack"]
    meta = _meta(case, crowded=pushed != 0)
    sb = _sorted(name, 16)
    grads = [torch.full_like(f, float("nan")) for f in feats]
    lib, grid = ops._lib.load(), ops._fill_grid(feats, meta, grads, data=False)
    assert int(lib.miso_grad_pull_levels(ops.C.byref(grid), 16)) == pulled
    assert int(lib.miso_sdf_bwd_push_levels(ops.C.byref(grid), 16, case.n)) == pushed
    assert ops.sdf_bwd_scattered_levels(feats, meta, grads, case.n) == (((1 << len(feats)) - 1) & ~pulled) | pushed
    with ops.exact_fp32(exact):
        _, mask = ops.sdf_fwd_raw(x, feats, meta, pack, True, sorted_batch=sb)
        ops.sdf_bwd_raw(x, feats, meta, pack, fc["g"], mask, False, [True] * len(feats), grads, sorted_batch=sb,
                        overwrite=True)
    _check_grads(fc, grads, fc["want"], f"sdf_bwd sorted, case {name}")


def _assert_loss_gradient_is_dyadic(fc, meta):
    """d loss / d sdf of the training kernels' L1 mean, through miso_mapping_loss_rows on the forward's own pred:
    exactly -sign(target) w_i / n."""
    from miso_amd import ops
    n = fc["case"].n
    sdf, _ = ops.sdf_fwd_raw(fc["dc"]["x"], fc["feats"], meta, fc["pack"], False)
    gp, loss = torch.empty(n, 1, device=DEV), torch.empty(2, device=DEV)
    ops.mapping_loss_rows_raw(sdf, fc["aux"], "L1", 1.0, 0.0, 0.0, gp, loss)
    assert bool((gp == fc["g"] / n).all()), "misbuilt case: d loss / d sdf is not -sign(target) w_i / n"


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact_fp32", "split_bf16"])
@pytest.mark.parametrize("name,scattered,pushed", [("F", 0, 0), ("G", 0b10, 0), ("P", 0, 0b01)])
def test_sdf_train_sorted_is_exact(name, scattered, pushed, exact):
    """ops.sdf_train_raw: forward, L1 loss and decoder backward in one launch, then the pull (F: all levels; G: the
    144-wide level is scattered from the training kernel itself; P, with MISO_F_CROWDED: the coarse level through the
    matrix-core push into the library's zero fill).  Overwrite semantics over NaN."""
    from miso_amd import ops
    fc = _fused_case(name)
    case, feats, pack = fc["case"], fc["feats"], fc["pack"]
    meta = _meta(case, crowded=pushed != 0)
    sb = _sorted(name, 16)
    grads = [torch.full_like(f, float("nan")) for f in feats]
    assert ops.sdf_train_supported(feats, meta, grads, pack)
    assert ops.sdf_train_scattered_levels(feats, meta, grads) == scattered
    grid = ops._fill_grid(feats, meta, grads, data=False)      # (the push rule is the same for the backward and the step)
    assert int(ops._lib.load().miso_sdf_bwd_push_levels(ops.C.byref(grid), 16, case.n)) == pushed
    slots = torch.zeros(ops._lib.LOSS_SLOTS, 2, device=DEV)
    with ops.exact_fp32(exact):
        _assert_loss_gradient_is_dyadic(fc, meta)
        ops.sdf_train_raw(feats, meta, pack, sb, fc["aux"], slots, grads, "L1", 1.0, 0.0, 0.0)
    _check_grads(fc, grads, fc["want_mean"], f"sdf_train sorted, case {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact_fp32", "split_bf16"])
@pytest.mark.parametrize("name", ["F", "G"])
def test_sdf_train_unsorted_is_exact(name, exact):
    """ops.sdf_train_unsorted_raw: one launch that scatters every level with float atomics, added to zeros."""
    from miso_amd import ops
    fc = _fused_case(name)
    case, feats, pack = fc["case"], fc["feats"], fc["pack"]
    meta = _meta(case)
    grads = [torch.zeros_like(f) for f in feats]
    slots = torch.zeros(ops._lib.LOSS_SLOTS, 2, device=DEV)
    with ops.exact_fp32(exact):
        _assert_loss_gradient_is_dyadic(fc, meta)
        ops.sdf_train_unsorted_raw(fc["dc"]["x"], feats, meta, pack, fc["aux"], slots, grads, "L1", 1.0, 0.0, 0.0)
    _check_grads(fc, grads, fc["want_mean"], f"sdf_train unsorted, case {name}")
