"""The mapping loss (map_loss_one, csrc/common.hpp) at its branch points, in every kernel that forms it: the float4 and
the scalar form of mapping_loss_kernel, mapping_loss_rows_kernel, sdf_fwd_kernel with the loss folded in and
sdf_train_kernel (binned and unbinned, 64- and 32-point trips) -- against loss_cases.loss_rule, a float64 restatement
whose branch decisions are single fp32 operations, pinned on the CPU to float64 autograd through grid_opt.loss.

Batches PLANT the rows that matter (d == 0 under L1, up == lo in the free-space maximum, valid / sign outside {0, 1}) and
every test asserts their counts.  Tolerances are rounding counts (loss_cases.gamma, term_bounds), none is a measurement:
on a dyadic lattice with a power-of-two n the gradients and the L1 sums are exact, and are compared bit for bit."""
import functools
import types

import numpy as np
import pytest
import torch

import loss_cases as lc
from loss_cases import F32, W_FS, W_SDF

gpu = pytest.mark.gpu
DEV = "cuda:0"

VEC_SIZES = [4, 252, 1024, 65536, 131080]      # n % 4 == 0: one float4 per array (131080: a third, partial pass of 64 blocks)
SCALAR_SIZES = [1, 3, 5, 255, 257, 1023, 16385, 40001]
ROWS_SIZES = [1, 255, 257, 1024, 16385, 40001]
COLS = ("pred", "target", "valid", "sign", "weight")


@functools.lru_cache(maxsize=None)
def _lattice(n, lt):
    return lc.lattice(n, lt)


@functools.lru_cache(maxsize=None)
def _random(n, lt):
    return lc.planted_random(n, lt)


def _pow2(n):
    return n & (n - 1) == 0


# ====================================================================================================================
# 1. the reference itself (no GPU)
# ====================================================================================================================
@pytest.mark.parametrize("lt", ["L1", "L2"])
def test_rule_equals_float64_autograd_through_grid_opt_loss(lt):
    """loss_rule == float64 autograd through miso_loss_regression + miso_loss_free_space (abs'(0) = 0, torch.maximum
    splits a tie evenly, relu'(0) = 0) on 4096 lattice rows that hold every branch class: difference 0.0, values and
    gradients (on the lattice every float64 sum is exact and 1/4096 is a power of two).  The CPU stand-in of the
    operator (oracle_backend.mapping_loss) agrees as well."""
    from miso_amd.grid_opt import loss as L
    import oracle_backend
    n = 4096
    b = _lattice(n, lt)
    lc.assert_planted(b)
    col = lambda k: torch.from_numpy(b[k].astype(np.float64)).reshape(n, 1)
    for drop in ((), ("valid",), ("weight",), ("valid", "weight")):
        a = {k: (None if k in drop else col(k)) for k in COLS}
        pred = col("pred").requires_grad_(True)
        t_sdf = W_SDF * L.miso_loss_regression(pred, a["target"], a["valid"], a["weight"], lt)
        t_fs = W_FS * L.miso_loss_free_space(pred, a["target"], a["sign"], b["trunc"])
        g_sdf, = torch.autograd.grad(t_sdf, pred)
        g_fs, = torch.autograd.grad(t_fs, pred)
        terms, r_sdf, r_fs = lc.loss_rule(b["pred"], b["target"], None if "valid" in drop else b["valid"], b["sign"],
                                          None if "weight" in drop else b["weight"], lt, W_SDF, W_FS, b["trunc"])
        assert terms[0] == t_sdf.item() and terms[1] == t_fs.item()
        assert np.array_equal(r_sdf, g_sdf.numpy().reshape(-1)) and np.array_equal(r_fs, g_fs.numpy().reshape(-1))
        assert np.abs(r_fs).max() > 0 and np.abs(r_sdf).max() > 0
        p2 = col("pred").requires_grad_(True)
        out = oracle_backend.mapping_loss(p2, a["target"], a["valid"], a["sign"], a["weight"], lt, W_SDF, W_FS, b["trunc"])
        assert out[0].item() == terms[0] and out[1].item() == terms[1]
        g2, = torch.autograd.grad(out.sum(), p2)
        assert np.array_equal(g2.numpy().reshape(-1), r_sdf + r_fs)
    # no free-space rows (sign None) and a padded batch's divisor
    terms, _, r_fs = lc.loss_rule(b["pred"], b["target"], b["valid"], None, b["weight"], lt, W_SDF, W_FS, b["trunc"])
    assert terms[1] == 0.0 and not r_fs.any()
    full = lc.loss_rule(b["pred"], b["target"], b["valid"], b["sign"], b["weight"], lt, W_SDF, W_FS, b["trunc"])
    half = lc.loss_rule(b["pred"], b["target"], b["valid"], b["sign"], b["weight"], lt, W_SDF, W_FS, b["trunc"], n_mean=n // 2)
    assert np.array_equal(half[0], 2 * full[0]) and np.array_equal(half[1], 2 * full[1])


def test_planted_batches_hold_their_classes():
    """Every size the GPU tests use: the lattice holds all seven classes, the off-lattice batch its d == 0 rows, its
    fp32 ties and the two one-ulp neighbours that break them."""
    for lt in ("L1", "L2"):
        for n in sorted(set(VEC_SIZES + SCALAR_SIZES + ROWS_SIZES)):
            lc.assert_planted(_lattice(n, lt))
            r = _random(n, lt)
            lc.assert_planted(r, classes=("d0", "tie_pos", "up_gt", "lo_gt"), odd=False)
    s = (0.3 * np.random.RandomState(5).standard_normal(4096)).astype(F32)
    t, t_up, t_down, kept, strict = lc.fs_ties(s, 0.15)
    assert kept[:1024].sum() >= 64 and strict.sum() >= 64
    one = np.ones(4096, dtype=F32)
    for tt, cls in ((t, "tie_pos"), (t_up, "lo_gt"), (t_down, "up_gt")):
        assert lc.classify(s, tt, one, one, 0.15)[cls][strict].all()


# ====================================================================================================================
# 2. the column kernel, both forms
# ====================================================================================================================
def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_cols(b, lt, want_fs_grad=True, w_fs=W_FS, drop=()):
    from miso_amd import ops
    n = len(b["pred"])
    a = {k: (None if k in drop else _dev(b[k])) for k in COLS}
    gp = torch.full((n,), 9.0, device=DEV)
    gfs = torch.full((n,), 9.0, device=DEV) if want_fs_grad else None
    loss = torch.full((2,), 9.0, device=DEV)
    ops.mapping_loss_raw(a["pred"], a["target"], a["valid"], a["sign"], a["weight"], lt, W_SDF, w_fs, b["trunc"],
                         grad_pred=gp, loss_out=loss, grad_pred_fs=gfs)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), gp.cpu().numpy(), None if gfs is None else gfs.cpu().numpy()


def _check_vs_rule(b, lt, out, K, B, on_lattice, w_fs=W_FS, drop=()):
    """One launch of a loss kernel over label columns against loss_rule."""
    loss, gp, gfs = out
    n = len(b["pred"])
    a = {k: (None if k in drop else b[k]) for k in COLS}
    terms, g, gf = lc.loss_rule(a["pred"], a["target"], a["valid"], a["sign"], a["weight"], lt, W_SDF, w_fs, b["trunc"])
    mag = np.abs(g) + np.abs(gf)                    # (both already carry the 1/n)
    if on_lattice and _pow2(n):
        # every factor is a short dyadic (w_sdf w slope: <= 5 + 6 + 2 bits; + w_fs: multiples of 2^-8 below 16) and inv_n a
        # power of two: nothing rounds
        assert np.array_equal(gp.astype(np.float64), g + gf)
        assert gfs is None or np.array_equal(gfs.astype(np.float64), gf)
    else:
        # on the lattice 2 roundings: fl(1 / fl(n)) and the product with it.  Off it at most 6: d = s - t, w_sdf * w, * d (L2;
        # * 2 is exact), g + gf, fl(1 / fl(n)), the product
        k = 2 if on_lattice else 6
        assert np.all(np.abs(gp - (g + gf)) <= lc.gamma(k) * mag)
        assert gfs is None or np.all(np.abs(gfs - gf) <= lc.gamma(2) * np.abs(gf))      # w_fs * inv_n: 2 roundings
    got = loss.astype(np.float64)
    if on_lattice and lt == "L1" and n <= 1024:
        # terms w |d| and max(up, lo) are multiples of 2^-12 below 2, so every partial sum of at most 1024 of them is a
        # multiple of 2^-12 below 2^11: 23 bits, representable -- any summation order gives the exact sum.  A power-of-two
        # n leaves it exact through w * sum * inv_n and the atomics (multiples of 2^-21 below 4)
        if _pow2(n):
            assert np.array_equal(got, terms)
        else:
            assert np.all(np.abs(got - terms) <= lc.exact_sum_bounds(terms, B))
    else:
        abs_sums = lc.abs_term_sums(a["pred"], a["target"], a["valid"], a["sign"], a["weight"], lt, w_fs, b["trunc"])
        assert np.all(np.abs(got - terms) <= lc.term_bounds(abs_sums, n, K, B, weights=(W_SDF, w_fs)))
    if "sign" in drop or w_fs <= 0:
        assert got[1] == 0.0 and (gfs is None or not gfs.any())
    return terms, g, gf


@gpu
@pytest.mark.parametrize("want_fs_grad", [True, False])
@pytest.mark.parametrize("lt", ["L1", "L2"])
@pytest.mark.parametrize("n", VEC_SIZES + SCALAR_SIZES)
def test_column_kernel_on_the_lattice(n, lt, want_fs_grad):
    b = _lattice(n, lt)
    lc.assert_planted(b)
    K, B = lc.column_launch(n, lc.takes_float4(n))
    _check_vs_rule(b, lt, _run_cols(b, lt, want_fs_grad), K, B, on_lattice=True)


@gpu
@pytest.mark.parametrize("lt", ["L1", "L2"])
@pytest.mark.parametrize("n", VEC_SIZES + SCALAR_SIZES)
def test_column_kernel_off_the_lattice(n, lt):
    """0.2 randn predictions, make_targets labels; planted: target == pred, the fp32 tie up == lo > 0 built from the
    prediction's bits, and the targets one ulp above and below it."""
    b = _random(n, lt)
    lc.assert_planted(b, classes=("d0", "tie_pos", "up_gt", "lo_gt"), odd=False)
    K, B = lc.column_launch(n, lc.takes_float4(n))
    _check_vs_rule(b, lt, _run_cols(b, lt), K, B, on_lattice=False)


@gpu
@pytest.mark.parametrize("lt", ["L1", "L2"])
def test_an_offset_view_falls_back_to_the_scalar_form_with_the_same_bits(lt):
    """Each of the seven arrays in turn as a [1:] view of an n + 1 allocation (4 bytes off a 16-byte boundary: the launch
    must take the scalar form), then as a [4:] view (aligned again): gradients bit for bit those of the aligned run, and
    the loss terms too (L1: exact sums, see _check_vs_rule; L2 on its 2^-4 lattice: terms w d^2 are multiples of 2^-12
    below 4, 1024 of them stay below 2^12: 24 bits).  The element in front of an output view is not written."""
    from miso_amd import ops
    n = 1024
    b = _lattice(n, lt)
    lc.assert_planted(b)
    base = _run_cols(b, lt)
    _check_vs_rule(b, lt, base, *lc.column_launch(n, True), on_lattice=True)
    for off in (1, 4):
        for which in COLS + ("grad_pred", "grad_pred_fs"):
            a = {k: _dev(b[k]) for k in COLS}
            a["grad_pred"], a["grad_pred_fs"] = torch.full((n,), 9.0, device=DEV), torch.full((n,), 9.0, device=DEV)
            buf = torch.full((n + off,), 7.0, device=DEV)
            buf[off:] = a[which]
            a[which] = buf[off:]
            assert a[which].data_ptr() % 16 == (4 * off) % 16 and a[which].is_contiguous()
            loss = torch.full((2,), 9.0, device=DEV)
            ops.mapping_loss_raw(a["pred"], a["target"], a["valid"], a["sign"], a["weight"], lt, W_SDF, W_FS, b["trunc"],
                                 grad_pred=a["grad_pred"], loss_out=loss, grad_pred_fs=a["grad_pred_fs"])
            torch.cuda.synchronize()
            assert np.array_equal(loss.cpu().numpy(), base[0]), (which, off)
            assert np.array_equal(a["grad_pred"].cpu().numpy(), base[1]), (which, off)
            assert np.array_equal(a["grad_pred_fs"].cpu().numpy(), base[2]), (which, off)
            assert torch.all(buf[:off] == 7.0)


@gpu
@pytest.mark.parametrize("lt", ["L1", "L2"])
@pytest.mark.parametrize("n", [1024, 1023])
@pytest.mark.parametrize("drop", [("valid",), ("weight",), ("sign",), ("valid", "sign", "weight")])
def test_absent_columns(n, lt, drop):
    """valid None: every row counts; weight None: 1; sign None with w_fs > 0: no free-space term, grad_pred_fs zeros."""
    b = _lattice(n, lt)
    lc.assert_planted(b)
    K, B = lc.column_launch(n, lc.takes_float4(n))
    _check_vs_rule(b, lt, _run_cols(b, lt, drop=drop), K, B, on_lattice=True, drop=drop)


def _col2(b, k):
    return _dev(b[k]).reshape(-1, 1)


@gpu
@pytest.mark.parametrize("lt", ["L1", "L2"])
@pytest.mark.parametrize("form", ["float4", "scalar"])
def test_the_two_terms_take_different_upstream_gradients(form, lt):
    """ops.mapping_loss under (0.75, -2) and under (0, 1): pred.grad == 0.75 g_sdf - 2 g_fs and g_fs -- exact on the
    lattice at n = 1024 (g_sdf = (g + g_fs) - g_fs is exact; 0.75 g_sdf has 2 more bits, -2 g_fs none).  scalar: the
    target is a view one float off its allocation."""
    from miso_amd import ops
    n = 1024
    b = _lattice(n, lt)
    lc.assert_planted(b)
    _, g, gf = lc.loss_rule(b["pred"], b["target"], b["valid"], b["sign"], b["weight"], lt, W_SDF, W_FS, b["trunc"])
    target = _col2(b, "target")
    if form == "scalar":
        buf = torch.zeros(n + 1, 1, device=DEV)
        buf[1:] = target
        target = buf[1:]
        assert target.data_ptr() % 16 == 4
    for up, want in (((0.75, -2.0), 0.75 * g - 2.0 * gf), ((0.0, 1.0), gf)):
        pred = _col2(b, "pred").requires_grad_(True)
        terms = ops.mapping_loss(pred, target, _col2(b, "valid"), _col2(b, "sign"), _col2(b, "weight"), lt, W_SDF, W_FS,
                                 b["trunc"])
        if up == (0.0, 1.0):
            terms[1].backward()
        else:
            (terms * torch.tensor(up, device=DEV)).sum().backward()
        assert np.array_equal(pred.grad.cpu().numpy().reshape(-1).astype(np.float64), want)
    assert np.abs(gf).max() > 0 and np.abs(g).max() > 0


@gpu
@pytest.mark.parametrize("dtype", [torch.bool, torch.int64])
def test_label_dtypes_give_the_bits_of_the_float_call(dtype):
    from miso_amd import ops
    n = 1024
    b = _lattice(n, "L1")
    valid, sign = (_col2(b, "valid") == 1), (_col2(b, "sign") == 1)
    assert int(valid.sum()) > 64 and int((~valid).sum()) > 64 and int(sign.sum()) > 64
    outs = []
    for dt in (torch.float32, dtype):
        pred = _col2(b, "pred").requires_grad_(True)
        terms = ops.mapping_loss(pred, _col2(b, "target"), valid.to(dt), sign.to(dt), _col2(b, "weight"), "L1", W_SDF, W_FS,
                                 b["trunc"])
        terms.sum().backward()
        outs.append((terms.detach().clone(), pred.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][1].abs().max()) > 0


# ====================================================================================================================
# 3. the rows kernel
# ====================================================================================================================
def _rows(b):
    return torch.stack([_dev(b[k]) for k in ("target", "valid", "sign", "weight")], dim=1).contiguous()


def _run_rows(b, lt, w_fs=W_FS):
    from miso_amd import ops
    n = len(b["pred"])
    gp, loss = torch.full((n,), 9.0, device=DEV), torch.full((2,), 9.0, device=DEV)
    ops.mapping_loss_rows_raw(_dev(b["pred"]), _rows(b), lt, W_SDF, w_fs, b["trunc"], gp, loss)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), gp.cpu().numpy(), None


def _rows_launch(n):
    """launch_mapping_loss_rows: 256 threads, at most 64 blocks, one row per thread and pass."""
    return lc.column_launch(n, False)


@gpu
@pytest.mark.parametrize("lt", ["L1", "L2"])
@pytest.mark.parametrize("n", ROWS_SIZES)
@pytest.mark.parametrize("on_lattice", [True, False])
def test_rows_kernel(n, lt, on_lattice):
    """Interleaved (N,4) label rows: the same arithmetic per point as the column kernel -- grad_pred bit for bit -- and
    the loss terms against the rule."""
    b = _lattice(n, lt) if on_lattice else _random(n, lt)
    if on_lattice:
        lc.assert_planted(b)
    else:
        lc.assert_planted(b, classes=("d0", "tie_pos", "up_gt", "lo_gt"), odd=False)
    out = _run_rows(b, lt)
    _check_vs_rule(b, lt, out, *_rows_launch(n), on_lattice=on_lattice)
    assert np.array_equal(out[1], _run_cols(b, lt)[1])


@gpu
@pytest.mark.parametrize("w_fs", [0.0, -0.5])
@pytest.mark.parametrize("lt", ["L1", "L2"])
@pytest.mark.parametrize("n", [257, 1024])
@pytest.mark.parametrize("rows", [True, False])
def test_a_free_space_weight_that_is_not_positive_switches_the_term_off(rows, n, lt, w_fs):
    """w_fs = 0, and w_fs < 0 (MisoLossMapping forms the term under `weight_fs > 0` only): term 1 is 0 and no free-space
    share enters the gradient, even on rows with sign == 1 -- rows kernel and column kernel (scalar form at 257, float4
    at 1024)."""
    b = _lattice(n, lt)
    lc.assert_planted(b)
    out = _run_rows(b, lt, w_fs=w_fs) if rows else _run_cols(b, lt, w_fs=w_fs)
    K, B = _rows_launch(n) if rows else lc.column_launch(n, lc.takes_float4(n))
    _, g, gf = _check_vs_rule(b, lt, out, K, B, on_lattice=True, w_fs=w_fs)
    assert not gf.any() and out[0][1] == 0.0
    free_only = (b["sign"] == 1) & (b["valid"] != 1) & (b["masks"]["up_gt"] | b["masks"]["lo_gt"])
    assert free_only.sum() >= 1 and not out[1][free_only].any()


@gpu
def test_rows_pointer_off_its_alignment_is_refused_and_nothing_is_written():
    from miso_amd import _lib, ops
    n = 256
    b = _lattice(n, "L1")
    flat = torch.zeros(4 * n + 1, device=DEV)
    rows = flat[1:].view(n, 4)
    rows.copy_(_rows(b))
    assert rows.is_contiguous() and rows.data_ptr() % 16 == 4
    gp, loss = torch.full((n,), 9.0, device=DEV), torch.full((2,), 9.0, device=DEV)
    with pytest.raises(_lib.MisoError) as e:
        ops.mapping_loss_rows_raw(_dev(b["pred"]), rows, "L1", W_SDF, W_FS, b["trunc"], gp, loss)
    assert e.value.code == _lib.E_BADARG
    torch.cuda.synchronize()
    assert torch.all(gp == 9.0) and torch.all(loss == 9.0)


# ====================================================================================================================
# 4. the fused homes: ties planted from the kernels' own output
# ====================================================================================================================
from test_train_fused import _both, _check, _setup      # noqa: E402  (the two-launch / one-launch pair and its comparison)

FUSED_SHAPES = [(4, (16, 80), 64), (8, (32, 64, 128), 64)]


@functools.lru_cache(maxsize=None)
def _ctx(shape, binned):
    """One grid, decoder and batch (3000 points unbinned, 20000 binned), and pass 1: the forward with the loss folded in,
    run once for its SDF bits -- every later batch's labels are built from them on the host."""
    from miso_amd import ops
    C, sizes, H = FUSED_SHAPES[shape]
    n = 20000 if binned else 3000
    feats, meta, pack, x, _ = _setup(C, sizes, H, n, seed=70 + shape + (10 if binned else 0))
    c = types.SimpleNamespace(feats=feats, meta=meta, pack=pack, x=x, n=n, binned=binned,
                              sb=ops.SortedBatch(n, DEV).sort(x, meta) if binned else None)
    neutral = np.tile(np.array([0, 1, 0, 1], dtype=F32), (n, 1))
    c.s = _fwd_loss(c, neutral, "L1", 1.0, 0.0, 0.0).sdf
    assert np.isfinite(c.s).all()
    # the truncation distance of the tie batches: the upper quartile of the predictions, so that three rows in four lie
    # below it (lo > 0) wherever this decoder's output happens to be centred
    c.trunc = float(F32(np.quantile(c.s.astype(np.float64), 0.75)))
    rs = np.random.RandomState(shape)
    c.weight = rs.uniform(0.5, 1.5, n).astype(F32)
    c.noise = (0.05 * rs.standard_normal(n)).astype(F32)
    return c


def _aux(c, target, valid, sign, weight):
    a = np.empty((c.n, 4), dtype=F32)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = target, valid, sign, weight
    return a


def _fwd_loss(c, aux, lt, ws, wf, td, n_live=None):
    """sdf_fwd_kernel with the loss folded in (miso_sdf_fwd_loss, over a binned batch and over caller-order points):
    -> slots (LOSS_SLOTS, 2) float64, gsdf in the CALLER's order, sdf."""
    from miso_amd import ops
    n = c.n
    mask = ops.sdf_mask_buffer(c.pack, n, DEV)
    g = torch.full((n,), 9.0, device=DEV)
    slots, sdf = torch.full((ops._lib.LOSS_SLOTS, 2), 9.0, device=DEV), torch.full((n, 1), 9.0, device=DEV)
    if c.binned:
        ops.sdf_fwd_loss_raw(c.feats, c.meta, c.pack, c.sb, _dev(aux), mask, g, slots, lt, ws, wf, td, sdf_out=sdf,
                             n_live=n_live)
        caller = torch.full((n,), 9.0, device=DEV)
        caller[c.sb.perm.long()] = g                 # gsdf_sorted[p] belongs to point perm[p]
        g = caller
    else:
        ops.sdf_fwd_loss_unsorted_raw(c.x, c.feats, c.meta, c.pack, _dev(aux), mask, g, slots, lt, ws, wf, td, sdf_out=sdf)
    torch.cuda.synchronize()
    return types.SimpleNamespace(slots=slots.cpu().double().numpy(), gsdf=g.cpu().numpy(), sdf=sdf.cpu().numpy().reshape(-1),
                                 mask=mask)


def _train(c, aux, lt, ws, wf, td, n_live=None, full_trips=False):
    """sdf_train_kernel (miso_sdf_train; binned: every level pulled and OVERWRITTEN; unbinned: every
    level scattered INTO zeroed gradients -- in 32-point trips at this size, in 64-point trips under MISO_F_FULL_TRIPS)
    -> slots float64, sdf, level gradients."""
    import dataclasses
    from miso_amd import ops
    n = c.n
    meta = dataclasses.replace(c.meta, flags=c.meta.flags | ops._lib.F_FULL_TRIPS) if full_trips else c.meta
    slots, sdf = torch.full((ops._lib.LOSS_SLOTS, 2), 9.0, device=DEV), torch.full((n, 1), 9.0, device=DEV)
    if c.binned:
        grads = [torch.full_like(f, -3.0) for f in c.feats]
        assert ops.sdf_train_supported(c.feats, c.meta, grads) and ops.sdf_train_scattered_levels(c.feats, c.meta, grads) == 0
        ops.sdf_train_raw(c.feats, c.meta, c.pack, c.sb, _dev(aux), slots, grads, lt, ws, wf, td, sdf_out=sdf, n_live=n_live)
    else:
        grads = [torch.zeros_like(f) for f in c.feats]
        ops.sdf_train_unsorted_raw(c.x, c.feats, meta, c.pack, _dev(aux), slots, grads, lt, ws, wf, td, sdf_out=sdf)
    torch.cuda.synchronize()
    return types.SimpleNamespace(slots=slots.cpu().double().numpy(), sdf=sdf.cpu().numpy().reshape(-1), grads=grads)


def _slot_bounds(c, aux, lt, wf, td, div=None):
    """Bound of the two slot totals (the test adds the LOSS_SLOTS partials in float64: B = 0): K points in a lane, 6
    shuffle steps, at most 3 additions of the wavefronts' sums (eight wavefronts: (a + b) + (c + d), twice, + 1)."""
    abs_sums = lc.abs_term_sums(c.s, aux[:, 0], aux[:, 1], aux[:, 2], aux[:, 3], lt, wf, td)
    return lc.term_bounds(abs_sums, c.n, lc.fused_K(c.n), 0, weights=(W_SDF, wf), div=div, lds_adds=3)


def _trains(c, *a, **kw):
    """The training kernel's launches for this batch: one binned, or the unbinned one in both trip sizes."""
    return [_train(c, *a, **kw)] + ([] if c.binned else [_train(c, *a, full_trips=True, **kw)])


def _all_zero(grads):
    return all(int(torch.count_nonzero(g)) == 0 for g in grads)


def _ties(c):
    t, t_up, t_down, kept, strict = lc.fs_ties(c.s, c.trunc)
    # three predictions in four lie below trunc and nearly all of those keep their tie (28 % .. 99.8 % of normal draws do,
    # whatever their spread): fewer than 64 of the first 1024 rows means the construction is broken
    assert kept[:1024].sum() >= 64
    return t, t_up, t_down, kept, strict


CTX = [pytest.param(s, b, id=f"shape{s}-{'binned' if b else 'unbinned'}") for s in (0, 1) for b in (False, True)]


@gpu
@pytest.mark.parametrize("shape,binned", CTX)
def test_fused_zero_ties_have_no_slope(shape, binned):
    """Batch Z1 (L1): target = the kernel's own SDF bits, every row valid and free, trunc below every prediction: d == 0
    and up == lo == 0 on every row.  Both forwards-with-loss write +-0 for every point and 0 for both terms; every level
    gradient of the training kernel is exactly zero.  sign(0) = +-1, or a slope at the zero tie, fails without a tolerance."""
    c = _ctx(shape, binned)
    trunc = float(c.s.min()) - 1.0
    aux = _aux(c, c.s, 1, 1, c.weight)
    m = lc.classify(c.s, aux[:, 0], aux[:, 1], aux[:, 2], trunc)
    assert m["d0"].sum() == c.n and m["tie_zero"].sum() == c.n
    f = _fwd_loss(c, aux, "L1", W_SDF, W_FS, trunc)
    assert np.array_equal(f.sdf.view(np.uint32), c.s.view(np.uint32))      # the labels were built from these bits
    assert not f.gsdf.any() and not f.slots.any()
    for t in _trains(c, aux, "L1", W_SDF, W_FS, trunc):
        assert np.array_equal(t.sdf.view(np.uint32), c.s.view(np.uint32))
        assert not t.slots.any() and _all_zero(t.grads)


@gpu
@pytest.mark.parametrize("lt", ["L1", "L2"])
@pytest.mark.parametrize("shape,binned", CTX)
def test_fused_free_space_ties_have_no_slope(shape, binned, lt):
    """Batch Z2: no valid row; free rows sit ON the fp32 tie up == lo > 0 (loss_cases.fs_ties from the SDF bits).
    Gradients exactly zero in all four entry points, term 0 exactly 0, term 1 == w_fs mean(lo) of the rule."""
    c = _ctx(shape, binned)
    tie, _, _, kept, _ = _ties(c)
    aux = _aux(c, np.where(kept, tie, c.s), 0, kept.astype(F32), c.weight)
    m = lc.classify(c.s, aux[:, 0], aux[:, 1], aux[:, 2], c.trunc)
    assert m["tie_pos"].sum() == kept.sum() >= 64 and m["valid_out"].all() and not (m["up_gt"] | m["lo_gt"]).any()
    terms, g, gf = lc.loss_rule(c.s, aux[:, 0], aux[:, 1], aux[:, 2], aux[:, 3], lt, W_SDF, W_FS, c.trunc)
    assert not g.any() and not gf.any() and terms[0] == 0.0 and terms[1] > 0
    bound = _slot_bounds(c, aux, lt, W_FS, c.trunc)
    f = _fwd_loss(c, aux, lt, W_SDF, W_FS, c.trunc)
    ts = _trains(c, aux, lt, W_SDF, W_FS, c.trunc)
    assert np.array_equal(f.sdf.view(np.uint32), c.s.view(np.uint32)) and not f.gsdf.any()
    for t in ts:
        assert np.array_equal(t.sdf.view(np.uint32), c.s.view(np.uint32)) and _all_zero(t.grads)
    for o in [f] + ts:
        assert not o.slots[:, 0].any()
        assert abs(o.slots[:, 1].sum() - terms[1]) <= bound[1]


def _batch_n(c):
    """Batch N: the tie targets moved one ulp, up on every other strict row (lo > up: slope -w_fs) and down on the rest
    (up > lo: +w_fs); every row valid with a random weight; the other rows are ordinary valid rows.  Mixed in: valid in
    {0.5, 2} (rows i % 7 == 3) and sign in {-1, 2} (rows i % 7 == 5), which must contribute nothing."""
    _, t_up, t_down, kept, strict = _ties(c)
    idx = np.arange(c.n)
    rank = np.cumsum(strict) - 1
    goes_up = strict & (rank % 2 == 0)
    target = np.where(strict, np.where(goes_up, t_up, t_down), c.s + c.noise).astype(F32)
    valid, sign = np.ones(c.n, dtype=F32), strict.astype(F32)
    valid[idx % 7 == 3] = np.where((idx // 7) % 2 == 0, 0.5, 2.0)[idx % 7 == 3]
    sign[idx % 7 == 5] = np.where((idx // 7) % 2 == 0, -1.0, 2.0)[idx % 7 == 5]
    return _aux(c, target, valid, sign, c.weight), strict, goes_up


def _check_batch_n(c, aux, strict, goes_up, lt, f, terms, g, gf, live=None):
    n = c.n if live is None else live
    m = lc.classify(c.s, aux[:, 0], aux[:, 1], aux[:, 2], c.trunc)
    free = m["up_gt"] | m["lo_gt"]
    # the slope is there on the moved rows and changes sign between the halves
    up_rows, down_rows = free & goes_up, free & strict & ~goes_up
    assert up_rows[:n].sum() >= 24 and down_rows[:n].sum() >= 24 and not m["tie_pos"].any()
    assert np.all(gf[up_rows] < 0) and np.all(gf[down_rows] > 0)
    assert m["valid_odd"][:n].sum() >= 64 and m["sign_odd"][:n].sum() >= 64
    dead = m["valid_out"] & m["sign_out"]                       # rows outside both terms
    assert dead[:n].sum() >= 16 and not g[dead].any() and not gf[dead].any()
    assert np.array_equal(f.sdf.view(np.uint32), c.s.view(np.uint32))
    # at most 6 roundings per point: d = s - t, w_sdf * w, * d (L2), g + gf, fl(1 / fl(n)), the product
    assert np.all(np.abs(f.gsdf - (g + gf)) <= lc.gamma(6) * (np.abs(g) + np.abs(gf)))
    assert not f.gsdf[dead].any()
    only_fs = m["valid_out"] & free
    assert only_fs[:n].sum() >= 1 and np.all(np.sign(f.gsdf[only_fs]) == np.sign(gf[only_fs]))


@gpu
@pytest.mark.parametrize("lt", ["L1", "L2"])
@pytest.mark.parametrize("shape,binned", CTX)
def test_fused_one_ulp_off_the_tie_and_outside_valued_labels(shape, binned, lt):
    """Batch N (_batch_n): d loss / d sdf of both forwards-with-loss against the rule's g_sdf + g_fs, decided from the same
    SDF bits; the slot totals of all entry points against its terms; the training kernel against the two launches."""
    from miso_amd import ops
    c = _ctx(shape, binned)
    aux, strict, goes_up = _batch_n(c)
    assert strict.sum() >= 64
    terms, g, gf = lc.loss_rule(c.s, aux[:, 0], aux[:, 1], aux[:, 2], aux[:, 3], lt, W_SDF, W_FS, c.trunc)
    f = _fwd_loss(c, aux, lt, W_SDF, W_FS, c.trunc)
    _check_batch_n(c, aux, strict, goes_up, lt, f, terms, g, gf)
    bound = _slot_bounds(c, aux, lt, W_FS, c.trunc)
    ts = _trains(c, aux, lt, W_SDF, W_FS, c.trunc)
    for o in [f] + ts:
        assert np.all(np.abs(o.slots.sum(0) - terms) <= bound)
    assert not any(_all_zero(t.grads) for t in ts)
    if binned:
        _check(*_both(c.feats, c.meta, c.pack, c.x, _dev(aux), lt, W_SDF, W_FS, c.trunc))
    else:
        # the two launches on the same zeroed buffers: equal to the order of the float atomics (the bound of
        # test_train_fused.py::test_unbinned_train_kernel_equals_forward_plus_backward)
        g2 = [torch.zeros_like(x) for x in c.feats]
        ops.sdf_bwd_raw(c.x, c.feats, c.meta, c.pack, _dev(f.gsdf).reshape(-1, 1), f.mask, False, [True] * len(c.feats), g2)
        torch.cuda.synchronize()
        for t in ts:
            assert np.array_equal(t.sdf.view(np.uint32), c.s.view(np.uint32))
            for a, b in zip(t.grads, g2):
                assert (a - b).abs().max().item() <= 2e-5 * b.abs().max().item() + 1e-9


@gpu
@pytest.mark.parametrize("lt", ["L1", "L2"])
def test_fused_padded_batch_divides_by_the_live_rows(lt):
    """Binned entry, rows past n_live neutral (all four labels 0): they contribute nothing and the means divide by n_live."""
    c = _ctx(0, True)
    live = 17000
    aux, strict, goes_up = _batch_n(c)
    aux[live:] = 0.0
    nl = torch.tensor([live], device=DEV, dtype=torch.int32)
    terms, g, gf = lc.loss_rule(c.s, aux[:, 0], aux[:, 1], aux[:, 2], aux[:, 3], lt, W_SDF, W_FS, c.trunc, n_mean=live)
    assert not g[live:].any() and not gf[live:].any()
    f = _fwd_loss(c, aux, lt, W_SDF, W_FS, c.trunc, n_live=nl)
    _check_batch_n(c, aux, strict & (np.arange(c.n) < live), goes_up, lt, f, terms, g, gf, live=live)
    assert not f.gsdf[live:].any()
    bound = _slot_bounds(c, aux, lt, W_FS, c.trunc, div=live)
    t = _train(c, aux, lt, W_SDF, W_FS, c.trunc, n_live=nl)
    for o in (f, t):
        assert np.all(np.abs(o.slots.sum(0) - terms) <= bound)
    _check(*_both(c.feats, c.meta, c.pack, c.x, _dev(aux), lt, W_SDF, W_FS, c.trunc, n_live=nl))
