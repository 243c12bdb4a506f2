"""ops.hash_encode on the GPU by gather equivalence: for a table T, the dense grid D[k, j, i, :] = T[row(i, j, k)] built
on the host with the numpy index (tests/hash_cases.py) is sampled by ops.encode, and the hashed encode must give the
same BITS in value, the oracle's value and d/dx within the bars of tests/sampler_cases.py, and the oracle's table
gradient -- the fp32 terms the kernel forms, summed in float64 through the index map -- within the reordering bound
m 2^-24 sum |terms| per row (hash_cases.py says why that is the bound), exactly where a row received one term.

Shapes: 5 x 7 x 3 and 23 x 17 x 9 vertices behind 2^6 rows (both hashed) and 2^8 rows (dense-indexed + hashed), every
channel count, batch sizes around the wavefront and the workgroup, every point kind of sampler_cases.points."""
import numpy as np
import pytest
import torch

import hash_cases as hc
import sampler_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _meta(ignore=None, flags=0):
    from miso_amd import ops
    return ops.GridMeta.from_bound(sc.BOUNDS[hc.BOUND], ignore, flags)


def _rows_of(o, idx):
    return type(o)(*(t[idx] for t in o))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _run(log2, C, n, ignore=(False, False), pad="zeros", ac=False, backward=True):
    """hash encode (and its backward) and the dense encode on n rows of the case; -> everything the checks need"""
    from miso_amd import _lib, ops
    ts, ds, pts, go, o = hc.case(log2, C, ignore, pad, ac)
    idx = hc.subset(n) if (pad, ac) == ("zeros", False) else torch.arange(pts.x.shape[0])
    x, g = pts.x[idx], go[idx]
    flags = (_lib.F_PAD_BORDER if pad == "border" else 0) | (_lib.F_ALIGN_CORNERS if ac else 0)
    meta = _meta(list(ignore), flags)
    xd = x.to(DEV).requires_grad_(backward)
    td = [t.to(DEV).requires_grad_(backward) for t in ts]
    out = ops.hash_encode(xd, td, meta, hc.DIMS, log2)
    with torch.no_grad():
        dense = ops.encode(x.to(DEV), [d.to(DEV).contiguous(memory_format=torch.channels_last_3d) for d in ds], meta)
    if backward:
        out.backward(g.to(DEV))
    torch.cuda.synchronize()
    return ts, x, g, _rows_of(o, idx), out, dense, xd, td


@pytest.mark.parametrize("n", hc.SIZES + (None,))
@pytest.mark.parametrize("C", hc.CHANNELS)
@pytest.mark.parametrize("log2", hc.LOG2S)
def test_value_and_gradients_by_gather_equivalence(log2, C, n):
    ts, x, g, o, out, dense, xd, td = _run(log2, C, n)
    tag = f"log2 {log2} C {C} n {n}"
    assert out.shape == (x.shape[0], 2 * C)
    assert torch.equal(_bits(out), _bits(dense)), f"{tag}: value differs from ops.encode on the dense grid"
    sc.check("hash-value", tag + " value", out, o.value, sc.value_bar_weight(o))
    if x.shape[0] == 0:
        assert xd.grad is None or xd.grad.shape == (0, 3)
        assert all(t.grad is None or not t.grad.any() for t in td)
        return
    sc.check("hash-grad-x", tag + " grad_x", xd.grad, o.grad_x, sc.grad_bar_weight(o, C))
    foff, singles, deepest = 0, 0, 0
    for l, (t, dims) in enumerate(zip(td, hc.DIMS)):
        ref, mag, m = hc.table_gradient64(hc.index_coords(x, dims), dims, log2, g[:, foff:foff + C].numpy(), C, t.shape[0])
        got = t.grad.detach().cpu().double().numpy()
        assert np.isfinite(got).all()
        bound = m[:, None] * hc.U * mag
        worst = np.abs(got - ref) - bound
        assert (worst <= 0).all(), (f"{tag} level {l}: table gradient {worst.max():.3e} beyond m 2^-24 sum|terms| at row "
                                    f"{int(np.argmax(worst.max(1)))} (m = {int(m[np.argmax(worst.max(1))])})")
        one = m == 1
        assert np.array_equal(got[one], ref[one]), f"{tag} level {l}: a row with one contribution is not exact"
        assert not got[m == 0].any(), f"{tag} level {l}: a row no corner maps to was written"
        singles, deepest = singles + int(one.sum()), max(deepest, int(m.max()))
        foff += C
    if n == 1:                                             # one point: a row holds one term unless its corners collide
        assert singles > 0
    elif n is None:                                        # ... and all of them: rows with many
        assert deepest >= 8


@pytest.mark.parametrize("ignore", [(True, False), (False, True)])
@pytest.mark.parametrize("log2", hc.LOG2S)
def test_ignored_levels_give_zeros_and_take_no_gradient(log2, ignore):
    C = 4
    ts, x, g, o, out, dense, xd, td = _run(log2, C, 257, ignore)
    assert torch.equal(_bits(out), _bits(dense))
    sc.check("hash-value", f"ignore {ignore} value", out, o.value, sc.value_bar_weight(o))
    sc.check("hash-grad-x", f"ignore {ignore} grad_x", xd.grad, o.grad_x, sc.grad_bar_weight(o, C))
    for l, ig in enumerate(ignore):
        cols = out[:, l * C:(l + 1) * C]
        if ig:
            assert not cols.any() and not td[l].grad.any()
        else:
            assert cols.any() and td[l].grad.any()


def test_other_sampling_flags_keep_the_equivalence():
    """border padding with align_corners=True: the flags only move the sample position, which the hashed encode takes
    from the same code."""
    ts, x, g, o, out, dense, xd, td = _run(8, 4, None, pad="border", ac=True)
    assert torch.equal(_bits(out), _bits(dense))
    sc.check("hash-value", "border/ac value", out, o.value, sc.value_bar_weight(o))
    sc.check("hash-grad-x", "border/ac grad_x", xd.grad, o.grad_x, sc.grad_bar_weight(o, 4))


def test_points_outside_and_nan_give_zero_rows_and_touch_no_row():
    from miso_amd import ops
    pts = hc.points()
    far = (pts.kind == sc.K["far"]) | (pts.kind == sc.K["nonfinite"])
    x = pts.x[far]
    assert x.shape[0] >= 12 and not torch.isfinite(x).all()
    for log2 in hc.LOG2S:
        td = [t.to(DEV).requires_grad_(True) for t in hc.tables(log2, 4)]
        xd = x.to(DEV).requires_grad_(True)
        out = ops.hash_encode(xd, td, _meta(), hc.DIMS, log2)
        out.backward(torch.ones_like(out))
        assert out.shape == (x.shape[0], 8) and not out.any()
        assert not xd.grad.any() and all(not t.grad.any() for t in td)
    # a poisoned table: nothing of it reaches rows that have no corner in range
    td = [torch.full_like(t, float("nan")).to(DEV) for t in hc.tables(6, 4)]
    assert not ops.hash_encode(x.to(DEV), td, _meta(), hc.DIMS, 6).any()


def test_no_double_backward():
    """create_graph=True builds a graph through the first backward; differentiating it raises a typed error.  Under
    coordinate_gradient_only (how the Eikonal term asks for d sdf / d x) the first backward forms no table gradient."""
    from miso_amd import ops
    ts = [t.to(DEV).requires_grad_(True) for t in hc.tables(8, 4)]
    x = hc.points().x[hc.subset(65)].to(DEV).requires_grad_(True)
    out = ops.hash_encode(x, ts, _meta(), hc.DIMS, 8)
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    assert gx.requires_grad
    with pytest.raises(ops.NoDoubleBackward, match="no second backward"):
        gx.square().sum().backward()
    with ops.coordinate_gradient_only():
        out = ops.hash_encode(x, ts, _meta(), hc.DIMS, 8)
        gx2, gt = torch.autograd.grad(out.sum(), [x, ts[0]], create_graph=True, allow_unused=True)
    assert torch.equal(gx2.detach(), gx.detach()) and gt is None


def _net_cfg(grid_type, log2=None):
    import golden_cases as gc
    cfg = gc.model_cfg(sc.BOUNDS[hc.BOUND], 0.4, 2.0, 2, 4, 64, init_stddev=0.1)
    cfg["grid"]["type"] = grid_type
    if log2 is not None:
        cfg["grid"]["log2_hashmap_size"] = log2
    return cfg


def test_dense_indexed_hash_gridnet_equals_the_regular_one_bit_for_bit(monkeypatch):
    """A hash GridNet whose levels all fit their table holds a FeatureGrid's values row for row: forward through the
    op-by-op route (encode + MLPNet, which is the hash net's only route) gives identical bits."""
    from miso_amd.grid_opt.models.grid_net import GridNet
    torch.manual_seed(3)
    reg = GridNet(_net_cfg("regular"), device=DEV).to(DEV)
    hsh = GridNet(_net_cfg("hash", 19), device=DEV).to(DEV)
    hsh.decoder.load_state_dict(reg.decoder.state_dict())
    with torch.no_grad():
        for a, b in zip(hsh.features, reg.features):
            assert a.dense_indexed and a.dims == tuple(reversed(b.feature.shape[2:]))
            a.feature.copy_(b.feature.permute(0, 2, 3, 4, 1).reshape(-1, a.feature.shape[1]))
    monkeypatch.setattr(GridNet, "_fused_decoder", lambda self, trainable=False: None)
    x = hc.points().x.to(DEV)
    with torch.no_grad():
        a, b = hsh(x), reg(x)
        fa, fb = hsh.query_feature(x), reg.query_feature(x)
    assert a.shape == (x.shape[0], 1) and torch.equal(_bits(fa), _bits(fb)) and torch.equal(_bits(a), _bits(b))
    assert a.abs().max() > 0


def test_large_dims_against_the_numpy_oracle_at_the_points():
    """2048^3 vertices (2^33: no dense grid can exist) behind 2^19 rows: the value at 257 points against a float64
    evaluation at those points only -- sample position from oracle.sample_index32, rows from the numpy index."""
    from miso_amd import ops
    dims, log2, C, n = (2048, 2048, 2048), 19, 4, 257
    g = torch.Generator().manual_seed(11)
    table = torch.randn(1 << log2, C, generator=g)
    b = torch.tensor(sc.BOUNDS[hc.BOUND], dtype=torch.float64)
    x = (b[:, 0] + (b[:, 1] - b[:, 0]) * (torch.rand(n, 3, generator=g, dtype=torch.float64) * 1.02 - 0.01)).float()
    x[0] = b[:, 1].float()                                  # the far corner of the bound: vertex 2047 on every axis
    out = ops.hash_encode(x.to(DEV), [table.to(DEV)], _meta(), [dims], log2).cpu().double()
    ix = hc.index_coords(x, dims).numpy()
    i0 = np.floor(ix).astype(np.int64)
    fr = ix - i0
    val, yard = np.zeros((n, C)), np.zeros((n, C))
    for k in range(8):
        o = (k & 1, (k >> 1) & 1, k >> 2)
        c = [i0[:, a] + o[a] for a in range(3)]
        inb = np.logical_and.reduce([(c[a] >= 0) & (c[a] < dims[a]) for a in range(3)])
        w = np.prod([fr[:, a] if o[a] else 1 - fr[:, a] for a in range(3)], axis=0)
        v = table.double().numpy()[hc.row_index(*[np.where(inb, c[a], 0) for a in range(3)], dims, log2)]
        val += np.where(inb[:, None], v * w[:, None], 0.0)
        yard += np.where(inb[:, None], np.abs(v) * w[:, None], 0.0)
    assert (yard > 0).all(1).sum() >= 200 and (i0.max(0) >= 2040).all()
    sc.check("hash-large", "2048^3 value", out, torch.from_numpy(val), 13 * sc.U * torch.from_numpy(yard) + sc.FLOOR)
