"""CPU: what the GPU module tests/test_first_order_oracle.py rests on.
(a) oracle.trilinear_first64 equals fp64 F.grid_sample + autograd, on every row whose index coordinate ATen re-forms
    exactly or that lies 1e-3 index units from every plane -- cell planes, faces and clip limits of the dyadic grids
    included (the cell of floor, no gradient at and beyond a clip limit);
(b) with NaN / inf in a vertex its non-finite entries are ATen's, entry for entry;
(c) every bar of tests/sampler_cases.py accepts an fp32 evaluation in the kernels' order, in corner-weight form and
    in lerp-tree form;
(d) every bar rejects the planted faults that change the output it guards."""
import pytest
import torch

import sampler_cases as S
from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64
CS = (1, 3, 4, 8)
CONFIGS = [(grid, bname) for grid in S.GRIDS for bname in S.BOUNDS]


# --------------------------------------------------------------------------- #
# fp64 ATen at the kernel's coordinate
# --------------------------------------------------------------------------- #
def _aten(feats, bound, x32, gout, pad, ac):
    """-> value (N,F), grad_x (N,3), rows (N,) bool that can be compared: finite, and on every level each axis either
    re-forms the kernel's index coordinate exactly in fp64 or lies 1e-3 from every plane."""
    n = x32.shape[0]
    value, grad = [], torch.zeros(n, 3, dtype=F64)
    rows = torch.isfinite(x32).all(1)
    foff = 0
    for f in feats:
        c, sizes = f.shape[1], (f.shape[4], f.shape[3], f.shape[2])
        ix, mult = R.sample_index32(x32, bound, sizes, ac, "zeros")          # before the clip: ATen clips itself
        ix = torch.where(torch.isfinite(ix), ix, torch.zeros_like(ix))
        dix = torch.tensor([(s - 1) / 2 if ac else s / 2 for s in sizes], dtype=F64)
        xn = (ix / dix - 1) if ac else ((2 * ix + 1) / torch.tensor(sizes, dtype=F64) - 1)
        back = torch.stack([R._unnormalize(xn[:, a], sizes[a], ac) for a in range(3)], 1)
        away = ((ix - torch.round(ix)).abs() >= 1e-3) & ((back - ix).abs() <= 1e-9)
        rows &= ((back == ix) | away).all(1)
        xn.requires_grad_(True)
        v = R.grid_sample_stock(f.double(), xn, ac, pad)
        (gxn,) = torch.autograd.grad(v, xn, gout[:, foff:foff + c].double())
        value.append(v.detach())
        grad += mult * (gxn / dix)
        foff += c
    return torch.cat(value, 1), grad, rows


@pytest.mark.parametrize("pad,ac", S.MODES)
@pytest.mark.parametrize("grid,bname", CONFIGS)
def test_oracle_equals_float64_aten(grid, bname, pad, ac):
    """(a), and that the planted rows of the dyadic grids take part: they are where the conventions show."""
    for C in (1, 4):
        feats, pts, go, o = S.case(grid, bname, C, pad, ac)
        val, grad, rows = _aten(feats, S.BOUNDS[bname], pts.x, go, pad, ac)
        assert rows.float().mean() > 0.9
        if grid == "dyadic" and not ac and bname != "metric":
            planted = (pts.kind == S.K["planes"]) | (pts.kind == S.K["clip"]) | (pts.kind == S.K["beyond"]) | \
                      (pts.kind == S.K["faces"])
            assert rows[planted].all(), "a planted row of the dyadic grid is not compared"
        dv = ((o.value - val).abs() - (1e-12 * o.value_w + 1e-300))[rows]
        dg = ((o.grad_x - grad).abs() - (1e-12 * o.grad_w + 1e-300))[rows]
        assert dv.max().item() <= 0, f"value: {int((dv > 0).sum())} entries beyond 1e-12 of the yardstick"
        assert dg.max().item() <= 0, f"grad_x: {int((dg > 0).sum())} entries beyond 1e-12 of the yardstick"


@pytest.mark.parametrize("grid,bname", CONFIGS)
def test_planted_rows_are_where_they_were_planted(grid, bname):
    """A condition on the inputs: every planted row has the kernel's index coordinate exactly at (side 0), below
    (-1) or above (+1) its target on every planted axis; three-axis plane rows exist on every level; and one index step
    beyond -1 / size no corner of that level is in range."""
    for ac in (False, True):
        pts = S.points(grid, bname, ac)
        levels = [S.xyz(lv) for lv in S.GRIDS[grid]]
        assert 2000 <= pts.x.shape[0] <= 4000
        for l, sz in enumerate(levels):
            sel = pts.level == l
            ix, _ = R.sample_index32(pts.x[sel], S.BOUNDS[bname], sz, ac, "zeros")
            ax, tg, side = pts.axes[sel], pts.target[sel], pts.side[sel][:, None]
            ok = torch.where(side == 0, ix == tg, torch.where(side < 0, ix < tg, ix > tg))
            assert ok[ax].all() and ax.any(1).all()
            on = (pts.kind[sel] == S.K["planes"])
            assert (ix[on] == torch.round(ix[on]))[ax[on]].all()
            for n_axes in (1, 2, 3):
                assert int((ax[on].sum(1) == n_axes).sum()) >= (20 if grid == "dyadic" and not ac else 1), (l, n_axes)
            for kind in ("beyond", "clip"):
                assert int((pts.kind[sel] == S.K[kind]).sum()) >= 3 * 8 * 2, kind
        for k in S.KINDS:
            assert (pts.kind == S.K[k]).any(), k


@pytest.mark.parametrize("pad,ac", S.MODES)
def test_rows_with_their_own_expectation(pad, ac):
    """NaN coordinates give zero rows; +-inf and the far rows do under zero padding (under border padding they are
    clipped like any row beyond a limit: the border's value, no gradient on that axis); one index step beyond -1 /
    size the level's columns are exactly zero under zero padding."""
    feats, pts, go, o = S.case("odd", "metric", 4, pad, ac)
    nan_rows = torch.isnan(pts.x).any(1)
    assert int(nan_rows.sum()) == 3
    gone = nan_rows if pad == "border" else (pts.kind == S.K["nonfinite"]) | (pts.kind == S.K["far"])
    assert (o.value[gone] == 0).all() and (o.grad_x[gone] == 0).all()
    if pad == "border":
        held = (pts.kind == S.K["far"]) | ((pts.kind == S.K["nonfinite"]) & ~nan_rows)
        axis = (~torch.isfinite(pts.x) | (pts.x.abs() >= 1e9))[held]
        assert (o.grad_x[held][axis] == 0).all() and (o.value_w[held].sum(1) > 0).all()
    else:
        for l in range(2):
            sel = (pts.kind == S.K["beyond"]) & (pts.level == l) & (pts.side != 0)
            assert sel.any() and (o.value[sel][:, 4 * l:4 * l + 4] == 0).all()


@pytest.mark.parametrize("where", ["first", "face", "interior"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_vertex_reaches_atens_rows(where, value):
    """(b) in both paddings and both align_corners: the oracle's non-finite entries are fp64 ATen's."""
    for grid, bname in (("odd", "metric"), ("dyadic", "normalized")):
        for pad, ac in S.MODES:
            feats, pts, go, _ = S.case(grid, bname, 4, pad, ac)
            bad = S.plant_vertex(feats, where, value)
            o = S.oracle(bad, S.BOUNDS[bname], pts.x, go, pad, ac)
            val, grad, rows = _aten(bad, S.BOUNDS[bname], pts.x, go, pad, ac)
            assert torch.equal(torch.isfinite(o.value[rows]), torch.isfinite(val[rows])), (grid, pad, ac)
            assert torch.equal(torch.isfinite(o.grad_x[rows]), torch.isfinite(grad[rows])), (grid, pad, ac)
            hit = ~torch.isfinite(o.value).all(1)
            assert hit.any() and not hit[pts.kind == S.K["interior"]].all()
            if where != "first" or pad == "border":
                continue
            # the half cell along the faces and everything outside: rows with an out-of-range corner that do not have
            # vertex 0 in their cell stay finite
            outside = (pts.kind == S.K["far"]) | ((pts.kind == S.K["beyond"]) & (pts.side != 0))
            assert torch.isfinite(o.value[outside][:, 4:]).all()
            assert torch.isfinite(o.value[pts.kind == S.K["far"]]).all()


# --------------------------------------------------------------------------- #
# The kernels' arithmetic restated in torch ops of one dtype, with the faults a bar has to reject
# --------------------------------------------------------------------------- #
def _lerp_tree(v, tx, ty, tz):
    """trilinear.hpp lerp_tree: f, fx, fy, fz of eight zero-padded corner values, operation for operation."""
    d00, d10, d01, d11 = v[1] - v[0], v[3] - v[2], v[5] - v[4], v[7] - v[6]
    a00, a10, a01, a11 = v[0] + tx * d00, v[2] + tx * d10, v[4] + tx * d01, v[6] + tx * d11
    e0, e1 = a10 - a00, a11 - a01
    b0, b1 = a00 + ty * e0, a01 + ty * e1
    gx0, gx1 = d00 + ty * (d10 - d00), d01 + ty * (d11 - d01)
    return b0 + tz * (b1 - b0), gx0 + tz * (gx1 - gx0), e0 + tz * (e1 - e0), b1 - b0


def _restate(feats, cs, gout, form, dtype=F32, fault=None):
    """value (N,F) and grad_x (N,3) in ``dtype``, form "weight" (encode_fwd_kernel / encode_bwd_kernel<false>: corner
    weights, channel by channel) or "lerp" (lerp_tree's value; encode_bwd_x_kernel).  cs: per level (ix, mult).
    fault: None, "drop_corner" (corner 5 on every 100th row), "cell_below" (a row on a plane takes the cell below),
    "swap_xz" (the x and z weights exchanged), "foff" (the two levels' columns exchanged)."""
    n = gout.shape[0]
    F_ = sum(f.shape[1] for f in feats)
    value, grad = torch.zeros(n, F_, dtype=dtype), torch.zeros(n, 3, dtype=dtype)
    offs, foff = [], 0
    for f in feats:
        offs.append(foff)
        foff += f.shape[1]
    if fault == "foff":
        offs = offs[::-1]
    every = torch.arange(n) % 100 == 0
    for f, (ix, mult), fo in zip(feats, cs, offs):
        _, c, d, h, w = f.shape
        flat = f.reshape(c, d * h * w).to(dtype)
        pos = ix.to(dtype)
        pos = torch.where(torch.isfinite(pos).all(1)[:, None], pos, torch.full_like(pos, -4.0))
        fl = torch.floor(pos)
        if fault == "cell_below":
            fl = torch.where(pos == fl, fl - 1, fl)
        fl = torch.maximum(torch.minimum(fl, torch.tensor([w + 1.0, h + 1.0, d + 1.0], dtype=dtype)),
                           torch.tensor(-2.0, dtype=dtype))
        w1, w0, i0 = pos - fl, (fl + 1) - pos, fl.long()
        wt = [(w0[:, a], w1[:, a]) for a in range(3)]
        if fault == "swap_xz":
            wt = [wt[2], wt[1], wt[0]]
        v, wk, dw = [], [], []
        for k in range(8):
            o = (k & 1, (k >> 1) & 1, k >> 2)
            xi, yi, zi = i0[:, 0] + o[0], i0[:, 1] + o[1], i0[:, 2] + o[2]
            inb = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (zi >= 0) & (zi < d)
            if fault == "drop_corner" and k == 5:
                inb = inb & ~every
            lin = (zi.clamp(0, d - 1) * h + yi.clamp(0, h - 1)) * w + xi.clamp(0, w - 1)
            zero = torch.zeros((), dtype=dtype)
            v.append(torch.where(inb[:, None], flat[:, lin].t(), zero))                  # (N,C)
            sg = [1.0 if o[a] else -1.0 for a in range(3)]
            wk.append(torch.where(inb, (wt[0][o[0]] * wt[1][o[1]]) * wt[2][o[2]], zero))
            dw.append([torch.where(inb, sg[a] * wt[p][o[p]] * wt[q][o[q]], zero)
                       for a, (p, q) in enumerate(((1, 2), (0, 2), (0, 1)))])
        g = gout[:, fo:fo + c].to(dtype)
        t = (wt[0][1], wt[1][1], wt[2][1])
        acc = torch.zeros(n, 3, dtype=dtype)
        if form == "weight":
            for ch in range(c):
                a = torch.zeros(n, dtype=dtype)
                for k in range(8):
                    a = a + v[k][:, ch] * wk[k]
                    dk = g[:, ch] * v[k][:, ch]
                    for ax in range(3):
                        acc[:, ax] = acc[:, ax] + dk * dw[k][ax]
                value[:, fo + ch] = a
        else:
            for ch in range(c):
                value[:, fo + ch] = _lerp_tree([v[k][:, ch] for k in range(8)], *t)[0]
            dk = [torch.zeros(n, dtype=dtype) for _ in range(8)]
            for ch in range(c):
                for k in range(8):
                    dk[k] = dk[k] + g[:, ch] * v[k][:, ch]
            _, fx, fy, fz = _lerp_tree(dk, *t)
            acc = torch.stack([fx, fy, fz], 1)
        grad = grad + acc * mult.to(dtype)
    return value, grad


def _ratios(feats, cs, go, o, C, fault=None, dtype=F32):
    """worst |restatement - oracle| / bar of the four bars: value and grad_x, weight and lerp form"""
    out = {}
    for form, vbar, gbar in (("weight", S.value_bar_weight(o), S.grad_bar_weight(o, C)),
                             ("lerp", S.value_bar_lerp(o), S.grad_bar_lerp(o, C))):
        val, grad = _restate(feats, cs, go, form, dtype, fault)
        for name, got, ref, bar in (("value", val, o.value, vbar), ("grad_x", grad, o.grad_x, gbar)):
            r, same = S.excess(got, ref, bar)
            assert same
            out[f"{name}/{form}"] = r.max().item()
    return out


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("grid,bname", CONFIGS)
def test_bars_accept_fp32_in_the_kernels_order(grid, bname, C):
    """(c) on every row of every point set, the four flag combinations, random and one-hot cotangents."""
    worst = {}
    for pad, ac in S.MODES:
        for one_hot in (False, True):
            feats, pts, go, o = S.case(grid, bname, C, pad, ac, one_hot)
            cs = S.coords(feats, S.BOUNDS[bname], pts.x, pad, ac)
            for k, r in _ratios(feats, cs, go, o, C).items():
                worst[k] = max(worst.get(k, 0.0), r)
    print(f"{grid}/{bname}/C={C}: fp32 restatement, worst |fp32 - fp64| / bar: " +
          ", ".join(f"{k} {r:.3f}" for k, r in sorted(worst.items())))
    for k, r in worst.items():
        assert r <= 1.0, f"{k}: {r:.3f} x the bar"


def _faulty_coords(fault, feats, bound, x32, pad, ac):
    cs = S.coords(feats, bound, x32, pad, ac)
    if fault == "clip_mult":           # d ix / d x kept at and beyond a clip limit
        return [(c[0], z[1]) for c, z in zip(cs, S.coords(feats, bound, x32, "zeros", ac))]
    if fault == "no_gscale":           # the binned path's 2 / len left out
        sc = torch.tensor([2 / (b[1] - b[0]) for b in bound], dtype=F64)
        return [(c[0], c[1] / sc) for c in cs]
    if fault == "ac_size":             # size for size - 1 under align_corners (no clip involved: zero padding)
        out = []
        for f, c in zip(feats, cs):
            sizes = torch.tensor([f.shape[4], f.shape[3], f.shape[2]], dtype=F64)
            out.append((c[0] * sizes / (sizes - 1), c[1] * sizes / (sizes - 1)))
        return out
    return cs


# fault -> (padding, align_corners, bound, the bars that have to see it).  A row on a plane has the same VALUE in the
# cell below (the interpolant is continuous), and mult / gscale scale grad_x alone: the value bars are not asked there.
FAULTS = {
    "drop_corner": ("zeros", False, "metric", ("value", "grad_x")),
    "cell_below": ("zeros", False, "dyadic", ("grad_x",)),
    "clip_mult": ("border", False, "metric", ("grad_x",)),
    "ac_size": ("zeros", True, "metric", ("value", "grad_x")),
    "swap_xz": ("zeros", False, "metric", ("value", "grad_x")),
    "foff": ("zeros", False, "metric", ("value", "grad_x")),
    "no_gscale": ("zeros", False, "metric", ("grad_x",)),
}


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("fault", list(FAULTS))
def test_bars_reject_planted_faults(fault, C):
    """(d): the fault planted in the fp32 restatement, both forms; the same restatement without it passes (c)."""
    pad, ac, bname, seen_by = FAULTS[fault]
    grid = "dyadic" if fault == "cell_below" else "odd"
    for one_hot in (False, True):
        feats, pts, go, o = S.case(grid, bname, C, pad, ac, one_hot)
        cs = _faulty_coords(fault, feats, S.BOUNDS[bname], pts.x, pad, ac)
        for k, r in _ratios(feats, cs, go, o, C, fault).items():
            if k.split("/")[0] in seen_by:
                assert r > 1.0, f"{fault} passes the {k} bar ({r:.3f})"
