"""The sampled value and its first coordinate gradient, in every kernel form that produces them, against the fp64
oracle at the kernel's own fp32 index coordinate (oracle.trilinear_first64; inputs and bars: tests/sampler_cases.py,
what they rest on: tests/test_sampler_first_order_host.py).

value    encode_fwd_kernel<true> (channels-last, C = 4 / 8), encode_fwd_kernel<false> (NCDHW; channels-last C = 1 / 3),
         both again on a binned batch (perm / pre-normalised xn), gather_level through ops.AtlasQuery (one submap, identity
         pose, no bound test, features only), and the 5-D wrapper ops.grid_sample_3d
grad_x   encode_bwd_x_kernel (lerp tree: float4 levels, no grid gradient from the launch, 16-byte aligned rows),
         encode_bwd_kernel<true> (MISO_ENCODE_NO_LEAN=1; a grid gradient asked; rows of stride F + 1),
         encode_bwd_kernel<false> (NCDHW; C = 1 / 3), each on a binned batch as well

No row is left out: cell planes, faces, the fade-out of zero padding, both clip limits of border padding and one index
step either side, 1e9 away, NaN and +-inf coordinates (zero rows), and NaN / +-inf planted in the grid (the oracle's
non-finite entries and no other).  Per entry |kernel - fp64| <= bar; the worst ratio per form is printed at the end."""
import pytest
import torch

import sampler_cases as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    S.WORST.clear()
    yield
    if S.WORST:
        print("\nworst |kernel - fp64| / bar per form:", {k: f"{v:.3f}" for k, v in sorted(S.WORST.items())})


# --------------------------------------------------------------------------- #
# Calls
# --------------------------------------------------------------------------- #
def _meta(bname, pad, ac, ignore=None):
    from miso_amd import _lib, ops
    flags = (_lib.F_ALIGN_CORNERS if ac else 0) | (_lib.F_PAD_BORDER if pad == "border" else 0)
    bound = S.BOUNDS[bname]
    if bound is None:
        bound, flags = [[-1.0, 1.0]] * 3, flags | _lib.F_COORDS_NORMALIZED
    return ops.GridMeta.from_bound(bound, ignore, flags)


def _to_dev(feats, layout):
    fd = [f.to(DEV) for f in feats]
    return [f.contiguous(memory_format=torch.channels_last_3d) for f in fd] if layout == "cl" else fd


def _float4(C, layout):
    return layout == "cl" and C % 4 == 0


def _value(fd, meta, x, binned):
    from miso_amd import ops
    sb = ops.SortedBatch(x.shape[0], x.device).sort(x, meta) if binned else None
    return ops.encode_fwd_raw(x, fd, meta, sorted_batch=sb)


def _grad_x(fd, meta, x, go, binned, grid_gradient=False, rows="packed"):
    """rows: "packed", or "pitched" -- row stride F + 1, which the float4 loads of the lerp-tree kernel cannot take"""
    from miso_amd import ops
    n, F = go.shape
    if rows == "pitched":
        g = torch.zeros(n, F + 1, device=DEV)[:, :F]
        g.copy_(go)
        assert g.stride(0) % 4 != 0
    else:
        g = go.to(DEV)
    sb = ops.SortedBatch(n, x.device).sort(x, meta) if binned else None
    gx, grads = ops.encode_bwd_raw(x, fd, meta, g, True, [grid_gradient] * len(fd), sorted_batch=sb)
    torch.cuda.synchronize()
    return gx


def _check_all_forms(what, feats, bname, x32, go, o, C, layout, binned, pad, ac, monkeypatch, ignore=None, pitched=True):
    """value and grad_x of one configuration in every form its layout reaches"""
    fd, meta, x = _to_dev(feats, layout), _meta(bname, pad, ac, ignore), x32.to(DEV)
    tail = ("/binned" if binned else "")
    vform = ("encode_fwd<float4>" if _float4(C, layout) else "encode_fwd<scalar>") + tail
    S.check("value " + vform, f"{what} value", _value(fd, meta, x, binned), o.value, S.value_bar_weight(o))
    wbar, lbar = S.grad_bar_weight(o, C), S.grad_bar_lerp(o, C)
    if not _float4(C, layout):
        S.check("grad_x encode_bwd<scalar>" + tail, f"{what} grad_x", _grad_x(fd, meta, x, go, binned), o.grad_x, wbar)
        S.check("grad_x encode_bwd<scalar>" + tail, f"{what} grad_x + grid gradient",
                _grad_x(fd, meta, x, go, binned, grid_gradient=True), o.grad_x, wbar)
        return
    S.check("grad_x encode_bwd_x (lerp)" + tail, f"{what} grad_x lerp", _grad_x(fd, meta, x, go, binned), o.grad_x, lbar)
    S.check("grad_x encode_bwd<float4>" + tail, f"{what} grad_x + grid gradient",
            _grad_x(fd, meta, x, go, binned, grid_gradient=True), o.grad_x, wbar)
    if pitched:
        S.check("grad_x encode_bwd<float4>" + tail, f"{what} grad_x pitched rows",
                _grad_x(fd, meta, x, go, binned, rows="pitched"), o.grad_x, wbar)
    with monkeypatch.context() as m:
        m.setenv("MISO_ENCODE_NO_LEAN", "1")
        S.check("grad_x encode_bwd<float4>" + tail, f"{what} grad_x weight form", _grad_x(fd, meta, x, go, binned),
                o.grad_x, wbar)


# --------------------------------------------------------------------------- #
# Every form, the full point set
# --------------------------------------------------------------------------- #
CONFIGS = [(grid, bname, C, layout) for grid in S.GRIDS for bname in S.BOUNDS for C in (1, 3, 4, 8)
           for layout in ("cl", "ncdhw")]


@pytest.mark.parametrize("binned", [False, True], ids=["caller-order", "binned"])
@pytest.mark.parametrize("grid,bname,C,layout", CONFIGS, ids=["-".join(map(str, c)) for c in CONFIGS])
def test_value_and_grad_x_vs_fp64(grid, bname, C, layout, binned, monkeypatch):
    """The four padding x align_corners combinations on the whole concatenated point set; random cotangents over all
    channels, and for the float4 layouts one non-zero channel per level (a wrong feature offset reads zeros)."""
    for pad, ac in S.MODES:
        for one_hot in ((False, True) if _float4(C, layout) and not binned else (False,)):
            feats, pts, go, o = S.case(grid, bname, C, pad, ac, one_hot)
            _check_all_forms(f"{grid}/{bname}/C={C}/{layout}/{pad}/ac={ac}/one_hot={one_hot}", feats, bname, pts.x, go, o, C,
                             layout, binned, pad, ac, monkeypatch, pitched=not one_hot)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes(n, monkeypatch):
    """Partial wavefronts and workgroups: the first n rows of a shuffled point set (every kind of row among them)."""
    for (pad, ac), (C, layout) in zip((("zeros", False), ("border", True)), ((4, "cl"), (3, "ncdhw"))):
        feats, pts, go, o = S.case("odd", "metric", C, pad, ac)
        idx = torch.randperm(pts.x.shape[0], generator=torch.Generator().manual_seed(n))[:n]
        part = type(o)(*(t[idx] for t in o))
        for binned in ((False, True) if n else (False,)):      # (an empty batch has no bins)
            _check_all_forms(f"n={n}/{pad}/ac={ac}/C={C}/{layout}/binned={binned}", feats, "metric", pts.x[idx].contiguous(),
                             go[idx].contiguous(), part, C, layout, binned, pad, ac, monkeypatch)


@pytest.mark.parametrize("ignore", [(True, False), (False, True)], ids=["level0", "level1"])
def test_ignored_level_is_exactly_zero(ignore, monkeypatch):
    """An ignored level's columns are exactly zero and it adds nothing to grad_x (the oracle leaves it out)."""
    for C, layout in ((4, "cl"), (3, "ncdhw")):
        for pad, ac in (("zeros", False), ("border", True)):
            feats, pts, go, _ = S.case("odd", "metric", C, pad, ac)
            o = S.oracle(feats, S.BOUNDS["metric"], pts.x, go, pad, ac, ignore)
            l = ignore.index(True)
            assert (o.value[:, l * C:(l + 1) * C] == 0).all() and o.value.abs().sum() > 0
            for binned in (False, True):
                _check_all_forms(f"ignore={ignore}/C={C}/{layout}/{pad}/binned={binned}", feats, "metric", pts.x, go, o, C, layout,
                                 binned, pad, ac, monkeypatch, ignore=list(ignore))
                v = _value(_to_dev(feats, layout), _meta("metric", pad, ac, list(ignore)), pts.x.to(DEV), binned)
                assert (v[:, l * C:(l + 1) * C] == 0).all()


@pytest.mark.parametrize("pad,ac", S.MODES)
def test_grid_sample_3d_wrapper(pad, ac):
    """ops.grid_sample_3d: the (1,Do,Ho,Wo,3) grid and (1,C,Do,Ho,Wo) output reshapes, value and grad of the grid."""
    from miso_amd import ops
    for C, layout in ((3, "ncdhw"), (4, "cl")):
        feats, pts, go, _ = S.case("dyadic", "normalized", C, pad, ac)
        n = pts.x.shape[0] // 6 * 6
        x32, go1 = pts.x[:n], go[:n, C:]
        o = S.oracle(feats[1:], None, x32, go1, pad, ac)
        fd = _to_dev(feats[1:], layout)[0]
        grid = x32.to(DEV).reshape(1, n // 6, 3, 2, 3).requires_grad_(True)
        out = ops.grid_sample_3d(fd, grid, padding_mode=pad, align_corners=ac)
        assert out.shape == (1, C, n // 6, 3, 2)
        (gg,) = torch.autograd.grad(out, grid, go1.t().reshape(1, C, n // 6, 3, 2).to(DEV))
        S.check("value grid_sample_3d", f"grid_sample_3d/{pad}/ac={ac}/C={C} value", out.detach()[0].reshape(C, n).t(),
                o.value, S.value_bar_weight(o))
        S.check("grad_x grid_sample_3d", f"grid_sample_3d/{pad}/ac={ac}/C={C} grad", gg.reshape(n, 3), o.grad_x,
                S.grad_bar_lerp(o, C) if layout == "cl" else S.grad_bar_weight(o, C))


@pytest.mark.parametrize("grid,bname,C", [("odd", "metric", 4), ("dyadic", "dyadic", 8)])
def test_atlas_feature_rows(grid, bname, C):
    """gather_level<C, true> as the fused kernels inline it: ops.AtlasQuery on one submap with an identity pose and no
    bound test returns the mean over one submap, the feature row itself.  Finite grids and finite points (the pose
    product turns an inf coordinate into NaN on every axis before the sampler sees it)."""
    from miso_amd import ops
    ident = torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], device=DEV)
    for pad, ac in S.MODES:
        feats, pts, go, o = S.case(grid, bname, C, pad, ac)
        fin = torch.isfinite(pts.x).all(1)
        part = type(o)(*(t[fin] for t in o))
        _, got = ops.AtlasQuery()([_to_dev(feats, "cl")], [_meta(bname, pad, ac)], ident, None, x=pts.x[fin].to(DEV),
                                  want_sdf=False, want_feats=True, no_bound=True)
        torch.cuda.synchronize()
        S.check("value gather_level (atlas)", f"atlas/{grid}/C={C}/{pad}/ac={ac}", got, part.value, S.value_bar_weight(part))


# --------------------------------------------------------------------------- #
# Rows with their own expectation
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("binned", [False, True], ids=["caller-order", "binned"])
@pytest.mark.parametrize("C,layout", [(4, "cl"), (8, "cl"), (3, "cl"), (4, "ncdhw")])
def test_non_finite_coordinates_give_zero_rows(C, layout, binned, monkeypatch):
    """A NaN coordinate: value row 0 and grad_x row 0 in every form, whatever the padding; +-inf and 1e9 / 3e9 away the
    same under zero padding.  Under border padding +-inf is clipped like any coordinate beyond a
    limit: the border's value, no gradient on that axis -- the oracle's rows, which S.check compares.  The lerp-tree
    kernel formed 0 + t x 0 with t = NaN / inf there before it skipped a level with no corner in range."""
    from miso_amd import ops
    for pad, ac in S.MODES:
        feats, pts, go, o = S.case("odd", "metric", C, pad, ac)
        sel = (pts.kind == S.K["nonfinite"]) | (pts.kind == S.K["far"]) | (pts.kind == S.K["interior"])
        zero = torch.isnan(pts.x).any(1) if pad == "border" else (pts.kind == S.K["nonfinite"]) | (pts.kind == S.K["far"])
        assert (o.value[zero] == 0).all() and (o.grad_x[zero] == 0).all() and int(zero.sum()) >= 3
        fd, meta, x = _to_dev(feats, layout), _meta("metric", pad, ac), pts.x[sel].to(DEV)
        z = zero[sel].to(DEV)
        assert (_value(fd, meta, x, binned)[z] == 0).all()
        forms = [{}] + ([{"MISO_ENCODE_NO_LEAN": "1"}] if _float4(C, layout) else [])
        for env in forms:
            with monkeypatch.context() as m:
                for k, v in env.items():
                    m.setenv(k, v)
                gx = _grad_x(fd, meta, x, go[sel], binned)
            assert (gx[z] == 0).all(), f"{pad}/ac={ac}/{env}: grad_x at a non-finite coordinate: {gx[z][:4].tolist()}"
            S.check("grad_x non-finite coordinates", f"{pad}/ac={ac}/{env}", gx, o.grad_x[sel],
                    S.grad_bar_weight(type(o)(*(t[sel] for t in o)), C) if env or not _float4(C, layout)
                    else S.grad_bar_lerp(type(o)(*(t[sel] for t in o)), C))


@pytest.mark.parametrize("value", [NAN, INF, -INF], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("where", ["first", "face", "interior"])
def test_non_finite_grid_values_reach_their_rows_only(where, value, monkeypatch):
    """NaN / inf in one vertex: the non-finite entries of value and grad_x are the oracle's (fp64 ATen's, CPU test (b))
    and every other entry stays within its bar -- the three generic first-order kernels, every layout, binned too.
    Vertex 0 was the address an out-of-range corner loaded, and 0 x NaN reached every row that had lost a corner; such a
    corner now re-reads an in-range corner of its own cell (encode.hip, reread_in_range)."""
    for (C, layout), modes in (((4, "cl"), S.MODES), ((8, "cl"), S.MODES[1:3]), ((3, "cl"), S.MODES[:1]),
                               ((4, "ncdhw"), S.MODES[::3])):
        for pad, ac in modes:
            feats, pts, go, _ = S.case("odd", "metric", C, pad, ac)
            bad = S.plant_vertex(feats, where, value)
            o = S.oracle(bad, S.BOUNDS["metric"], pts.x, go, pad, ac)
            hit = ~torch.isfinite(o.value).all(1)
            assert hit.any() and not hit.all()
            for binned in (False, True):
                _check_all_forms(f"{where}={value}/C={C}/{layout}/{pad}/ac={ac}/binned={binned}", bad, "metric", pts.x, go, o, C,
                                 layout, binned, pad, ac, monkeypatch)
