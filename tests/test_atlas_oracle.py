"""The fused atlas query (atlas_sdf_kernel, csrc/atlas.hip + atlas_eval.hpp) and its one-launch backward
(atlas_sdf_bwd_kernel + atlas_pose_reduce_kernel, csrc/atlas_bwd.hip) against the fp64 oracle at the kernels' own fp32
membership and coordinates (oracle.atlas64; atlases, points and bars: tests/atlas_cases.py, what they rest on:
tests/test_atlas_host.py).  Raw calls -- ops.AtlasQuery.__call__ and AtlasQuery._backward -- in both decoder forms:
features, SDF, gx, the (S,12) pose-table gradient and every level gradient, no finite row left out, equal non-finite
sets; then the statements that hold exactly, the lattice form, the persistent loops' second trip, and GridAtlas with
fused_backward down to the gradients of the pose corrections.  The worst ratio per output and form is printed at the end."""
import time

import pytest
import torch

import atlas_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = ("exact_fp32", "split")


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    A.WORST.clear()
    t0 = time.time()
    yield
    if A.WORST:
        print(f"\nworst |kernel - fp64| / bar per output and form ({time.time() - t0:.1f} s):",
              {k: f"{v:.3f}" for k, v in sorted(A.WORST.items()) if k.startswith("atlas")})


_DEVICE = {}


def on_device(a):
    """(features channels-last, metas, pose table, decoder pack, query) of an atlas_cases.Atlas, uploaded once"""
    from miso_amd import ops
    if a.name not in _DEVICE:
        feats = [[f.to(DEV).contiguous(memory_format=torch.channels_last_3d) for f in fs] for fs in a.feats]
        metas = [ops.GridMeta.from_bound(b, None if a.ignore is None else a.ignore[s]) for s, b in enumerate(a.bounds)]
        pack = ops.DecoderPack([w.to(DEV) for w in a.ws], [b.to(DEV) for b in a.bs])
        _DEVICE[a.name] = (feats, metas, a.poses.to(DEV).contiguous(), pack, ops.AtlasQuery())
    return _DEVICE[a.name]


def forward(a, form, x=None, axes=None):
    """-> (feats (N,F), sdf (N,)) on the device"""
    from miso_amd import ops
    feats, metas, poses, pack, q = on_device(a)
    with ops.exact_fp32(form == "exact_fp32"):
        sdf, rows = q(feats, metas, poses, pack, x=None if x is None else x.to(DEV), axes=axes, want_sdf=True, want_feats=True)
    torch.cuda.synchronize()
    return rows, sdf[:, 0]


def backward(a, form, x, gsdf, want=True):
    """-> (gx, gposes, level gradients) on the device; want False: neither gx nor the pose gradient is asked"""
    feats, metas, poses, pack, q = on_device(a)
    need = [[s not in a.locked] * len(fs) for s, fs in enumerate(feats)]
    out = q._backward(feats, metas, poses, pack, x.to(DEV).contiguous(), gsdf.to(DEV).contiguous(), want, want, need,
                      form == "exact_fp32")
    torch.cuda.synchronize()
    return out


def outputs(a, form, x, gsdf, want=True):
    rows, sdf = forward(a, form, x)
    gx, gposes, grids = backward(a, form, x, gsdf, want)
    return A.Outputs(rows, sdf, gx, gposes, grids)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", A.SMALL_CASES)
def test_every_output_within_its_bar(name, form):
    """every case and kind of row: features, SDF, gx, the pose-table gradient and the level gradients"""
    c = A.case(name)
    got = outputs(c.atlas, form, c.x, c.gsdf)
    A.check_outputs(form, f"{name}/{form}", got, c)
    if name in ("ignored", "locked"):
        # neither gx nor the pose gradient asked: the per-submap loop leaves early where it has nothing to scatter
        bare = outputs(c.atlas, form, c.x, c.gsdf, want=False)
        assert bare.gx is None and bare.gposes is None
        A.check_outputs(form, f"{name}/{form}/grids only", bare, c, fields=("grids",))


@pytest.mark.parametrize("form", FORMS)
def test_statements_that_hold_exactly(form):
    c = A.case("generic42")
    a, o, n = c.atlas, c.o, c.x.shape[0]
    got = outputs(a, form, c.x, c.gsdf)
    outside = (o.count == 0).to(DEV)
    # rows inside nothing: a zero feature row and exactly zero gx, whatever their wavefront
    assert not bool(got.feat[outside].any()) and not bool(got.gx[outside].any())
    # an outside row's SDF: the bits of sdf_empty (a run with no lane inside anything) and of the decoded zero mean (an
    # outside lane of a populated run) are the same
    lonely = got.sdf[65:128]                      # outside lanes beside one inside lane
    assert bool(o.inside[64].any()) and same_bits(lonely, got.sdf[0].expand_as(lonely)), \
        "the zero row decodes to other bits than sdf_empty"
    assert same_bits(got.sdf[outside], got.sdf[0].expand(int(outside.sum())))
    # a batch wholly outside: every gradient exactly zero
    far = torch.cat((c.x[:64], c.x[65:128], c.x[:3]))
    gx, gposes, grids = backward(a, form, far, torch.ones(far.shape[0]))
    assert not bool(gx.any()) and not bool(gposes.any()) and not any(bool(g.any()) for gs in grids for g in gs)
    # a row's features, SDF and gx do not depend on its neighbours: any order of the rows, and the row alone
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    moved = outputs(a, form, c.x[perm], c.gsdf[perm])
    for f in ("feat", "sdf", "gx"):
        assert same_bits(getattr(moved, f), getattr(got, f)[perm.to(DEV)]), f"{f} depends on the order of the rows"
    interior = (c.kind == A.K["interior"])
    rows = [int(torch.nonzero((o.count == k) & interior)[0]) for k in range(6)] + [256, 261, 266]      # (and three non-finite rows)
    for r in rows:
        alone = outputs(a, form, c.x[r:r + 1], c.gsdf[r:r + 1])
        for f in ("feat", "sdf", "gx"):
            assert same_bits(getattr(alone, f), getattr(got, f)[r:r + 1]), f"row {r} alone: other {f}"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dims", A.LATTICES)
def test_lattice_form_equals_the_point_list(dims, form):
    a = A.atlas("generic42")
    lo, hi = A.global_bound(a)
    axes = [torch.linspace(float(lo[i]), float(hi[i]), dims[i]) if dims[i] > 1 else torch.tensor([float(lo[i] + hi[i]) / 2])
            for i in range(3)]
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    rows_l, sdf_l = forward(a, form, axes=tuple(t.to(DEV) for t in axes))
    rows_p, sdf_p = forward(a, form, x=pts)
    assert same_bits(rows_l, rows_p) and same_bits(sdf_l, sdf_p)
    o = A.oracle(a, pts, torch.zeros(pts.shape[0]))
    A.check(f"atlas feat ({form})", f"lattice {dims}", rows_l, o.feat, A.feat_bar(o))
    A.check(f"atlas sdf ({form})", f"lattice {dims}", sdf_l, o.sdf, A.kbar(form, "sdf") * A.U * o.sdf_y + A.FLOOR)


@pytest.mark.parametrize("form", FORMS)
def test_second_trip_of_the_persistent_loops(form):
    """n beyond blocks x wavefronts x 64 (atlas_cases.N_STRIDE_*): every row against the oracle, and bit for bit the
    rows of launches below the cap"""
    c = A.case("stride_fwd")
    rows, sdf = forward(c.atlas, form, c.x)
    A.check(f"atlas feat ({form})", "stride_fwd", rows, c.o.feat, A.feat_bar(c.o))
    A.check(f"atlas sdf ({form})", "stride_fwd", sdf, c.o.sdf, A.bars(c, form).sdf)
    step = 1 << 18
    parts = [forward(c.atlas, form, c.x[i:i + step]) for i in range(0, c.x.shape[0], step)]
    assert same_bits(torch.cat([p[0] for p in parts]), rows) and same_bits(torch.cat([p[1] for p in parts]), sdf)
    c = A.case("stride_bwd")
    gx, gposes, grids = backward(c.atlas, form, c.x, c.gsdf)
    A.check_outputs(form, f"stride_bwd/{form}", A.Outputs(None, None, gx, gposes, grids), c, fields=("gx", "gposes", "grids"))
    step = 1 << 16
    parts = [backward(c.atlas, form, c.x[i:i + step], c.gsdf[i:i + step])[0] for i in range(0, c.x.shape[0], step)]
    assert same_bits(torch.cat(parts), gx)


@pytest.mark.parametrize("form", FORMS)
def test_grid_atlas_with_fused_backward_down_to_the_corrections(form):
    """GridAtlas.forward under autograd with fused_backward set, corrections unlocked: SDF, d/dx, every level gradient
    and the gradients of rotation_corrections / translation_corrections -- the oracle's table gradient pulled back
    through a float64 copy of the table's construction.  Non-finite rows: the fused forward, the fused backward and
    the package's loop on the device agree -- a zero-row SDF and exactly zero d/dx."""
    from miso_amd import ops
    m = A.module_atlas(DEV)
    with torch.no_grad():
        table = m._pose_table(DEV)
    c = A.module_case(m, table)
    n = c.x.shape[0]
    x, w = c.x.to(DEV), c.gsdf.to(DEV)
    with ops.exact_fp32(form == "exact_fp32"):
        m.fused_backward = True
        try:
            xd = x.clone().requires_grad_(True)
            sdf = m(xd)
            assert type(sdf.grad_fn).__name__ == "_AtlasSdfBackward", "the fused route was not taken"
            (w * sdf[:, 0]).sum().backward()
        finally:
            m.fused_backward = False
        with torch.no_grad():
            plain = m(x)
    torch.cuda.synchronize()
    assert same_bits(plain, sdf.detach())
    grids = [[g.feature.grad for g in sm.features] for sm in m.submaps]
    A.check_outputs(form, f"module/{form}", A.Outputs(None, sdf.detach()[:, 0], xd.grad, None, grids), c, fields=("sdf", "gx", "grids"))
    want, ys = A.corrections(m, c.o.gposes, c.o.gposes_y)
    for s, (wn, bar) in enumerate(zip(want, A.corrections_bars(form, n, ys))):
        A.check(f"atlas corrections ({form})", f"module/rotation {s}", m.rotation_corrections[s].grad, wn[0], bar[0])
        A.check(f"atlas corrections ({form})", f"module/translation {s}", m.translation_corrections[s].grad, wn[1], bar[1])
    # the package's loop on the same rows
    m.zero_grad(set_to_none=True)
    xl = x.clone().requires_grad_(True)
    loop = m(xl)
    assert type(loop.grad_fn).__name__ != "_AtlasSdfBackward"
    (w * loop[:, 0]).sum().backward()
    bad = ~torch.isfinite(x).all(1)
    assert int(bad.sum()) == 64 * 3 // 4 + 9
    zero = sdf.detach()[0, 0]                      # (row 0: the empty run)
    assert same_bits(sdf.detach()[bad, 0], zero.expand(int(bad.sum())))
    assert bool(((loop.detach()[bad, 0] - zero).abs() <= A.bars(c, "split").sdf[bad.cpu()].to(DEV).float()).all())
    assert not bool(xd.grad[bad].any()) and not bool(xl.grad[bad].any())
