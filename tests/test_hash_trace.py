"""Sphere tracing through a hash GridNet in one launch (grid.hash_fused = True: GridNet.sphere_trace ->
ops.hash_sphere_trace, csrc/hash_trace.hip) against

  * the Python loop of utils_sdf.sphere_tracing over ``lambda p: net(p)``, the fused hash forward: points, masks, field
    values and step counts bit for bit, for ray counts around the 64-ray wavefront and the four-wavefront workgroup, every
    cut-off that stops rays on their way, both decoder arithmetics, a table where every level collides, an ignored
    level, rays outside the bound and non-finite rays;
  * atlas_trace_kernel: a hash net whose levels are all dense-indexed gives the regular net's bits in every output;
  * itself: a ray's result does not depend on the rays it shares a wavefront with;
  * diff.gradient3d (the normals) and the op-by-op route through render_depth.

The fixtures are tests/test_hash_routing.py's: [-1, 1]^3, level 0 (8^3 vertices) dense-indexed behind 2^10 rows, level 1
(16^3) hashed four vertices to a row, C = 4.  The fields are built as tests/test_sphere_trace.py builds its own: random
features, the decoder's output bias shifted so that a quarter of the origins start below epsilon, max_dist in the widest
gap between the distances the loop itself sees -- and the mix of outcomes is checked on the loop's record."""
import contextlib
import functools

import pytest
import torch

import hash_cases as hc
import sampler_cases as sc
import sphere_trace_cases as stc
import test_hash_routing as base
from test_sphere_trace import _gap, _shift_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MIN_DIST = 1e-4, 1e-3
COUNTS = (1, 63, 64, 65, 257, 1000)      # a lone lane, a chunk edge, a second chunk, a workgroup's fifth wavefront
ITERS = (1, 2, 3, 12, 100)
FORMS = ("split", "exact")


def _arith(form):
    from miso_amd import ops
    return ops.exact_fp32() if form == "exact" else contextlib.nullcontext()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype == torch.float32:
        a, b = _bits(a), _bits(b)
    assert torch.equal(a.cpu(), b.cpu()), f"{what}: differs on {int((a.cpu() != b.cpu()).reshape(a.shape[0], -1).any(1).sum())} rays"


def _net(log2=base.LOG2, fused=True, seed=0, std=1.0):
    """test_hash_routing's net with tables of 2^log2 rows and features of a size the decoder answers to"""
    from miso_amd.grid_opt.models.grid_net import GridNet
    cfg = base._cfg()
    cfg["grid"]["log2_hashmap_size"] = log2
    cfg["grid"]["hash_fused"] = fused
    torch.manual_seed(seed)
    net = GridNet(cfg, device=DEV).to(DEV)
    net.randn_features(std)
    assert [g.dims for g in net.features] == [(8, 8, 8), (16, 16, 16)]
    return net


def _rays(n, seed, margin=0.05):
    gen = torch.Generator().manual_seed(seed)
    o = (torch.rand(n, 3, generator=gen) * 2 - 1) * (1 + margin)
    d = torch.randn(n, 3, generator=gen) * (0.5 + torch.rand(n, 1, generator=gen))       # random, not unit length
    return o.to(DEV), d.to(DEV)


def _loop(net, o, d, **kw):
    """utils_sdf.sphere_tracing over a lambda (the Python loop) with every query logged.  -> dict: points, mask, dists
    (rounds, N), steps (N) int32 the rounds in which a ray moved, moving (N) at the cut-off, last (N,1) the loop's last
    field values"""
    import miso_amd.grid_opt.utils.utils_sdf as US
    log = []

    def query(p):
        s = net(p)
        log.append((p, s))
        return s

    points, mask = US.sphere_tracing(lambda p: query(p), o, d, **kw)
    dists = torch.stack([torch.norm(p - o, dim=1, keepdim=True) for p, _ in log])
    stop = torch.stack([s < kw["epsilon"] for _, s in log]) | (dists > kw["max_dist"])
    return dict(points=points, mask=mask, dists=dists[..., 0], steps=(~stop).sum(dim=0).reshape(-1).to(torch.int32),
                moving=~stop[-1].reshape(-1), last=log[-1][1])


def _check_against_loop(net, o, d, kw, tag):
    """the kernel's four outputs against the loop's record, bit for bit; -> the loop's record"""
    ref = _loop(net, o, d, **kw)
    clear = (ref["dists"] - kw["max_dist"]).abs()
    assert float(clear[~clear.isnan()].min()) >= 1e-5, f"{tag}: the far test hinges on a rounding"
    got = net.sphere_trace(o, d, want_sdf=True, want_steps=True, **kw)
    assert got is not None, "the fused trace was not taken"
    points, mask, extras = got
    n = o.shape[0]
    assert mask.dtype == torch.bool and tuple(mask.shape) == (n, 1) and tuple(points.shape) == (n, 3)
    _same(points, ref["points"], f"{tag} points")
    _same(mask, ref["mask"], f"{tag} mask")
    _same(extras["steps"], ref["steps"], f"{tag} steps")
    _same(extras["sdf"], net(points), f"{tag} sdf")
    frozen = ~ref["moving"]          # a ray that had stopped: the loop's last value is the value at its point
    _same(extras["sdf"][frozen], ref["last"][frozen], f"{tag} sdf of the stopped rays")
    return ref


@functools.lru_cache(maxsize=None)
def _case(name, form):
    """-> (net, origins, dirs, kw): the field of one configuration in one arithmetic, its output bias shifted, with
    max_dist chosen on the loop's own record; built once and left unchanged"""
    net = _net(log2=4 if name == "all_hashed" else base.LOG2)
    if name == "all_hashed":
        assert not any(g.dense_indexed for g in net.features) and all(g.rows == 16 for g in net.features)
    else:
        assert [g.dense_indexed for g in net.features] == [True, False]
    if name == "ignore1":
        net.ignore_level(1)
    o, d = _rays(1000, seed=7)
    with torch.no_grad(), _arith(form):
        net.decoder.linears()[-1].bias -= _shift_for(net(o), 0.25, EPS)
        free = dict(min_dist=MIN_DIST, max_dist=float("inf"), epsilon=EPS)
        # max_dist: what the farthest 15 - 30 % of the rays have reached after 12 rounds, in the widest gap between the
        # distances the loop sees in 100 (a run with a finite max_dist walks a prefix of each of these paths)
        q = torch.quantile(_loop(net, o, d, max_iters=12, **free)["dists"][-1], torch.tensor([0.70, 0.85], device=DEV))
        kw = dict(free, max_dist=_gap(_loop(net, o, d, max_iters=100, **free)["dists"], float(q[0]), float(q[1])))
    return net, o, d, kw


def _shares(ref):
    conv = ref["mask"].reshape(-1)
    return [float(v.float().mean()) for v in (conv, ~conv & ~ref["moving"], ref["moving"])]


# --------------------------------------------------------------------------------------------------------------------
# 1. the kernel is the loop, bit for bit
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_fused_trace_is_the_loop_bit_for_bit(form):
    net, o, d, kw = _case("plain", form)
    with torch.no_grad(), _arith(form):
        for iters in ITERS:
            for n in COUNTS:
                ref = _check_against_loop(net, o[:n], d[:n], dict(kw, max_iters=iters), f"{form} n={n} max_iters={iters}")
                if n == 1000 and iters == 12:      # hit, far, still moving at the cut-off: each a tenth of the rays
                    shares = _shares(ref)
                    print(f"{form}: max_dist {kw['max_dist']:.4f}, converged / far / moving {shares}")
                    assert min(shares) >= 0.10, shares
                if n == 1000 and iters == 1:
                    assert _shares(ref)[2] > 0.5      # (the short runs stop rays on their way)


def test_the_two_arithmetics_are_two_fields():
    from miso_amd import ops
    net, o, d, kw = _case("plain", "split")
    with torch.no_grad():
        a = net.sphere_trace(o, d, max_iters=12, **kw)[0]
        with ops.exact_fp32():
            b = net.sphere_trace(o, d, max_iters=12, **kw)[0]
    assert not torch.equal(_bits(a), _bits(b))      # the switch reaches the kernel


# --------------------------------------------------------------------------------------------------------------------
# 2. all levels dense-indexed: the regular net's kernel (atlas_trace_kernel), bit for bit in every output
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twins():
    """test_hash_sdf_routing.test_dense_indexed_twin_gives_the_regular_nets_fused_bits' construction"""
    import golden_cases as gc
    from miso_amd.grid_opt.models.grid_net import GridNet

    def cfg(grid_type):
        c = gc.model_cfg(sc.BOUNDS[hc.BOUND], 0.4, 2.0, 2, 4, 64, init_stddev=1.0)
        c["grid"]["type"] = grid_type
        if grid_type == "hash":
            c["grid"]["log2_hashmap_size"], c["grid"]["hash_fused"] = 19, True
        return c
    torch.manual_seed(3)
    reg = GridNet(cfg("regular"), device=DEV).to(DEV)
    hsh = GridNet(cfg("hash"), device=DEV).to(DEV)
    b = torch.tensor(sc.BOUNDS[hc.BOUND])
    gen = torch.Generator().manual_seed(11)
    o = (b[:, 0] - 0.1 + (b[:, 1] - b[:, 0] + 0.2) * torch.rand(777, 3, generator=gen)).to(DEV)
    d = torch.randn(777, 3, generator=gen).to(DEV)
    with torch.no_grad():
        reg.decoder.linears()[-1].bias -= _shift_for(reg(o), 0.25, EPS)
        hsh.decoder.load_state_dict(reg.decoder.state_dict())
        for a, r in zip(hsh.features, reg.features):
            assert a.dense_indexed and a.dims == tuple(reversed(r.feature.shape[2:]))
            a.feature.copy_(r.feature.permute(0, 2, 3, 4, 1).reshape(-1, a.feature.shape[1]))
    assert reg._fused_decoder() is not None and hsh._fused_hash_decoder() is not None
    return reg, hsh, o, d


@pytest.mark.parametrize("form", FORMS)
def test_dense_indexed_twin_gives_the_regular_kernels_bits(form, monkeypatch):
    from miso_amd import ops
    reg, hsh, o, d = _twins()
    calls = {"hash_sphere_trace": 0}
    real = ops.hash_sphere_trace
    monkeypatch.setattr(ops, "hash_sphere_trace", lambda *a, **k: calls.__setitem__("hash_sphere_trace", 1) or real(*a, **k))
    kw = dict(min_dist=MIN_DIST, max_dist=0.45, max_iters=16, epsilon=EPS, want_sdf=True, want_steps=True, grad_step=1e-2)
    with torch.no_grad(), _arith(form):
        p, m, e = reg.sphere_trace(o, d, **kw)
        ph, mh, eh = hsh.sphere_trace(o, d, **kw)
    assert calls["hash_sphere_trace"] == 1
    # worth comparing: rays that hit and rays that did not, that moved often and never, a gradient that is not flat
    assert 0.1 < float(m.float().mean()) < 0.9 and int(e["steps"].min()) == 0 and int(e["steps"].max()) >= 8
    assert float(e["grad"].abs().max()) > 0
    _same(ph, p, "points")
    _same(mh, m, "mask")
    for k in ("sdf", "steps", "grad"):
        _same(eh[k], e[k], k)


# --------------------------------------------------------------------------------------------------------------------
# 3. every level hashed with collisions (B = 4: 512 and 4096 vertices on 16 rows each); an ignored level
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["all_hashed", "ignore1"])
def test_colliding_tables_and_an_ignored_level(name, form):
    net, o, d, kw = _case(name, form)
    with torch.no_grad(), _arith(form):
        ref = _check_against_loop(net, o, d, dict(kw, max_iters=12), f"{name} {form}")
        shares = _shares(ref)
        print(f"{name} {form}: max_dist {kw['max_dist']:.4f}, converged / far / moving {shares}")
        assert min(shares) >= 0.10, shares
        if name == "ignore1":       # the level counts when it is not ignored
            net.include_level(1)
            other = net.sphere_trace(o, d, max_iters=12, **kw)[0]
            net.ignore_level(1)
            assert not torch.equal(_bits(other), _bits(ref["points"]))


# --------------------------------------------------------------------------------------------------------------------
# 4. outside the bound: the decoder's value at a zero row, on to `far`
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_rays_outside_the_bound_march_on_to_far(form):
    net = _net(seed=1)
    gen = torch.Generator().manual_seed(23)
    n = 257
    o = torch.rand(n, 3, generator=gen) * 2 - 1
    # half start outside -- past the half cell beyond the bound in which level 0's zero padding still fades -- ...
    o[: n // 2, 0] = 1.15 + 0.3 * torch.rand(n // 2, generator=gen)
    d = torch.randn(n, 3, generator=gen)
    d[: n // 4, 0] = d[: n // 4, 0].abs() + 0.5                                # ... half of those never come in
    o, d = o.to(DEV), d.to(DEV)
    with torch.no_grad(), _arith(form):
        last = net.decoder.linears()[-1]
        last.bias += 0.25 - net(torch.full((1, 3), 7.0, device=DEV)).reshape(-1)      # the zero row's value: 0.25
        outside = net(o[: n // 2])
        assert float((outside - 0.25).abs().max()) < 1e-6 and float(net(o).min()) > 0.05
        free = dict(min_dist=MIN_DIST, max_dist=float("inf"), epsilon=EPS, max_iters=100)
        kw = dict(free, max_dist=_gap(_loop(net, o, d, **free)["dists"], 2.9, 3.1))
        ref = _check_against_loop(net, o, d, kw, f"outside {form}")
        assert not ref["mask"].any() and not ref["moving"].any()               # every ray went far within max_iters
        assert int(ref["steps"].max()) < 100


# --------------------------------------------------------------------------------------------------------------------
# 5. non-finite rays
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_non_finite_rays_stay_unhit_and_leave_the_others_alone(form):
    net, o, d, kw = _case("plain", form)
    kw = dict(kw, max_iters=12)
    o, d = o[:65].clone(), d[:65].clone()
    bad_o, bad_d = 3, 40
    with torch.no_grad(), _arith(form):
        clean = net.sphere_trace(o, d, want_sdf=True, want_steps=True, **kw)
        o[bad_o, 0] = float("nan")
        d[bad_d, 2] = float("inf")
        ref = _check_against_loop(net, o, d, kw, f"non-finite {form}")         # bits equal the loop's, NaN words included
        got = net.sphere_trace(o, d, want_sdf=True, want_steps=True, **kw)
    assert not got[1][bad_o] and not got[1][bad_d]
    assert torch.isnan(got[0][bad_o]).any() and torch.isnan(got[0][bad_d]).any()
    keep = torch.ones(65, dtype=torch.bool, device=DEV)
    keep[[bad_o, bad_d]] = False
    _same(got[0][keep], clean[0][keep], "points of the finite rays")
    _same(got[1][keep], clean[1][keep], "mask of the finite rays")
    for k in ("sdf", "steps"):
        _same(got[2][k][keep], clean[2][k][keep], k)


# --------------------------------------------------------------------------------------------------------------------
# 6. a ray's result does not depend on its wavefront
# --------------------------------------------------------------------------------------------------------------------
def test_rays_do_not_depend_on_their_wavefront():
    net, o, d, kw = _case("plain", "split")
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(17)).to(DEV)
    kw = dict(kw, max_iters=12, want_sdf=True, want_steps=True, grad_step=1e-2)
    with torch.no_grad():
        p, m, e = net.sphere_trace(o, d, **kw)
        pp, mp, ep = net.sphere_trace(o[perm], d[perm], **kw)
    assert 0 < int(m.sum()) < 1000 and int(e["steps"].min()) < int(e["steps"].max())
    _same(pp, p[perm], "points")
    _same(mp, m[perm], "mask")
    for k in ("sdf", "steps", "grad"):
        _same(ep[k], e[k][perm], k)


# --------------------------------------------------------------------------------------------------------------------
# 7. central differences
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_normals(form):
    """grad = diff.gradient3d(points, net, 'finitediff', h): the six field values are the same bits, only the final
    scaling may round differently (a division here, a product with the reciprocal there) -- the tolerance of
    tests/test_sphere_trace.py::test_normals."""
    from miso_amd.grid_opt import diff
    net, o, d, kw = _case("plain", form)
    h = 1e-2
    with torch.no_grad(), _arith(form):
        points, _, extras = net.sphere_trace(o[:777], d[:777], max_iters=8, grad_step=h, **kw)
        ref = diff.gradient3d(points, net, 'finitediff', h)
    assert float(ref.abs().max()) > 0
    torch.testing.assert_close(extras["grad"], ref, rtol=5e-7, atol=0)


# --------------------------------------------------------------------------------------------------------------------
# 8. routing
# --------------------------------------------------------------------------------------------------------------------
def _count(monkeypatch, *names):
    """call counters on ops.<name> (tests/test_hash_sdf_routing.py's)"""
    from miso_amd import ops
    calls = {n: 0 for n in names}
    for n in names:
        def wrapped(*a, _n=n, _f=getattr(ops, n), **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, n, wrapped)
    return calls


def test_sphere_tracing_takes_the_one_launch_route(monkeypatch):
    import miso_amd.grid_opt.utils.utils_sdf as US
    net, o, d, kw = _case("plain", "split")
    kw = dict(kw, max_iters=12)
    with torch.no_grad():
        want = net.sphere_trace(o, d, **kw)
    calls = _count(monkeypatch, "hash_sphere_trace", "hash_sdf_fwd_raw", "hash_encode_fwd_raw")
    with torch.no_grad():
        points, mask = US.sphere_tracing(net, o, d, **kw)
        assert calls == {"hash_sphere_trace": 1, "hash_sdf_fwd_raw": 0, "hash_encode_fwd_raw": 0}
        _same(points, want[0], "points")
        _same(mask, want[1], "mask")
        US.sphere_tracing(net.forward, o, d, **kw)                                 # a bound method too
        assert calls["hash_sphere_trace"] == 2 and calls["hash_sdf_fwd_raw"] == 0
    # what declines: autograd on, a trainable decoder, the switch off -- the loop runs
    with torch.enable_grad():
        assert net.sphere_trace(o, d, **kw) is None
    seen = calls["hash_sphere_trace"]
    net.hash_fused = False
    try:
        with torch.no_grad():
            assert net.sphere_trace(o, d, **kw) is None
            US.sphere_tracing(net, o[:65], d[:65], **kw)
    finally:
        net.hash_fused = True
    assert calls["hash_sphere_trace"] == seen and calls["hash_encode_fwd_raw"] > 0
    other = _net(seed=2)
    for p in other.decoder.parameters():
        p.requires_grad_(True)
    with torch.no_grad():
        assert other._fused_hash_decoder() is None and other.sphere_trace(o, d, **kw) is None
    from miso_amd import ops
    trainable = ops.DecoderPack([l.weight for l in other.decoder.linears()], [l.bias for l in other.decoder.linears()])
    with torch.no_grad(), pytest.raises(ops.NotCovered, match="frozen decoder"):
        ops.hash_sphere_trace(*other._hash_args(detach=True), trainable, o, d, **kw)
    with torch.no_grad():      # no rays: empty results, nothing launched
        e = torch.empty(0, 3, device=DEV)
        points, mask = US.sphere_tracing(net, e, e)
        assert tuple(points.shape) == (0, 3) and tuple(mask.shape) == (0, 1) and mask.dtype == torch.bool


PLANE_Z, ZERO_ROW = -0.5, 0.3
VIEW = dict(eye=[0.03, -0.02, 0.6], look_at=[0.03, -0.02, -0.5], H=24, W=32, fx=229.0, fy=229.0, cx=15.5, cy=11.5)


def bake_plane(net):
    """The plane z = PLANE_Z as a hash net's field, in place: its signed distance less ZERO_ROW at the cell centres of
    the dense-indexed level 0 (channel 0; a plane is reproduced by trilinear interpolation away from the half cell at the
    bound), random values in every channel the decoder does not read, and sphere_trace_cases' pass-through decoder
    reading that one channel, with ZERO_ROW as its output bias: outside the bound the field is ZERO_ROW, not a surface."""
    with torch.no_grad():
        g0, g1 = net.features
        assert g0.dense_indexed and not g1.dense_indexed
        gen = torch.Generator().manual_seed(41)
        for g in (g0, g1):
            g.feature.copy_(torch.randn(g.feature.shape, generator=gen))
            g.feature[:, 0] = 0.0
        g0.feature[:, 0] = (g0.cell_centres()[:, 2] - PLANE_Z - ZERO_ROW).to(g0.feature)
        lin = net.decoder.linears()
        for l in lin:
            l.weight.zero_()
            l.bias.zero_()
        lin[0].weight[0, 0], lin[0].weight[1, 0] = 1.0, -1.0
        lin[1].weight[0, 0] = lin[1].weight[1, 1] = 1.0
        lin[2].weight[0, 0], lin[2].weight[0, 1] = 1.0, -1.0
        lin[2].bias.fill_(ZERO_ROW)
    return net


def test_render_depth_takes_the_route_and_agrees_with_the_op_by_op_net(monkeypatch):
    """The view looks down on the plane along its normal from inside the region where the interpolant is exact: a ray
    lands on the surface in two steps and no field value of the loop comes near epsilon (checked below on the loop's
    record; on the CPU oracle, in fp32 and in fp64, the same view gives second values 1.1 (1 - cos a) <= 3.9e-3 and third
    values <= 8.9e-5 that stay 1.08e-5 clear of epsilon, with no mask flipped between the two), so the two decoder routes,
    2.2e-6 apart at most, take the same stop decisions.  A grazing view does
    not: DESIGN.md 4.10."""
    import miso_amd.grid_opt.utils.utils_sdf as US
    from miso_amd.grid_opt.utils.utils_data import CameraParameters
    net = bake_plane(_net(seed=4))
    R, t = stc.camera_pose(VIEW)
    R, t = torch.from_numpy(R), torch.from_numpy(t)
    cam = CameraParameters(VIEW["fx"], VIEW["fy"], VIEW["cx"], VIEW["cy"], VIEW["H"], VIEW["W"])
    kw = dict(max_dist=1.5, min_dist=MIN_DIST, epsilon=EPS, max_iters=100)
    o, dw = (torch.from_numpy(a).to(DEV) for a in stc.rays(VIEW))
    with torch.no_grad():
        log = []
        US.sphere_tracing(lambda p: log.append(net(p)) or log[-1], o, dw, **kw)
        assert 2 <= len(log) <= 4 and float((torch.stack(log) - EPS).abs().min()) >= 5e-6      # (> twice 2.2e-6)
    calls = _count(monkeypatch, "hash_sphere_trace", "hash_sdf_fwd_raw", "hash_encode_fwd_raw")
    depth, mask, nrm = US.render_depth(net, R, t, cam, normals=True, **kw)
    assert calls == {"hash_sphere_trace": 1, "hash_sdf_fwd_raw": 0, "hash_encode_fwd_raw": 0}
    net.hash_fused = False
    depth0, mask0, nrm0 = US.render_depth(net, R, t, cam, normals=True, **kw)
    net.hash_fused = True
    assert calls["hash_sphere_trace"] == 1 and calls["hash_encode_fwd_raw"] > 0
    assert tuple(depth.shape) == (24, 32) and tuple(nrm.shape) == (24, 32, 3) and mask.dtype == torch.bool
    # the two routes differ by the decoder's arithmetic: tests/test_hash_sdf_routing.py's level on the field
    with torch.no_grad():
        field = float(net(o + torch.rand(o.shape[0], 1, device=DEV) * dw).abs().max())
    tol = 2e-6 * max(1.0, field)
    assert float((mask != mask0).float().mean()) <= 0.01
    both = mask & mask0
    assert bool(both.all())                                                   # (this view: every pixel sees the plane)
    assert float((depth - depth0)[both].abs().max()) <= tol
    # z-depth of a plane seen along its normal; a ray stops less than epsilon above it
    assert float((depth[both] - (VIEW["eye"][2] - PLANE_Z)).abs().max()) <= 1.1 * EPS
    # normals: central differences with step h of two fields `tol` apart differ by at most 2 tol / (2 h)
    up = torch.tensor([0.0, 0.0, 1.0], device=DEV)
    assert float((nrm[both] - up).abs().max()) <= 1e-4 and float((nrm - nrm0)[both].abs().max()) <= tol / 1e-2
