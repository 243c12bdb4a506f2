"""Sphere tracing (utils_sdf.sphere_tracing, render_depth; miso_atlas_sphere_trace, csrc/trace.hip) against
  * the reference's own sphere_tracing on the reference's GridNet, fp32 and fp64 (tests/golden/sphere_trace.npz, written
    by tools/make_goldens.py from the inputs of tests/sphere_trace_cases.py),
  * the Python loop of this package over model(points): the one-launch kernel gives its points, mask, field values and
    step counts bit for bit, for every covered decoder form and ray counts around the 64-ray wavefront,
  * itself: a ray's result does not depend on the rays it shares a wavefront with,
  * diff.gradient3d (the normals) and the analytic scene (the depth image)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import golden_cases as gc
import sphere_trace_cases as stc
from test_grid_opt_mirror import G, T, make_atlas, make_gridnet

DEV = "cuda:0"


def scene_net(dev):
    from miso_amd.grid_opt.models.grid_net import GridNet
    return stc.bake(GridNet(stc.model_cfg(), device=dev)).to(dev)


def check_against_golden(points, mask, iters):
    """Masks equal the reference's fp32 masks outside `marginal`; every point within epsilon + 4 dev32 of the reference's
    fp64 point: a stop decision that flips moves a point by one step of at most ~epsilon, a second fp32 evaluation of the
    same sequence deviates from fp64 by about what the reference's own fp32 did (x4: the <= 2x admissibility margin of
    test_split_precision.py on each side)."""
    g = G("sphere_trace")
    marginal = g[f"marginal_{iters}"].reshape(-1)
    mask = mask.cpu().numpy()
    assert mask.shape == g[f"mask32_{iters}"].shape and mask.dtype == np.bool_
    # (the fixture is worth its name: half of the rays hit and half go far in the long runs, none has hit in the short)
    assert g["mask32_100"].sum() * 2 == mask.size and not g["mask32_1"].any() and not g["marginal_100"].all()
    assert np.array_equal(mask.reshape(-1)[~marginal], g[f"mask32_{iters}"].reshape(-1)[~marginal])
    err = np.abs(points.cpu().numpy().astype(np.float64) - g[f"points64_{iters}"])
    bound = stc.TRACE["epsilon"] + 4.0 * float(g[f"dev32_{iters}"])
    print(f"max_iters={iters}: max|p - p64| = {err.max():.3e} (bound {bound:.3e})")
    assert err.max() <= bound


def test_loop_matches_reference_golden(device_backend):
    import miso_amd.grid_opt.utils.utils_sdf as US
    dev = device_backend
    net = scene_net(dev)
    o, d = (T(a).to(dev) for a in stc.golden_rays())
    for iters in stc.RUNS:
        with torch.no_grad():
            points, mask = US.sphere_tracing(lambda p: net(p), o, d, max_iters=iters, **stc.TRACE)   # a lambda: the loop
        check_against_golden(points, mask, iters)


@pytest.mark.gpu
def test_fused_trace_matches_reference_golden():
    import miso_amd.grid_opt.utils.utils_sdf as US
    net = scene_net(DEV)
    o, d = (T(a).to(DEV) for a in stc.golden_rays())
    calls = []
    fused = net.sphere_trace
    net.sphere_trace = lambda *a, **k: calls.append(1) or fused(*a, **k)
    for iters in stc.RUNS:
        with torch.no_grad():
            got = fused(o, d, max_iters=iters, **stc.TRACE)
            assert got is not None, "the fused trace was not taken"
            check_against_golden(got[0], got[1], iters)
            n = len(calls)
            points, mask = US.sphere_tracing(net, o, d, max_iters=iters, **stc.TRACE)
            assert len(calls) == n + 1, "sphere_tracing(model, ...) did not go through model.sphere_trace"
            check_against_golden(points, mask, iters)
            points, mask = US.sphere_tracing(net.forward, o, d, max_iters=iters, **stc.TRACE)     # a bound method too
            assert len(calls) == n + 2
            check_against_golden(points, mask, iters)


# --------------------------------------------------------------------------------------------------------------------
# the kernel is the loop, bit for bit
# --------------------------------------------------------------------------------------------------------------------
def _three_submaps(C, L, H):
    """the three overlapping submaps of test_atlas_fused.py::test_fused_atlas_query_other_shapes_vs_the_loop"""
    from miso_amd.grid_opt.models.grid_atlas import GridAtlas
    cfg = {"name": "grid_net", "spatial_dim": 3,
           "decoder": {"type": "mlp", "hidden_dim": H, "hidden_layers": 1, "out_dim": 1, "pos_invariant": True,
                       "fix": True, "pretrained_model": None},
           "grid": {"type": "regular", "feature_dim": C, "init_stddev": 3e-2, "bound": [[-1.0, 1.0], [-0.5, 0.75], [-1.0, 1.0]],
                    "base_cell_size": 0.25, "per_level_scale": 2, "n_levels": L},
           "pose": {"optimize": False, "num_poses": 1}}
    torch.manual_seed(3)
    atlas = GridAtlas(cfg, device=DEV)
    lb = torch.tensor(cfg["grid"]["bound"])
    for s, (tx, ang) in enumerate(((0.0, 0.0), (1.2, 0.3), (-0.8, -1.1))):
        Rz = torch.tensor([[math.cos(ang), -math.sin(ang), 0.0], [math.sin(ang), math.cos(ang), 0.0], [0.0, 0.0, 1.0]])
        atlas.add_submap(lb, Rz, torch.tensor([[tx], [0.1 * s], [-0.2 * s]]), num_poses=1)
        atlas.add_kf(torch.eye(3), torch.zeros(3, 1))
    return atlas.to(DEV)


def _model(name):
    """-> (model, (3,2) bound the rays start in, margin around it, the decoder's last linear)"""
    if name == "golden_atlas":
        m = make_atlas(DEV)
    elif name.startswith("atlas"):
        m = _three_submaps(*(int(v) for v in name.split("_")[1:]))
    else:
        m = make_gridnet(gc.CASES["cfg2"], DEV)
        if name == "gridnet_ignore1":
            m.ignore_level(1)
        return m, m.bound.detach().cpu(), 0.1, m.decoder.linears()[-1]
    return m, m.global_bound(device="cpu").detach(), 0.3, m.submaps[0].decoder.linears()[-1]


def _rays(bound, margin, n, seed):
    gen = torch.Generator().manual_seed(seed)
    lo, hi = bound[:, 0] - margin, bound[:, 1] + margin
    o = lo + (hi - lo) * torch.rand(n, 3, generator=gen)
    d = torch.randn(n, 3, generator=gen) * (0.5 + torch.rand(n, 1, generator=gen))       # random, not unit length
    return o.to(DEV), d.to(DEV)


def _recorded_loop(model, o, d, **kw):
    """utils_sdf.sphere_tracing over a lambda (the Python loop) with every query logged.
    -> points, mask, dists (iterations, N), steps (N) the iterations in which a ray moved, moving (N) at the cut-off"""
    import miso_amd.grid_opt.utils.utils_sdf as US
    log = []

    def query(p):
        s = model(p)
        log.append((p, s))
        return s

    points, mask = US.sphere_tracing(lambda p: query(p), o, d, **kw)
    dists = torch.stack([torch.norm(p - o, dim=1, keepdim=True) for p, _ in log])
    stop = torch.stack([s < kw["epsilon"] for _, s in log]) | (dists > kw["max_dist"])
    return points, mask, dists[..., 0], (~stop).sum(dim=0).reshape(-1).to(torch.int32), ~stop[-1].reshape(-1)


def _gap(values, lo, hi):
    """the middle of the widest gap between neighbouring distinct `values` inside [lo, hi]"""
    v = torch.unique(values.reshape(-1).double().cpu())
    v = v[(v >= lo) & (v <= hi)]
    k = int(torch.argmax(v[1:] - v[:-1]))
    return float((v[k] + v[k + 1]) / 2)


def _shift_for(field, share, eps):
    """the largest field value that, taken off the decoder's output bias, leaves at most `share` of `field` below eps
    (the points inside no submap all see the one value of the zero row: a quantile may land on it)"""
    fs = torch.sort(field.reshape(-1)).values
    below = torch.searchsorted(fs, fs + eps)                      # how many values end up below eps with shift = fs[k]
    k = int((below <= share * fs.numel()).sum()) - 1
    return fs[max(k, 0)].reshape(1).clone()


MODELS = ["golden_atlas", "atlas_8_3_64", "atlas_4_1_32", "atlas_8_4_64", "gridnet", "gridnet_ignore1"]
ITERS, EPS = 16, 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["split", "exact"])
@pytest.mark.parametrize("name", MODELS)
def test_fused_trace_is_the_loop_bit_for_bit(name, form):
    import contextlib
    from miso_amd import ops
    model, bound, margin, last = _model(name)
    o, d = _rays(bound, margin, 1000, seed=len(name))
    with torch.no_grad(), (ops.exact_fp32() if form == "exact" else contextlib.nullcontext()):
        # random features: shift the decoder's output bias so that the field is positive at three quarters of the origins
        shift = _shift_for(model(o), 0.25, EPS)
        last.bias -= shift
        try:
            # max_dist: what the farthest 7 - 20 % of the rays reach, in the widest gap between the distances the loop
            # sees there, so that the far test cannot hinge on the last bit of a norm
            free = dict(min_dist=1e-3, max_dist=float("inf"), max_iters=ITERS, epsilon=EPS)
            _, _, dists, _, _ = _recorded_loop(model, o, d, **free)
            q = torch.quantile(dists[-1], torch.tensor([0.80, 0.93], device=DEV))
            kw = dict(free, max_dist=_gap(dists, float(q[0]), float(q[1])))
            points, mask, dists, steps, moving = _recorded_loop(model, o, d, **kw)
            # preconditions, on the loop's own record
            conv = mask.reshape(-1)
            far = ~conv & ~moving
            shares = [float(v.float().mean()) for v in (conv, far, moving)]
            print(f"{name} {form}: max_dist {kw['max_dist']:.4f}, converged / far / moving {shares}")
            assert min(shares) >= 0.05, shares
            assert float((dists - kw["max_dist"]).abs().min()) >= 1e-5
            for n in (1, 63, 64, 65, 1000):
                if n < 1000:
                    p_n, m_n, _, s_n, _ = _recorded_loop(model, o[:n], d[:n], **kw)
                else:
                    p_n, m_n, s_n = points, mask, steps
                got = model.sphere_trace(o[:n], d[:n], want_sdf=True, want_steps=True, **kw)
                assert got is not None, "the fused trace was not taken"
                fp, fm, extras = got
                assert fm.dtype == torch.bool and tuple(fm.shape) == (n, 1)
                assert torch.equal(fp, p_n), f"n={n}: points differ on {int((fp != p_n).any(dim=1).sum())} rays"
                assert torch.equal(fm, m_n), f"n={n}: masks differ on {int((fm != m_n).sum())} rays"
                assert torch.equal(extras["sdf"], model(fp)), f"n={n}"
                assert torch.equal(extras["steps"], s_n), f"n={n}"
        finally:
            last.bias += shift


@pytest.mark.gpu
def test_rays_do_not_depend_on_their_wavefront():
    model, bound, margin, last = _model("golden_atlas")
    o, d = _rays(bound, margin, 1000, seed=5)
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(17)).to(DEV)
    with torch.no_grad():
        shift = _shift_for(model(o), 0.25, EPS)
        last.bias -= shift
        try:
            kw = dict(min_dist=1e-3, max_dist=0.4, max_iters=ITERS, epsilon=EPS, want_sdf=True, want_steps=True, grad_step=1e-2)
            p, m, e = model.sphere_trace(o, d, **kw)
            pp, mp, ep = model.sphere_trace(o[perm], d[perm], **kw)
        finally:
            last.bias += shift
    assert 0 < int(m.sum()) < 1000 and int(e["steps"].min()) < int(e["steps"].max())
    assert torch.equal(pp, p[perm]) and torch.equal(mp, m[perm])
    for k in ("sdf", "steps", "grad"):
        assert torch.equal(ep[k], e[k][perm]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["golden_atlas", "gridnet"])
def test_normals(name):
    """grad = diff.gradient3d(points, model, 'finitediff', h): the six field values are the same bits, only the final
    scaling may round differently (a division here, a product with the reciprocal there)."""
    from miso_amd.grid_opt import diff
    model, bound, margin, _ = _model(name)
    o, d = _rays(bound, margin, 777, seed=9)
    h = 1e-2
    with torch.no_grad():
        points, _, extras = model.sphere_trace(o, d, max_dist=0.5, max_iters=8, epsilon=EPS, grad_step=h)
        ref = diff.gradient3d(points, model, 'finitediff', h)
    assert float(ref.abs().max()) > 0
    torch.testing.assert_close(extras["grad"], ref, rtol=5e-7, atol=0)


@pytest.mark.gpu
def test_rendered_normals_are_unit_where_hit():
    import miso_amd.grid_opt.utils.utils_sdf as US
    from miso_amd.grid_opt.utils.utils_data import CameraParameters
    net = scene_net(DEV)
    c = stc.VIEW
    R, t = stc.camera_pose(c)
    cam = CameraParameters(c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"])
    depth, mask, nrm = US.render_depth(net, T(R), T(t), cam, max_dist=stc.TRACE["max_dist"], normals=True,
                                       epsilon=stc.TRACE["epsilon"])
    assert tuple(nrm.shape) == (c["H"], c["W"], 3) and 0 < int(mask.sum()) < mask.numel()
    assert float((nrm[mask].norm(dim=-1) - 1).abs().max()) < 1e-5
    assert float(nrm[~mask].abs().max()) == 0.0
    # the floor's normal points up, at the camera
    floor = mask & (depth > 0) & (nrm[..., 1] > 0.99)
    assert int(floor.sum()) > 20


def test_render_depth_of_the_golden_scene(device_backend):
    import miso_amd.grid_opt.utils.utils_sdf as US
    import miso_amd.grid_opt.utils.utils_sample as USA
    from miso_amd.grid_opt.utils.utils_data import CameraParameters
    dev = device_backend
    net = scene_net(dev)
    c, tr = stc.VIEW, stc.TRACE
    R, t = stc.camera_pose(c)
    cam = CameraParameters(c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"])
    kw = dict(max_dist=tr["max_dist"], min_dist=tr["min_dist"], epsilon=tr["epsilon"], max_iters=100)
    depth, mask = US.render_depth(net, T(R), T(t), cam, **kw)
    assert tuple(depth.shape) == (c["H"], c["W"]) and tuple(mask.shape) == (c["H"], c["W"]) and mask.dtype == torch.bool
    hit = mask.cpu().numpy()
    assert 100 < hit.sum() < hit.size - 100
    # against the analytic scene's ray-surface distance (float64), as z-depth; the field is a trilinear interpolant of
    # the scene: epsilon + base cell
    o, dw = stc.rays(c)
    length = np.linalg.norm(dw.astype(np.float64), axis=1)
    z_true = (stc.scene_ray_distance(o, dw / length[:, None]) / length).reshape(c["H"], c["W"])
    z = depth.cpu().numpy().astype(np.float64)
    err = np.abs(z - z_true)[hit]
    print(f"{int(hit.sum())} of {hit.size} pixels hit; max |z - z_true| = {err.max():.4f}")
    assert err.max() <= tr["epsilon"] + stc.GRID["base_cell"]
    assert np.all(z[~hit] == 0.0)
    # row-major (H,W) as pointcloud_from_depth_torch reads it: back-projecting the depth returns the traced points
    with torch.no_grad():
        query = net if dev != "cpu" else (lambda p: net(p))
        points, m2 = US.sphere_tracing(query, T(o).to(dev), T(dw).to(dev), **kw)
    assert torch.equal(m2.reshape(c["H"], c["W"]), mask)
    pc = USA.pointcloud_from_depth_torch(depth, c["fx"], c["fy"], c["cx"], c["cy"])
    world = pc.reshape(-1, 3) @ T(R).float().to(dev).T + T(t).float().to(dev)
    sel = mask.reshape(-1)
    assert float((world[sel] - points[sel]).abs().max()) <= 1e-5


def test_trace_refuses_malformed_calls():
    """Every BADARG case of miso_atlas_sphere_trace, before any launch (null or host pointers only); max_iters = 0 in
    Python; no fused trace with autograd on or with host tensors."""
    import miso_amd.grid_opt.utils.utils_sdf as US
    from miso_amd import _lib
    lib = _lib.load()
    E = _lib.E_BADARG
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    ptr = ctypes.c_void_p((base + 15) // 16 * 16)                  # a host address: never dereferenced by a refused call
    g = _lib.Grid()
    g.n_levels = 1
    g.level[0].C = 4; g.level[0].X = 2; g.level[0].Y = 2; g.level[0].Z = 2
    g.level[0].sC = 1; g.level[0].sX = 4; g.level[0].sY = 8; g.level[0].sZ = 16
    m = _lib.Mlp()
    m.in_dim, m.hidden_dim, m.out_dim, m.n_linear = 4, 32, 1, 3
    # a well-formed call of zero rays: MISO_OK with nothing launched -- so each refusal below is due to its one change
    good = dict(plan=ptr, n_submaps=1, shape=ctypes.byref(g), poses=ptr, mlp=ctypes.byref(m), packed=ptr, origins=ptr,
                dirs=ptr, n_rays=0, min_dist=1e-3, max_dist=1.0, max_iters=10, epsilon=1e-4, fd_step=0.0, points=ptr,
                hit=ptr, sdf=None, steps=None, grad=None, flags=0, stream=None)

    def call(**over):
        return lib.miso_atlas_sphere_trace(*{**good, **over}.values())

    assert call() == 0
    assert call(flags=_lib.F_EXACT_F32 | _lib.F_ATLAS_NO_BOUND, grad=ptr, fd_step=1e-2, sdf=ptr, steps=ptr) == 0
    for name in ("plan", "shape", "poses", "mlp", "packed", "origins", "dirs", "points", "hit"):
        assert call(**{name: None}) == E, name
    assert call(n_rays=-1) == E
    assert call(max_iters=0) == E
    assert call(n_submaps=0) == E
    assert call(grad=ptr, fd_step=0.0) == E
    assert call(grad=ptr, fd_step=float("nan")) == E
    assert call(flags=1 << 20) == E
    assert call(flags=_lib.F_CROWDED) == E                          # a flag of another entry point
    assert call(packed=ctypes.c_void_p(ptr.value + 4)) == E          # misaligned weight pack
    m.hidden_dim = 48                                               # a decoder outside the fused table
    assert call() == _lib.E_UNSUPPORTED
    m.hidden_dim = 32

    net = scene_net("cpu")
    o, d = (T(a) for a in stc.golden_rays())
    with pytest.raises(ValueError):
        US.sphere_tracing(lambda p: p[:, :1], o, d, max_iters=0)
    with torch.no_grad():
        assert net.sphere_trace(o, d) is None                      # host tensors
    assert net.sphere_trace(o, d) is None                          # autograd on
    from miso_amd.grid_opt.models.grid_atlas import GridAtlas
    atlas = GridAtlas(stc.model_cfg(), device="cpu")
    atlas.add_submap(torch.tensor(stc.GRID["bound"]), torch.eye(3), torch.zeros(3, 1), num_poses=1)
    atlas.add_kf(torch.eye(3), torch.zeros(3, 1))
    with torch.no_grad():
        assert atlas.sphere_trace(o, d) is None
    assert atlas.sphere_trace(o, d) is None
    if torch.cuda.is_available():
        net = net.to(DEV)
        assert net.sphere_trace(o.to(DEV), d.to(DEV)) is None       # autograd on, device tensors
        with torch.no_grad(), pytest.raises(ValueError):
            net.sphere_trace(o.to(DEV), d.to(DEV), max_iters=0)
        with torch.no_grad():                                       # no rays: empty results, nothing launched
            e = torch.empty(0, 3, device=DEV)
            points, mask = US.sphere_tracing(net, e, e)
            assert tuple(points.shape) == (0, 3) and tuple(mask.shape) == (0, 1) and mask.dtype == torch.bool
