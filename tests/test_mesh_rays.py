"""Ray casting against a mesh on the GPU (csrc/mesh.hip: ops.MeshIndex / cast_rays_all / cast_rays), and what is built on
it: utils_sdf.render_mesh_depth, datasets.sdf_3d.PosedSdf3D, mesh depth frames into PosedSdfRgbd.

The grid route and the all-triangles route agree bit for bit on every fixture of tests/mesh_cases.py at two cell sizes;
both are the float64 first hit on the well-conditioned rays within mesh_cases.T_TOL (exact on `lattice`); ties go to
the lowest triangle index; NaN rays and NaN triangles never match; out= buffers, strided views, a side stream and a
replayed graph return the eager bits."""
import numpy as np
import pytest
import torch

import mesh_cases as mc

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_results = {}


def _run(name):
    """{'all': (t, tri), cell: (t, tri, index stats, walk stats)} of a fixture as numpy arrays, computed once"""
    if name not in _results:
        from miso_amd import ops
        fx = mc.fixture(name)
        V, T, O, D = (_dev(fx[k]) for k in ("vertices", "triangles", "origins", "dirs"))
        out = {"all": tuple(x.cpu().numpy() for x in ops.cast_rays_all(O, D, V, T))}
        for cell in fx["cells"]:
            ix = ops.MeshIndex(V, T, cell=cell)
            walk = torch.zeros(3, dtype=torch.int64, device="cuda")
            t, tri = ix.cast_rays(O, D, stats=walk)
            out[cell] = (t.cpu().numpy(), tri.cpu().numpy(), ix.stats(), walk.cpu().numpy())
        _results[name] = out
    return _results[name]


def _same(a, b):
    return bool((a[0].view(np.int32) == b[0].view(np.int32)).all() and (a[1] == b[1]).all())


# --------------------------------------------------------------------------- 1. the two routes
@pytest.mark.parametrize("name", list(mc.FIXTURES))
def test_grid_route_and_all_triangles_route_agree_bit_for_bit(name):
    fx, got = mc.fixture(name), _run(name)
    n = len(fx["origins"])
    small, large = fx["cells"]
    for cell in (small, large):
        t, tri, stats, walk = got[cell]
        assert t.shape == (n,) and tri.shape == (n,) and t.dtype == np.float32 and tri.dtype == np.int64
        assert _same((t, tri), got["all"]), (name, cell)
        assert stats["cell"] == pytest.approx(cell) and stats["entries"] >= int(mc.hittable(fx["vertices"], fx["triangles"]).sum())
        assert walk[2] == 0                                    # every ray of the fixtures is inside the walk's guarantee
    # the small cell forces long walks, the large one puts everything in a few cells
    assert got[small][3][0] > got[large][3][0] and got[small][2]["cells"] > 5 * got[large][2]["cells"]
    assert got[large][2]["cells"] <= 400


def test_a_huge_slanted_triangle_is_not_listed_in_its_whole_box():
    """`sliver` at its small cell: the triangle across the grid's diagonal has 86 x 86 x 58 = 429 000 box cells; the
    plane-slab test keeps its list entries near the cells its plane crosses."""
    stats = _run("sliver")[0.07][2]
    assert stats["dims"] == (86, 86, 58) and stats["entries"] < 40000


# --------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("name", list(mc.FIXTURES))
def test_answer_is_the_float64_first_hit(name):
    fx, got = mc.fixture(name), _run(name)
    ref, kept = fx["ref"], fx["kept"]
    t, tri = got["all"]
    assert ((tri >= 0) == (ref["tri"] >= 0))[kept].all()                           # hit / miss agrees
    hit = kept & (tri >= 0)
    e = mc.t_error(fx, t)
    print(f"{name}: max e over kept rays {np.nanmax(e[hit], initial=0.0):.3e} (T_TOL {mc.T_TOL:.3e}), "
          f"triangle differs on {int((tri != ref['tri'])[hit].sum())}")
    assert (e[hit] <= mc.T_TOL).all()
    # the float64 winner, or a triangle whose own t64 is within the tolerance of it
    other = np.nonzero(hit & (tri != ref["tri"]))[0]
    for r, k in zip(other, tri[other]):
        one = mc.oracle(fx["origins"][r:r + 1], fx["dirs"][r:r + 1], fx["vertices"], fx["triangles"][k:k + 1])
        assert one["tri"][0] == 0
        dn = np.linalg.norm(fx["dirs"][r].astype(np.float64))
        assert abs(one["t"][0] - ref["t"][r]) * dn <= mc.T_TOL * (fx["coord_max"] + ref["t"][r] * dn)
    if name == "lattice":
        assert (t.astype(np.float64) == ref["t"]).all() and (tri == ref["tri"]).all()


# --------------------------------------------------------------------------- 3, 4. ties, misses, NaN
def test_ties_misses_and_non_finite_inputs():
    from miso_amd import ops
    fx, got = mc.fixture("lattice"), _run("lattice")
    assert (got["all"][1] == fx["ref"]["tri"]).all()                                # the lowest index of every tie
    miss = fx["ref"]["tri"] < 0
    assert miss.any() and np.isposinf(got["all"][0][miss]).all() and (got["all"][1][miss] == -1).all()
    # NaN / inf triangles, zero-area triangles and the later copy of a duplicate are never returned
    fs, gs = mc.fixture("sliver"), _run("sliver")
    dead = np.nonzero(~mc.hittable(fs["vertices"], fs["triangles"]))[0]
    for key in ("all",) + fs["cells"]:
        assert not np.isin(gs[key][1], dead).any() and not np.isin(gs[key][1], np.arange(501, 521)).any()
    # NaN / inf origins, a NaN direction, a zero direction: (+inf, -1) from both routes; a far origin: the same bits
    fr = mc.fixture("room")
    V, T = _dev(fr["vertices"]), _dev(fr["triangles"])
    O, D = fr["origins"][:64].copy(), fr["dirs"][:64].copy()
    O[0, 0], O[1, 2], D[2, 1], D[3] = np.nan, np.inf, np.nan, 0.0
    O[4] = (4.0e4, 3.0, 1.5)                                                        # beyond 4 coord_mag: answered from all rows
    D[4] = (-1.0, 0.0, 0.0)
    D[5, 0] = 1e-42                                                                 # a reciprocal that overflows
    ix = ops.MeshIndex(V, T, cell=0.5)
    walk = torch.zeros(3, dtype=torch.int64, device="cuda")
    t, tri = ix.cast_rays(_dev(O), _dev(D), stats=walk)
    ta, ia = ops.cast_rays_all(_dev(O), _dev(D), V, T)
    t, tri, ta, ia = (x.cpu().numpy() for x in (t, tri, ta, ia))
    assert _same((t, tri), (ta, ia))
    assert np.isposinf(t[:4]).all() and (tri[:4] == -1).all()
    assert tri[4] >= 0 and abs(t[4] - (4.0e4 - 8.0)) < 1.0 and tri[5] >= 0
    assert int(walk.cpu()[2]) == 5                                                  # rays 0, 1, 2, 4 and 5 left the walk
    want = mc.oracle(O[6:], D[6:], fr["vertices"], fr["triangles"])
    assert (tri[6:] == want["tri"])[fr["kept"][6:64]].all()


# --------------------------------------------------------------------------- edge cases of the call
def test_edge_cases_of_the_call():
    from miso_amd import ops
    fr = mc.fixture("room")
    V, T, O, D = (_dev(fr[k]) for k in ("vertices", "triangles", "origins", "dirs"))
    none_v, none_t = torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int64, device="cuda")
    # an empty mesh
    ix = ops.MeshIndex(none_v, none_t)
    for t, tri in (ix.cast_rays(O[:100], D[:100]), ops.cast_rays_all(O[:100], D[:100], none_v, none_t)):
        assert torch.isposinf(t).all() and (tri == -1).all()
    assert ix.stats()["entries"] == 0
    # zero rays
    full = ops.MeshIndex(V, T, cell=0.5)
    t, tri = full.cast_rays(O[:0], D[:0])
    assert t.shape == (0,) and tri.shape == (0,)
    assert ops.cast_rays_all(O[:0], D[:0], V, T)[0].shape == (0,)
    # one triangle; a mesh of nothing but dead triangles
    one_v = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]], device="cuda")
    one_t = torch.tensor([[0, 1, 2]], device="cuda")
    o = torch.tensor([[0.25, 0.25, 0.0], [0.75, 0.75, 0.0], [0.25, 0.25, 2.0]], device="cuda")
    d = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [0.0, 0.0, -1.0]], device="cuda")
    for t, tri in (ops.MeshIndex(one_v, one_t).cast_rays(o, d), ops.cast_rays_all(o, d, one_v, one_t)):
        assert t.tolist() == [0.5, float("inf"), 1.0] and tri.tolist() == [0, -1, 0]      # t in units of |d|
    dead = ops.MeshIndex(one_v, torch.tensor([[0, 0, 1], [0, 1, 7]], device="cuda"))          # zero area; an index out of range
    assert dead.stats()["entries"] == 0 and (dead.cast_rays(o, d)[1] == -1).all()
    assert (ops.cast_rays_all(o, d, one_v, torch.tensor([[0, 0, 1], [0, 1, 7]], device="cuda"))[1] == -1).all()
    # a t window that hides the nearest hit
    ref = fr["ref"]
    lo = float(np.median(ref["t"]))
    want = mc.oracle(fr["origins"], fr["dirs"], fr["vertices"], fr["triangles"], t_min=np.float32(lo), t_max=np.float32(2 * lo))
    tw, iw = full.cast_rays(O, D, t_min=lo, t_max=2 * lo)
    ta, ia = ops.cast_rays_all(O, D, V, T, t_min=lo, t_max=2 * lo)
    assert _same((tw.cpu().numpy(), iw.cpu().numpy()), (ta.cpu().numpy(), ia.cpu().numpy()))
    k = fr["kept"] & mc.kept_rays(fr["origins"], fr["dirs"], fr["vertices"], fr["triangles"], want["t"])
    edge = np.abs(ref["t"] / lo - 1.0) < 1e-5                                          # a first hit on the window's border
    assert (iw.cpu().numpy() == want["tri"])[k & ~edge].all() and (iw.cpu().numpy() != ref["tri"]).sum() > 1000
    # ray counts around a wavefront and a block, against the full run
    base = _run("room")["all"]
    for n in (1, 63, 64, 65, 255, 256, 257):
        for t, tri in (full.cast_rays(O[:n], D[:n]), ops.cast_rays_all(O[:n], D[:n], V, T)):
            assert _same((t.cpu().numpy(), tri.cpu().numpy()), (base[0][:n], base[1][:n])), n
    # more triangles than one LDS tile of the all-triangles kernel (512): room twice over and then some
    rng = np.random.default_rng(1)
    extra = mc.small_triangles(rng, 72, (0.5, 0.5, 1.2), (7.5, 5.5, 2.8), 0.05)
    v3, t3 = mc.join([(fr["vertices"], fr["triangles"]), (fr["vertices"] + np.float32(0.01), fr["triangles"]), extra])
    assert len(t3) == 3000
    V3, T3 = _dev(v3.astype(np.float32)), _dev(t3)
    a = ops.cast_rays_all(O[:1024], D[:1024], V3, T3)
    b = ops.MeshIndex(V3, T3, cell=0.3).cast_rays(O[:1024], D[:1024])
    assert _same(tuple(x.cpu().numpy() for x in a), tuple(x.cpu().numpy() for x in b))
    want = mc.oracle(fr["origins"][:1024], fr["dirs"][:1024], v3.astype(np.float32), t3)
    k3 = mc.kept_rays(fr["origins"][:1024], fr["dirs"][:1024], v3.astype(np.float32), t3, want["t"])
    assert (a[1].cpu().numpy() == want["tri"])[k3].all() and (want["tri"] >= 1464).sum() > 100


# --------------------------------------------------------------------------- 5. buffers, views, streams, graphs
def test_out_buffers_strided_views_a_side_stream_and_a_replayed_graph_return_the_eager_bits():
    """The build reads the bounds and the entry count back, so it stays outside the capture; the query replays."""
    from miso_amd import ops
    fx = mc.fixture("room")
    want = _run("room")["all"]
    n = len(fx["origins"])
    V, T, O, D = (_dev(fx[k]) for k in ("vertices", "triangles", "origins", "dirs"))

    def same(t, tri):
        torch.cuda.synchronize()
        return _same((t[:n].cpu().numpy(), tri[:n].cpu().numpy()), want)

    # strided views are read in place
    V4 = torch.full((len(fx["vertices"]), 4), 9.0, device="cuda")
    T5 = torch.full((len(fx["triangles"]), 5), -3, dtype=torch.int64, device="cuda")
    R8 = torch.full((n, 8), 5.0, device="cuda")
    V4[:, :3], T5[:, 1:4], R8[:, :3], R8[:, 4:7] = V, T, O, D
    ix = ops.MeshIndex(V4[:, :3], T5[:, 1:4], cell=0.4)
    assert ix.vertices.data_ptr() == V4.data_ptr() and ix.triangles.data_ptr() == T5[:, 1:4].data_ptr()
    assert same(*ix.cast_rays(R8[:, :3], R8[:, 4:7]))
    assert same(*ops.cast_rays_all(R8[:, :3], R8[:, 4:7], V4[:, :3], T5[:, 1:4]))
    # out= buffers (larger than needed), a second call
    out = (torch.zeros(n + 7, device="cuda"), torch.zeros(n + 7, device="cuda", dtype=torch.int64))
    got = ix.cast_rays(O, D, out=out)
    assert got[0] is out[0] and got[1] is out[1] and same(*out) and same(*ix.cast_rays(O, D))
    oa = (torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda", dtype=torch.int64))
    ops.cast_rays_all(O, D, V, T, out=oa)
    assert same(*oa)
    # a side stream: build and query there
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = ops.MeshIndex(V, T, cell=0.4).cast_rays(O, D)
    side.synchronize()
    assert same(*res)
    # a captured graph replays the query
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ix.cast_rays(O, D, out=out)
    for _ in range(2):
        for x in out:
            x.zero_()
        graph.replay()
        assert same(*out)


# --------------------------------------------------------------------------- 6. the route picked by size
def test_cast_rays_picks_a_route_by_size_and_both_give_the_same_bits(monkeypatch):
    from miso_amd import ops
    fx = mc.fixture("open")
    want = _run("open")["all"]
    V, T, O, D = (_dev(fx[k]) for k in ("vertices", "triangles", "origins", "dirs"))
    built = []
    real = ops.MeshIndex

    class Spy(real):
        def __init__(self, *a, **k):
            built.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(ops, "MeshIndex", Spy)
    nt = len(fx["triangles"])
    monkeypatch.setattr(ops, "MESH_ALL_BELOW", nt + 1)
    small = ops.cast_rays(O, D, V, T)
    assert not built
    monkeypatch.setattr(ops, "MESH_ALL_BELOW", nt)
    large = ops.cast_rays(O, D, V, T)
    assert built == [1]
    for t, tri in (small, large):
        assert _same((t.cpu().numpy(), tri.cpu().numpy()), want)


# --------------------------------------------------------------------------- 7. render_mesh_depth
def test_render_mesh_depth_on_room():
    import test_mesh_host as host
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_sdf
    from miso_amd.grid_opt.utils.utils_geometry import cast_rays_torch
    from miso_amd.grid_opt.utils.utils_sample import ray_dirs_C
    fx = mc.fixture("room")
    V, T = _dev(fx["vertices"]), _dev(fx["triangles"])
    ix = ops.MeshIndex(V, T)
    cam = host._camera()
    R, t = host._pose(35.0, 12.0, (3.0, 2.0, 1.9))
    R, t = torch.tensor(R, dtype=torch.float32, device="cuda"), torch.tensor(t, dtype=torch.float32, device="cuda")
    depth, mask, nrm = utils_sdf.render_mesh_depth(ix, R, t, cam, normals=True)
    assert depth.shape == (48, 64) and depth.is_cuda and mask.dtype == torch.bool and nrm.shape == (48, 64, 3)
    dirs = ray_dirs_C(1, 48, 64, cam.fx, cam.fy, cam.cx, cam.cy, "cuda", "z").reshape(-1, 3) @ R.T
    tt, tri = cast_rays_torch(t.reshape(1, 3).expand(48 * 64, 3), dirs, V, T, chunk=1024)
    hit = tri >= 0
    assert hit.float().mean() > 0.99 and (mask.reshape(-1) == hit).all()
    # the same formula on the same device: equal up to the fused multiply-adds torch's kernels may contract
    print(f"render_mesh_depth vs cast_rays_torch on the device: max |dt| {(depth.reshape(-1) - tt)[hit].abs().max().item():.3e}")
    assert torch.allclose(depth.reshape(-1)[hit], tt[hit], rtol=4 * mc.T_TOL, atol=0) and (depth.reshape(-1)[~hit] == 0).all()
    _, tri_k = ix.cast_rays(t.reshape(1, 3).expand(48 * 64, 3).contiguous(), dirs)
    want = ix.triangle_normals()[tri_k.clamp(min=0)]
    want = torch.where(hit[:, None], want, torch.zeros_like(want))
    assert torch.allclose(nrm.reshape(-1, 3), want, atol=1e-6)
    assert torch.allclose(nrm.reshape(-1, 3)[hit].norm(dim=1), torch.ones(int(hit.sum()), device="cuda"), atol=1e-5)
    # a TriangleMesh goes the same way as the index
    mesh = utils_sdf.TriangleMesh(fx["vertices"], fx["triangles"])
    d2, m2 = utils_sdf.render_mesh_depth(mesh, R, t, cam)
    assert torch.equal(d2, depth) and torch.equal(m2, mask)


# --------------------------------------------------------------------------- 8. PosedSdf3D on the device
def test_posed_sdf_3d_on_the_device_matches_its_cpu_route():
    import test_mesh_host as host
    from miso_amd.grid_opt.datasets.sdf_3d import PosedSdf3D
    from miso_amd.grid_opt.utils import utils_sdf
    mesh = utils_sdf.box_mesh(host.ROOM)
    kw = dict(frame_batchsize=128, frame_samples=256, near_surface_n=2, free_space_n=1, trunc_dist=0.15,
              frame_poses=host.posed_sdf_3d_poses(), width_px=64, height_px=48)
    np.random.seed(4)
    dev = PosedSdf3D(mesh, device="cuda:0", **kw)
    host.check_posed_sdf_3d(dev, 3, 256, 2, 1, 0.15, tol=mc.T_TOL * 20.0)
    assert dev.frames[0]["points_frame"].is_cuda
    np.random.seed(4)
    cpu = PosedSdf3D(mesh, device="cpu", **kw)
    for a, b in zip(dev.frames, cpu.frames):
        # the draws are shared (same seed, same order) as long as both routes hit with the same pixels
        for k in ("sdfs", "sdfs_valid", "signs"):
            assert torch.allclose(a[k].cpu(), b[k], atol=1e-5), k
        assert torch.allclose(a["points_frame"].cpu(), b["points_frame"], atol=1e-4)


# --------------------------------------------------------------------------- 9. mesh depth frames into PosedSdfRgbd
def test_mesh_depth_frames_feed_posed_sdf_rgbd():
    """A furnished room of boxes -> render_mesh_depth for three poses -> PosedSdfRgbd.from_frames: the surface samples of a
    batch lie within 1e-3 m of the analytic union of boxes (the depth tolerance T_TOL at 10 m is 2e-4 m; the back-
    projection adds a few fp32 roundings at the same scale)."""
    import test_mesh_host as host
    from miso_amd import ops
    from miso_amd.grid_opt.datasets.sdf_rgbd import PosedSdfRgbd
    from miso_amd.grid_opt.utils import utils_sdf
    furniture = [np.array([[1.0, 2.2], [3.5, 4.5], [0.0, 0.8]]), np.array([[5.0, 6.5], [1.0, 1.8], [0.0, 1.1]])]
    v, t = mc.join([(m.vertices, m.triangles) for m in [utils_sdf.box_mesh(host.ROOM)] + [utils_sdf.box_mesh(b) for b in furniture]])
    ix = ops.MeshIndex(_dev(v.astype(np.float32)), _dev(t))
    cam = host._camera()
    Rs, ts = host.posed_sdf_3d_poses()
    frames = [utils_sdf.render_mesh_depth(ix, Rs[k], ts[k], cam)[0] for k in range(3)]
    depth = torch.stack(frames)
    assert (depth > 0).float().mean() > 0.99
    ds = PosedSdfRgbd.from_frames(depth.cpu(), Rs, ts, cam, n_rays=512, n_strat_samples=3, n_surf_samples=4, trunc_dist=0.15,
                                  max_depth=12.0, device="cuda:0")
    torch.manual_seed(2)
    inp, gt = ds[0]
    rows, S = int(gt["sdf"].shape[0]), 4 + 3                   # S rows per ray: [surface, near x 3, stratified x 3]
    assert rows % S == 0 and rows >= 1000 * S
    surf = torch.arange(0, rows, S, device=gt["sdf"].device)
    assert (gt["sdf"][surf].abs() <= 1e-6).all() and gt["sdf_valid"][surf].all()
    ids = inp["sample_frame_ids"][:, 0][surf].cpu()
    x = inp["coords_frame"][surf].cpu().double()
    world = (torch.einsum("nij,nj->ni", Rs[ids].double(), x) + ts[ids, :, 0].double()).numpy()

    def box_sdf(p, b):                                          # signed distance to a box, negative inside
        q = np.maximum(b[:, 0] - p, p - b[:, 1])
        return np.linalg.norm(np.maximum(q, 0.0), axis=1) + np.minimum(q.max(axis=1), 0.0)

    dist = np.minimum.reduce([np.abs(box_sdf(world, host.ROOM))] + [np.abs(box_sdf(world, b)) for b in furniture])
    print(f"surface samples: {len(surf)}, max distance to the union of boxes {dist.max():.3e} m")
    assert dist.max() <= 1e-3
