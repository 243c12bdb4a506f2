"""Closest triangle, crossing counts and signed distance on the GPU (csrc/mesh_sdf.hip: ops.MeshIndex.closest /
count_crossings / contains / signed_distance, ops.closest_all / count_crossings_all / closest), and what is built on
them: utils_sdf.MeshSdf, datasets.sdf_3d.PosedSdf3D(sdf_fn='mesh') and Sdf3D.

The index route -- fine shells only, and with the coarse level at two (factor, rings) settings -- and the all-triangles
route agree bit for bit on every fixture of tests/msdf_cases.py at two cell sizes; both are the float64 distance within
msdf_cases.D_TOL (equal on `cube`); ties go to the lowest triangle index; NaN queries and NaN triangles never match;
crossing counts agree between the routes on all rays and with float64 on the kept ones (exactly on `lattice`)."""
import numpy as np
import pytest
import torch

import mesh_cases as mc
import msdf_cases as md

pytestmark = pytest.mark.gpu

FAR_SETTINGS = ((None, None), (8.0, 1))        # the library's (factor, rings), and a setting that sends most queries coarse


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(*xs):
    return tuple(x.cpu().numpy() for x in xs)


_results = {}


def _run(name):
    """{'all': (d2, tri, vw), (cell, far): (d2, tri, vw, stats)} of a fixture as numpy arrays, computed once;
    far: None = the fine shells only, else an index into FAR_SETTINGS"""
    if name not in _results:
        from miso_amd import ops
        fx = md.fixture(name)
        V, T, P = (_dev(fx[k]) for k in ("vertices", "triangles", "points"))
        out = {"all": _np(*ops.closest_all(P, V, T, want_vw=True))}
        for cell in fx["cells"]:
            ix = ops.MeshIndex(V, T, cell=cell)
            stats = torch.zeros(5, dtype=torch.int64, device="cuda")
            out[(cell, None)] = _np(*ix.closest(P, want_vw=True, stats=stats, far=False), stats)
            for k, (factor, rings) in enumerate(FAR_SETTINGS):
                ix.prepare_distance(factor, rings)
                out[(cell, k)] = _np(*ix.closest(P, want_vw=True, stats=stats), stats)
        _results[name] = out
    return _results[name]


def _same(a, b):
    """d2 as int32 bits, tri, vw as bits"""
    return bool((a[0].view(np.int32) == b[0].view(np.int32)).all() and (a[1] == b[1]).all() and
                (len(a) < 3 or len(b) < 3 or (a[2].view(np.int32) == b[2].view(np.int32)).all()))


# --------------------------------------------------------------------------- 1. the routes
@pytest.mark.parametrize("name", list(md.FIXTURES))
def test_index_route_and_all_triangles_route_agree_bit_for_bit(name):
    fx, got = md.fixture(name), _run(name)
    n = len(fx["points"])
    d2, tri, vw = got["all"]
    assert d2.shape == (n,) and tri.shape == (n,) and vw.shape == (n, 2) and d2.dtype == np.float32 and tri.dtype == np.int64
    for cell in fx["cells"]:
        for far in (None, 0, 1):
            assert _same(got[(cell, far)][:3], got["all"]), (name, cell, far)
        fine, coarse = got[(cell, None)][3], got[(cell, 1)][3]
        assert fine[1] == 0 and fine[3] == 0                           # no far set: nothing goes coarse
        assert fine[4] == coarse[4] == int((~fx["walks"]).sum())       # answered from all rows: the queries beyond 4 coord_mag
    small = fx["cells"][0]
    assert got[(small, 1)][3][3] > 0 and got[(small, 1)][3][1] > 0     # one fine shell at the small cell: some go coarse
    assert got[(small, 1)][3][0] < got[(small, None)][3][0]            # ... and walk fewer fine cells for it


# --------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("name", list(md.FIXTURES))
def test_answer_is_the_float64_distance(name):
    fx, got = md.fixture(name), _run(name)
    ref = fx["ref"]
    d2, tri, vw = got["all"]
    assert ((tri >= 0) == (ref["tri"] >= 0)).all()
    e, e_tri = md.d_error(fx, d2, tri)
    won = tri >= 0
    print(f"{name}: max e {np.nanmax(e[won], initial=0.0):.3e} (D_TOL {md.D_TOL:.3e}), triangle differs on "
          f"{int((tri != ref['tri'])[won].sum())}, worst own-distance error of a differing triangle {np.nanmax(e_tri[won], initial=0.0):.3e}")
    assert (e[won] <= md.D_TOL).all()
    assert (e_tri[won] <= md.D_TOL).all()          # the float64 winner, or a triangle whose own d64 is within the tolerance
    # the barycentrics name the closest point: |q - (v0 + v e1 + w e2)|^2 is d2
    v = fx["vertices"].astype(np.float64)[fx["triangles"][np.maximum(tri, 0)]]
    p = v[:, 0] + vw[:, :1].astype(np.float64) * (v[:, 1] - v[:, 0]) + vw[:, 1:].astype(np.float64) * (v[:, 2] - v[:, 0])
    dist = np.linalg.norm(fx["points"].astype(np.float64) - p, axis=1)
    assert (np.abs(dist - np.sqrt(d2.astype(np.float64)))[won] <= md.D_TOL * (fx["coord_max"] + dist[won])).all()
    assert (vw[won] >= 0).all() and (vw[won].sum(axis=1) <= 1 + 2.0 ** -23).all()
    if name == "cube":
        assert (d2.astype(np.float64) == ref["d2"]).all() and (tri == ref["tri"]).all()
        centre = np.nonzero((fx["points"] == 2.0).all(axis=1))[0]
        assert len(centre) == 1 and tri[centre[0]] == 0 and d2[centre[0]] == 4.0        # every face ties: the lowest index


# --------------------------------------------------------------------------- 3. the three routes of a query
def test_far_takes_all_three_routes_and_keeps_the_bits():
    fx, got = md.fixture("far"), _run("far")
    small = fx["cells"][0]
    d2, tri, vw, stats = got[(small, 0)]                               # the library's factor and rings
    n = len(fx["points"])
    print(f"far: {n} queries, stats {stats.tolist()}")
    assert stats[4] == fx["n_beyond"] and 0 < stats[3] < n - fx["n_beyond"] and stats[0] > 0 and stats[1] > 0
    assert _same((d2, tri, vw), got["all"])
    beyond = slice(n - fx["n_beyond"], n)
    assert (tri[beyond] >= 0).all() and np.isfinite(d2[beyond]).all()


# --------------------------------------------------------------------------- 4. crossing counts
_counts = {}


def _count_run(name):
    if name not in _counts:
        from miso_amd import ops
        if name == "lattice":
            fx = md.lattice()
            o, d, cells = fx["origins"], fx["dirs"], fx["cells"]
        else:
            fx = md.fixture(name)
            o, d = md.parity_rays(fx["points"])
            cells = fx["cells"]
        V, T, O, D = _dev(fx["vertices"]), _dev(fx["triangles"]), _dev(o), _dev(d)
        out = {"all": ops.count_crossings_all(O, D, V, T).cpu().numpy()}
        for cell in cells:
            out[cell] = ops.MeshIndex(V, T, cell=cell).count_crossings(O, D).cpu().numpy()
        _counts[name] = out
    return _counts[name]


@pytest.mark.parametrize("name", ["lattice"] + list(md.FIXTURES))
def test_crossing_counts_agree_between_the_routes_and_with_float64(name):
    got = _count_run(name)
    cells = [k for k in got if k != "all"]
    assert got["all"].dtype == np.int32 and len(cells) == 2
    if name == "lattice":
        want = md.lattice()["count"]
        assert (got["all"] == want).all() and want.max() >= 8           # edge and vertex rays count every triangle they touch
        for cell in cells:
            assert (got[cell] == want).all()
        return
    fx = md.fixture(name)
    inside, counts, kept = md.parity(name)
    finite = np.tile(fx["walks"] | np.isfinite(fx["points"]).all(axis=1), 3)
    for cell in cells:
        assert (got[cell] == got["all"]).all(), (name, cell)            # all rays, never filtered
    k3 = np.tile(kept, 3) & finite
    assert (got["all"][k3] == counts.reshape(-1)[k3]).all()


# --------------------------------------------------------------------------- 5. contains and signed distance
@pytest.mark.parametrize("name", [n for n in md.FIXTURES])
def test_contains_and_signed_distance_against_float64(name):
    from miso_amd import ops
    fx = md.fixture(name)
    inside, counts, kept = md.parity(name)
    if name != "cube":
        assert (~kept).mean() <= md.KEPT_CAP
    ix = ops.MeshIndex(_dev(fx["vertices"]), _dev(fx["triangles"]), cell=fx["cells"][0])
    P = _dev(fx["points"])
    got = ix.contains(P).cpu().numpy()
    assert (got == inside)[kept].all()
    sd = ix.signed_distance(P).cpu().numpy()
    neg = ix.signed_distance(P, inside_positive=False).cpu().numpy()
    d = np.sqrt(_run(name)["all"][0])
    assert (sd == np.where(got, d, -d)).all() and (neg == -sd).all()
    if name == "nested":
        assert (got == md.nested_inside(fx["points"]))[kept].all() and got.any() and (~got).any()


# --------------------------------------------------------------------------- 6. NaN, empty, sizes
def test_non_finite_queries_dead_triangles_and_an_empty_mesh():
    from miso_amd import ops
    fs, gs = md.fixture("sliver"), _run("sliver")
    dead = np.nonzero(~mc.hittable(fs["vertices"], fs["triangles"]))[0]
    assert len(dead) == 4
    for key in gs:
        assert not np.isin(gs[key][1], dead).any() and not np.isin(gs[key][1], np.arange(501, 521)).any()   # nor a duplicate's copy
    fr = md.fixture("room")
    V, T = _dev(fr["vertices"]), _dev(fr["triangles"])
    P = fr["points"][:64].copy()
    P[0, 0], P[1, 2], P[2] = np.nan, np.inf, -np.inf
    ix = ops.MeshIndex(V, T, cell=0.5)
    stats = torch.zeros(5, dtype=torch.int64, device="cuda")
    a = _np(*ix.closest(_dev(P), want_vw=True, stats=stats))
    b = _np(*ops.closest_all(_dev(P), V, T, want_vw=True))
    assert _same(a, b) and np.isposinf(a[0][:3]).all() and (a[1][:3] == -1).all() and (a[2][:3] == 0).all()
    assert int(stats.cpu()[4]) == 0                                     # a non-finite query is answered without a scan
    assert (a[1][3:] == _run("room")["all"][1][3:64]).all()
    assert (ix.count_crossings(_dev(P), _dev(np.tile(md.PARITY_DIRS[:1].astype(np.float32), (64, 1)))).cpu().numpy()[:3] == 0).all()
    assert not ix.contains(_dev(P))[:3].any()
    # an empty mesh, and a mesh of nothing but dead triangles
    none_v, none_t = torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int64, device="cuda")
    one_v = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]], device="cuda")
    bad_t = torch.tensor([[0, 0, 1], [0, 1, 7]], device="cuda")
    Q = _dev(fr["points"][:100])
    for v, t in ((none_v, none_t), (one_v, bad_t)):
        e = ops.MeshIndex(v, t)
        for d2, tri, vw in (e.closest(Q, want_vw=True), ops.closest_all(Q, v, t, want_vw=True)):
            assert torch.isposinf(d2).all() and (tri == -1).all() and (vw == 0).all()
        assert torch.isposinf(e.signed_distance(Q)).all() and not e.contains(Q).any()
        assert (e.count_crossings(Q, Q).cpu() == 0).all() and (ops.count_crossings_all(Q, Q, v, t).cpu() == 0).all()
    # a wrong dtype, a wrong shape, an out= of the wrong kind
    with pytest.raises(RuntimeError, match="fp32"):
        ix.closest(Q.double())
    for call in (lambda: ix.closest(Q[:, :2]), lambda: ix.closest(Q, out=(torch.zeros(100, device="cuda"),)),
                 lambda: ix.closest(Q, out=(torch.zeros(100, device="cuda"), torch.zeros(100, device="cuda", dtype=torch.int32))),
                 lambda: ix.count_crossings(Q, Q[:5]), lambda: ix.count_crossings(Q, Q, out=torch.zeros(100, device="cuda")),
                 lambda: ix.closest(Q, stats=torch.zeros(3, dtype=torch.int64, device="cuda"))):
        with pytest.raises(AssertionError):
            call()
    # zero queries; one triangle; counts around a wavefront and a block
    assert ix.closest(Q[:0])[0].shape == (0,) and ops.closest_all(Q[:0], V, T)[1].shape == (0,) and ix.count_crossings(Q[:0], Q[:0]).shape == (0,)
    one = ops.MeshIndex(one_v, torch.tensor([[0, 1, 2]], device="cuda"))
    q = torch.tensor([[0.25, 0.25, 3.0], [2.0, 0.0, 1.0], [-1.0, -1.0, 1.0]], device="cuda")
    d2, tri, vw = one.closest(q, want_vw=True)
    assert d2.tolist() == [4.0, 1.0, 2.0] and tri.tolist() == [0, 0, 0] and vw.tolist() == [[0.25, 0.25], [1.0, 0.0], [0.0, 0.0]]
    base = _run("room")["all"]
    R = _dev(fr["points"])
    for n in (1, 63, 64, 65, 255, 256, 257):
        for res in (ix.closest(R[:n], want_vw=True), ops.closest_all(R[:n], V, T, want_vw=True)):
            assert _same(_np(*res), tuple(x[:n] for x in base)), n


# --------------------------------------------------------------------------- 7. buffers, views, streams, graphs
def test_out_buffers_strided_views_a_side_stream_and_a_replayed_graph_return_the_eager_bits():
    """prepare_distance() builds the coarse index (a host read) outside the capture; closest and count_crossings replay."""
    from miso_amd import ops
    fx = md.fixture("room")
    want = _run("room")["all"]
    n = len(fx["points"])
    V, T, P = (_dev(fx[k]) for k in ("vertices", "triangles", "points"))
    O, D = (_dev(x) for x in md.parity_rays(fx["points"][:512]))
    want_c = ops.count_crossings_all(O, D, V, T).cpu().numpy()

    def same(d2, tri, vw):
        torch.cuda.synchronize()
        return _same((d2[:n].cpu().numpy(), tri[:n].cpu().numpy(), vw.reshape(-1)[:2 * n].reshape(n, 2).cpu().numpy()), want)

    V4 = torch.full((len(fx["vertices"]), 4), 9.0, device="cuda")
    T5 = torch.full((len(fx["triangles"]), 5), -3, dtype=torch.int64, device="cuda")
    R8 = torch.full((n, 8), 5.0, device="cuda")
    V4[:, :3], T5[:, 1:4], R8[:, 1:4] = V, T, P
    ix = ops.MeshIndex(V4[:, :3], T5[:, 1:4], cell=0.4)
    assert same(*ix.closest(R8[:, 1:4], want_vw=True))
    assert same(*ops.closest_all(R8[:, 1:4], V4[:, :3], T5[:, 1:4], want_vw=True))
    out = (torch.zeros(n + 7, device="cuda"), torch.zeros(n + 7, device="cuda", dtype=torch.int64), torch.zeros(n + 7, 2, device="cuda"))
    got = ix.closest(P, out=out, want_vw=True)
    assert all(g is o for g, o in zip(got, out)) and same(*out)
    oa = (torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda", dtype=torch.int64), torch.zeros(n, 2, device="cuda"))
    ops.closest_all(P, V, T, out=oa, want_vw=True)
    assert same(*oa)
    oc = torch.zeros(len(O) + 3, device="cuda", dtype=torch.int32)
    assert ix.count_crossings(O, D, out=oc) is oc and (oc[:len(O)].cpu().numpy() == want_c).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = ops.MeshIndex(V, T, cell=0.4).closest(P, want_vw=True)
    side.synchronize()
    assert same(*res)
    ix2 = ops.MeshIndex(V, T, cell=0.2).prepare_distance()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ix2.closest(P, out=out, want_vw=True)
        ix2.count_crossings(O, D, out=oc)
    for _ in range(2):
        for x in out + (oc,):
            x.zero_()
        graph.replay()
        assert same(*out) and (oc[:len(O)].cpu().numpy() == want_c).all()


# --------------------------------------------------------------------------- 8. the route picked by size
def test_closest_picks_a_route_by_size_and_both_give_the_same_bits(monkeypatch):
    from miso_amd import ops
    fx = md.fixture("open")
    want = _run("open")["all"]
    V, T, P = (_dev(fx[k]) for k in ("vertices", "triangles", "points"))
    nt = len(fx["triangles"])
    monkeypatch.setattr(ops, "MESH_ALL_BELOW", nt + 1)
    small = ops.closest(P, V, T, want_vw=True)
    monkeypatch.setattr(ops, "MESH_ALL_BELOW", nt)
    large = ops.closest(P, V, T, want_vw=True)
    assert _same(_np(*small), want) and _same(_np(*large), want)


# --------------------------------------------------------------------------- 9. the host layers on the device
def test_mesh_sdf_and_the_datasets_on_the_device_match_their_cpu_twins():
    import test_mesh_sdf_host as host
    from miso_amd.grid_opt.datasets.sdf_3d import PosedSdf3D, Sdf3D
    from miso_amd.grid_opt.utils import utils_sdf
    mesh = utils_sdf.box_mesh(host.ROOM)
    p = host.box_points()
    tol = md.D_TOL * (host.ROOM.max() + 1.5)
    f_dev, f_cpu = utils_sdf.MeshSdf(mesh.vertices, mesh.triangles, device="cuda:0"), utils_sdf.MeshSdf(mesh.vertices, mesh.triangles, device="cpu")
    a, b = f_dev(p), f_cpu(p)
    assert a.dtype == np.float32 and np.abs(a - b).max() <= tol and (f_dev.contains(p) == f_cpu.contains(p)).all()
    assert np.abs(a - host.box_signed_distance(p.astype(np.float64))).max() <= tol
    on = utils_sdf.mesh_signed_distance(mesh, _dev(p))
    assert on.is_cuda and np.abs(on.cpu().numpy() - a).max() == 0
    kw = dict(sdf_fn="mesh", num_frames=2, width_px=32, height_px=24, frame_samples=64, frame_batchsize=64)
    np.random.seed(5)
    dev = PosedSdf3D(mesh, device="cuda:0", **kw)
    np.random.seed(5)
    cpu = PosedSdf3D(mesh, device="cpu", **kw)
    host.check_posed_mesh(dev)
    assert dev.frames[0]["sdfs"].is_cuda and torch.allclose(dev.t_world_frame_gt.cpu(), cpu.t_world_frame_gt)
    for fa, fb in zip(dev.frames, cpu.frames):
        for k in ("sdfs", "sdfs_valid", "signs"):
            assert torch.allclose(fa[k].cpu(), fb[k], atol=1e-5), k
        assert torch.allclose(fa["points_frame"].cpu(), fb["points_frame"], atol=1e-4)
    for trunc in (None, 0.2):
        np.random.seed(9)
        sd = Sdf3D(mesh, total_samples=2 ** 10, batch_size=128, trunc_dist=trunc, device="cuda:0")
        np.random.seed(9)
        sc = Sdf3D(mesh, total_samples=2 ** 10, batch_size=128, trunc_dist=trunc, device="cpu")
        host.check_sdf_3d(sd, 2 ** 10, 128, trunc)
        assert sd.coords.is_cuda and torch.equal(sd.coords.cpu(), sc.coords)
        assert torch.allclose(sd.sdfs.cpu(), sc.sdfs, atol=tol)
        near = ((sc.sdfs.abs() - (trunc or 1e9)).abs() < 10 * tol) | (sc.sdfs.abs() < 10 * tol)      # labels on a threshold may flip
        assert torch.equal(sd.sdf_valid.cpu()[~near], sc.sdf_valid[~near]) and torch.equal(sd.sdf_signs.cpu()[~near], sc.sdf_signs[~near])
