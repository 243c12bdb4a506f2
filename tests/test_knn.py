"""k nearest neighbours on the cell-list index and normals from them (csrc/knn.hip; ops.NearestIndex.knn / normals(knn=),
ops.knn / knn_all_pairs, utils_registration.estimate_normals and the callers that take kNN normals), on the GPU.

The index route and the all-pairs route agree bit for bit on every case and k, both equal the rule restated in numpy
fp32, every returned neighbour is one of the true k nearest within the rounding of its distance, the fallback kernel is
forced and gives the same bits, and a strided view, a second call, a side stream and a replayed graph return them too.
kNN normals are held to numpy.linalg.eigh on the same neighbour sets and to bit equality across two builds."""
import numpy as np
import pytest
import torch

import icp_cases as ic
import knn_cases as kc
import nn_cases as nc

pytestmark = pytest.mark.gpu


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


_indices, _results = {}, {}


def _index(name):
    if name not in _indices:
        from miso_amd import ops
        c = kc.case(name)
        _indices[name] = ops.NearestIndex(_dev(c["tgt"]), cell=c["cell"], max_rings=c["max_rings"])
    return _indices[name]


def _run(name, k):
    """(index route d2, idx, stats; all-pairs route d2, idx) of a case at k as numpy arrays, computed once"""
    if (name, k) not in _results:
        from miso_amd import ops
        c = kc.case(name)
        src = _dev(c["src"])
        d2, idx, stats = _index(name).knn(src, k)
        e2, edx = ops.knn_all_pairs(src, _dev(c["tgt"]), k)
        torch.cuda.synchronize()
        _results[(name, k)] = tuple(_host(t) for t in (d2, idx, stats, e2, edx))
    return _results[(name, k)]


def _same(got_d2, got_idx, want_d2, want_idx):
    return np.array_equal(_bits(got_d2), _bits(want_d2)) and np.array_equal(got_idx, want_idx)


# --------------------------------------------------------------------------- 1, 2. the two routes and the fp32 rule
@pytest.mark.parametrize("k", kc.KS)
@pytest.mark.parametrize("name", nc.NAMES)
def test_index_and_all_pairs_agree_bit_for_bit(name, k):
    d2, idx, stats, e2, edx = _run(name, k)
    n = len(kc.case(name)["src"])
    assert d2.shape == (n, k) == idx.shape and d2.dtype == np.float32 and idx.dtype == np.int64
    assert _same(d2, idx, e2, edx)
    assert int(stats[0]) + int(stats[1]) == n


@pytest.mark.parametrize("k", kc.KS)
@pytest.mark.parametrize("name", nc.NAMES)
def test_both_routes_equal_the_rule_in_numpy_fp32(name, k):
    """d2 bits and indices: ties to the lowest index (`lattice` at k = 7 cuts through eight equidistant corners, `dup`
    holds every target twice), (+inf, -1) beyond the finite targets (`single`, `empty`, `nan_targets`) and for a query
    with a non-finite coordinate (`nan`)."""
    d2, idx, _, e2, edx = _run(name, k)
    D, I = kc.reference32(name, k)
    assert _same(d2, idx, D, I) and _same(e2, edx, D, I)


@pytest.mark.parametrize("name", nc.NAMES)
def test_k_equal_to_one_is_the_query(name):
    c = kc.case(name)
    d2, idx, stats, _, _ = _run(name, 1)
    q2, qdx, qstats = _index(name).query(_dev(c["src"]))
    assert _same(d2[:, 0], idx[:, 0], _host(q2), _host(qdx)) and np.array_equal(stats, _host(qstats))


# --------------------------------------------------------------------------- 3. float64
@pytest.mark.parametrize("k", kc.KS)
@pytest.mark.parametrize("name", nc.NAMES)
def test_every_neighbour_is_among_the_true_k_nearest(name, k):
    """D_k = the true k-th smallest squared distance (float64 on the fp32 inputs).  A computed d2 is within 5.1 u (u = 2^-24,
    relative) of the true one on both sides (csrc/nn.hpp, ring_finished), and the kernel orders computed values: a
    returned neighbour j has computed d2_j <= the computed k-th smallest <= D_k (1 + 5.1 u), hence a true
    D_j <= D_k (1 + 5.1 u) / (1 - 5.1 u) < D_k (1 + 2^-20).  Derived, not measured.  The number of neighbours is that of
    the reference, and no index repeats."""
    d2, idx, _, _, _ = _run(name, k)
    c = kc.case(name)
    D, I = kc.reference64(name, k)
    assert np.array_equal(idx >= 0, I >= 0)
    assert (idx < max(len(c["tgt"]), 1)).all()
    has = idx >= 0
    assert np.isposinf(d2[~has]).all() and np.isfinite(d2[has]).all()
    with np.errstate(invalid="ignore"):
        assert (np.diff(d2.astype(np.float64), axis=1)[has[:, 1:]] >= 0).all()          # ascending
    taken = np.sort(np.where(has, idx, -1 - np.arange(k)[None, :]), axis=1)
    assert (np.diff(taken, axis=1) != 0).all()                                           # no neighbour twice
    Dj = kc.true_d2(c["src"], c["tgt"], idx)
    kth = np.where(has, D, -np.inf).max(axis=1, keepdims=True)                           # the last finite column
    assert (Dj[has] <= np.broadcast_to(kth, Dj.shape)[has] * (1.0 + 2.0 ** -20)).all()
    assert (np.abs(d2[has].astype(np.float64) - Dj[has]) <= 2.0 ** -21 * Dj[has]).all()


# --------------------------------------------------------------------------- 4. the fallback
def test_the_all_pairs_kernel_behind_the_rings():
    """`far` and `segments` reach it as they are; on `room` it is forced with no ring beyond the query's own 2 cm cell.
    The listed queries get the bits of the all-pairs route, and the counters add up to the (all finite) queries."""
    from miso_amd import ops
    for name, k in (("far", 30), ("segments", 30), ("segments", 7)):
        d2, idx, stats, e2, edx = _run(name, k)
        n = len(kc.case(name)["src"])
        assert int(stats[0]) + int(stats[1]) == n and _same(d2, idx, e2, edx)
    assert int(_run("far", 30)[2][1]) == 700
    assert int(_run("segments", 30)[2][1]) >= 230
    c = kc.case("room")
    index = ops.NearestIndex(_dev(c["tgt"]), cell=0.02, max_rings=0)
    for k in (1, 30):
        d2, idx, stats = (_host(t) for t in index.knn(_dev(c["src"]), k))
        want = _run("room", k)
        assert int(stats[0]) + int(stats[1]) == len(c["src"]) and int(stats[1]) >= 1000
        assert _same(d2, idx, want[3], want[4])
    nrm_forced, cnt_forced = index.normals(_dev(c["src"]), knn=30)                       # normals of listed queries too
    nrm, cnt = _index("room").normals(_dev(c["src"]), knn=30)
    assert torch.equal(nrm_forced.view(torch.int32), nrm.view(torch.int32)) and torch.equal(cnt_forced, cnt)


# --------------------------------------------------------------------------- 5. edge sizes
@pytest.mark.parametrize("name", kc.N_NAMES + kc.M_NAMES)
def test_edge_sizes(name):
    """N in {0, 1, 63, 64, 65, 255, 256, 257} against 1 031 targets, M in {0, 1, 2, 29, 30, 31}, all at k = 30"""
    d2, idx, stats, e2, edx = _run(name, 30)
    D, I = kc.reference32(name, 30)
    c = kc.case(name)
    assert d2.shape == (len(c["src"]), 30)
    assert _same(d2, idx, D, I) and _same(e2, edx, D, I)
    assert ((idx >= 0).sum(axis=1) == min(30, len(c["tgt"]))).all()
    assert int(stats[0]) + int(stats[1]) == len(c["src"])


def test_more_queries_than_one_chunk():
    """N = 2^20 + 1 queries at k = 2 against 1 031 targets run as two chunks: the routes agree bit for bit, the counters
    add up, and the queries around the chunk border and at both ends follow the fp32 rule."""
    from miso_amd import _lib, ops
    n = _lib.NN_CHUNK + 1
    rng = np.random.default_rng(1700)
    tgt = kc.case("n257")["tgt"]
    src = rng.random((n, 3), dtype=np.float32)
    src[[5, _lib.NN_CHUNK - 1, _lib.NN_CHUNK]] += np.float32(3.0)                        # listed queries in both chunks
    s, t = _dev(src), _dev(tgt)
    d2, idx, stats = ops.NearestIndex(t, cell=0.1, max_rings=2).knn(s, 2)
    e2, edx = ops.knn_all_pairs(s, t, 2)
    assert torch.equal(d2.view(torch.int32), e2.view(torch.int32)) and torch.equal(idx, edx)
    stats = _host(stats)
    assert int(stats[0]) + int(stats[1]) == n and int(stats[1]) >= 3
    pick = np.concatenate([np.arange(300), np.arange(_lib.NN_CHUNK - 300, n)])
    D, I = kc.knn32(src[pick], tgt, 2)
    assert _same(_host(d2)[pick], _host(idx)[pick], D, I)


# --------------------------------------------------------------------------- 6. reproducibility
def test_strided_view_two_calls_a_side_stream_and_a_replayed_graph_return_the_same_bits():
    from miso_amd import ops
    c = kc.case("room")
    k = 30
    want = _run("room", k)
    src, tgt = _dev(c["src"]), _dev(c["tgt"])
    src4 = torch.zeros(len(c["src"]), 4, device="cuda")
    tgt4 = torch.full((len(c["tgt"]), 4), 7.0, device="cuda")
    src4[:, :3], tgt4[:, :3] = src, tgt
    ix = ops.NearestIndex(tgt4[:, :3], cell=c["cell"], max_rings=c["max_rings"])
    assert ix.tgt.data_ptr() == tgt4.data_ptr()                          # no copy

    def same(d2, idx, stats=None):
        torch.cuda.synchronize()
        return _same(_host(d2), _host(idx), want[0], want[1]) and (stats is None or np.array_equal(_host(stats), want[2]))

    assert same(*ix.knn(src4[:, :3], k))                                 # a second index over a view, a view queried
    assert same(*ix.knn(src, k))                                         # a second call
    assert same(*ops.knn_all_pairs(src4[:, :3], tgt4[:, :3], k))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = ops.NearestIndex(tgt, cell=c["cell"], max_rings=c["max_rings"]).knn(src, k)
    side.synchronize()
    assert same(*out)
    n = len(c["src"])
    out = (torch.empty((n, k), device="cuda"), torch.empty((n, k), device="cuda", dtype=torch.int64),
           torch.empty(2, device="cuda", dtype=torch.int32))
    ix.knn(src, k, out=out)                                              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ix.knn(src, k, out=out)
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        assert same(*out)


def test_knn_picks_a_route_by_size_and_both_give_the_same_bits(monkeypatch):
    from miso_amd import ops
    c = kc.case("crowd")
    src, tgt = _dev(c["src"]), _dev(c["tgt"])
    want = _run("crowd", 7)
    assert len(c["src"]) * len(c["tgt"]) < ops.NN_ALL_PAIRS_BELOW
    small = ops.knn(src, tgt, 7)                                         # the all-pairs route
    monkeypatch.setattr(ops, "NN_ALL_PAIRS_BELOW", 0)
    large = ops.knn(src, tgt, 7)                                         # the index route, default cell and rings
    for d2, idx in (small, large):
        assert _same(_host(d2), _host(idx), want[0], want[1])
    with pytest.raises(ValueError, match="outside 1 .. 32"):
        ops.knn(src, tgt, 33)
    with pytest.raises(ValueError, match="outside 1 .. 32"):
        ops.NearestIndex(tgt).knn(src, 0)


# --------------------------------------------------------------------------- 7. normals
NORMALS_ASSERTED = 1e-6     # rad: the bound tests/test_icp.py holds the radius normals to (same closed form, same sums)


def _angles(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.arcsin(np.minimum(np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)), 1.0))


def test_knn_normals_against_eigh():
    """The fixture's targets among themselves at k = 30: the fp32 and float64 neighbour sets are equal
    (tests/test_knn_host.py), so numpy.linalg.eigh on knn64's sets is the reference.  Counts equal min(k, M); where the
    eigen-gap is at least 0.05 (all but one point) the angle is asserted below 1e-6 rad.  The measured worst angle is
    printed, and recorded in DESIGN.md section 4.14."""
    from miso_amd import ops
    f = ic.fixture()
    want, counts, gaps = kc.fixture_normals()
    index = ops.NearestIndex(_dev(f["tgt"]))
    normals, got_counts = index.normals(knn=kc.K_NORMALS)
    assert normals.dtype == torch.float32 and normals.shape == (6000, 3) and got_counts.dtype == torch.int32
    assert (_host(got_counts) == kc.K_NORMALS).all() and np.array_equal(_host(got_counts), counts)
    n = _host(normals).astype(np.float64)
    assert np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    clear = gaps >= 0.05
    worst = _angles(n[clear], want[clear]).max()
    print(f"knn normals: worst angle {worst:.3e} rad over {clear.sum()} points with an eigen-gap >= 0.05")
    assert worst <= NORMALS_ASSERTED
    # the lists behind them are the reference's
    d2, idx, stats = index.knn(_dev(f["tgt"]), kc.K_NORMALS)
    assert _same(_host(d2), _host(idx), *kc.fixture_neighbours()[2:])
    assert int(_host(stats)[1]) == 0                                     # the default index finishes the fixture in its rings
    # another cloud against the index
    q = f["src"][:500]
    qI = kc.knn64(q, f["tgt"], kc.K_NORMALS)[1]
    assert np.array_equal(np.sort(qI, axis=1), np.sort(kc.knn32(q, f["tgt"], kc.K_NORMALS)[1], axis=1))
    want_q, counts_q, gaps_q = kc.knn_normals64(f["tgt"], q, qI)
    nq, cq = index.normals(_dev(q), knn=kc.K_NORMALS)
    assert np.array_equal(_host(cq), counts_q)
    assert _angles(_host(nq)[gaps_q >= 0.05], want_q[gaps_q >= 0.05]).max() <= NORMALS_ASSERTED
    with pytest.raises(ValueError, match="not both"):
        index.normals(radius=0.4, knn=30)
    assert torch.equal(index.normals()[1], index.normals(radius=ops.NN_NORMAL_SPACINGS * index.spacing)[1])   # the default stays


def test_knn_normals_do_not_depend_on_the_build():
    """Two indices over a permuted copy of the targets, and a second build of the same one: the same normal bits for the
    same points (compared through the permutation).  The fixture has no fp32 tie inside a list
    (tests/test_knn_host.py), so the order of accumulation is the same under the permutation too."""
    from miso_amd import ops
    t = ic.fixture()["tgt"]
    perm = np.random.default_rng(1701).permutation(len(t))
    a, ca = ops.NearestIndex(_dev(t)).normals(knn=kc.K_NORMALS)
    b, cb = ops.NearestIndex(_dev(t)).normals(knn=kc.K_NORMALS)
    p, cp = ops.NearestIndex(_dev(t[perm])).normals(knn=kc.K_NORMALS)
    assert np.array_equal(_bits(_host(a)), _bits(_host(b))) and torch.equal(ca, cb)
    assert np.array_equal(_bits(_host(a))[perm], _bits(_host(p))) and np.array_equal(_host(ca)[perm], _host(cp))
    q32 = kc.knn32(ic.fixture()["src"][:700], t, kc.K_NORMALS)[0]
    assert not (np.diff(q32, axis=1) == 0).any()                          # no tie here either
    q = _dev(ic.fixture()["src"][:700])
    qa, _ = ops.NearestIndex(_dev(t)).normals(q, knn=kc.K_NORMALS)
    qp, _ = ops.NearestIndex(_dev(t[perm]), cell=0.13).normals(q, knn=kc.K_NORMALS)       # another cell as well
    assert np.array_equal(_bits(_host(qa)), _bits(_host(qp)))


def test_knn_normals_fall_back_to_z():
    """fewer than three targets, targets on a line, a query with a non-finite coordinate, no target: (0, 0, 1) and the
    count; a patch in the plane x = 5: (+-1, 0, 0)"""
    from miso_amd import ops
    for m in (1, 2):
        tgt = np.array([[0.0, 0, 0], [1.0, 2.0, 3.0]], dtype=np.float32)[:m]
        n, c = ops.NearestIndex(_dev(tgt)).normals(knn=30)
        assert (_host(c) == m).all() and (_host(n) == [0.0, 0.0, 1.0]).all()
    line = np.stack([np.arange(40) * 0.1, np.zeros(40), np.zeros(40)], axis=1).astype(np.float32)
    n, c = ops.NearestIndex(_dev(line)).normals(knn=30)
    assert (_host(c) == 30).all() and (_host(n) == [0.0, 0.0, 1.0]).all()
    k = np.arange(6) * 0.1
    patch = np.stack([np.full(36, 5.0), *[g.ravel() for g in np.meshgrid(k, k, indexing="ij")]], axis=1).astype(np.float32)
    index = ops.NearestIndex(_dev(patch))
    n, c = (_host(t) for t in index.normals(knn=30))
    assert (c == 30).all() and np.abs(np.abs(n[:, 0]) - 1.0).max() < 1e-6 and np.abs(n[:, 1:]).max() < 1e-6
    n, c = index.normals(_dev(np.array([[np.nan, 0, 0], [0, np.inf, 0]])), knn=30)
    assert _host(c).tolist() == [0, 0] and (_host(n) == [0.0, 0.0, 1.0]).all()
    empty = ops.NearestIndex(torch.empty((0, 3), device="cuda"))
    n, c = empty.normals(_dev(patch), knn=30)
    assert (_host(c) == 0).all() and (_host(n) == [0.0, 0.0, 1.0]).all()
    d2, idx, stats = empty.knn(_dev(patch), 3)
    assert np.isposinf(_host(d2)).all() and (_host(idx) == -1).all() and _host(stats).tolist() == [36, 0]


# --------------------------------------------------------------------------- 8. users
def test_estimate_normals_defaults_to_the_thirty_nearest():
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_registration as reg
    t = _dev(ic.fixture()["tgt"])
    index = ops.NearestIndex(t)
    got = reg.estimate_normals(t)
    assert got.shape == (6000, 3) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), index.normals(knn=30)[0].view(torch.int32))
    assert torch.equal(reg.estimate_normals(t, index=index).view(torch.int32), got.view(torch.int32))
    assert torch.equal(reg.estimate_normals(t, knn=12).view(torch.int32), index.normals(knn=12)[0].view(torch.int32))
    assert torch.equal(reg.estimate_normals(t, radius=0.4).view(torch.int32), index.normals(radius=0.4)[0].view(torch.int32))
    with pytest.raises(ValueError, match="not built on points"):
        reg.estimate_normals(t[:100], index=index)


def test_align_submap_pair_with_knn_normals_on_the_golden_atlas():
    import fusion_cases as fc
    from test_grid_opt_mirror import _OneBatch, make_atlas_two_kf
    from miso_amd.grid_opt.align import icp
    atlas = make_atlas_two_kf("cuda:0")
    mi, gt = fc.fusion_batch()

    class OnDevice(_OneBatch):
        def __getitem__(self, i):
            a, b = super().__getitem__(i)
            return {k: v.to("cuda:0") for k, v in a.items()}, {k: v.to("cuda:0") for k, v in b.items()}

    kw = dict(voxel_size=0.3, threshold_factor_fine=6, num_batches=1, trunc_dist=0.05, update_grid_atlas=False)
    result, info, _ = icp.align_submap_pair(atlas, OnDevice(mi, gt), 0, 1, normals_knn=30, **kw)
    print(f"align_submap_pair(normals_knn=30): {result}")
    assert np.isfinite(result.transformation).all() and np.isfinite(result.fitness) and np.isfinite(result.inlier_rmse)
    assert np.allclose(result.transformation[:3, :3] @ result.transformation[:3, :3].T, np.eye(3), atol=1e-5)
    assert info.shape == (6, 6) and np.isfinite(info).all() and np.allclose(info, info.T)
    assert np.linalg.eigvalsh(info).min() >= -1e-9 * max(np.abs(info).max(), 1.0)       # positive semi-definite


def test_align_mesh_to_ref_with_knn_normals():
    """Two meshes of the fixture shape 2 deg / 4 cm apart.  The float64 loop (icp_cases.icp_loop64: coarse with the L2
    loss, fine with Tukey's) runs on the SAME samples with knn_normals64's normals of the float64 neighbour sets; the
    device's pose is asked to lie within twice the float64 loop's error against the true pose.  utils_ncd's function is
    the same pipeline for a mesh reference, and takes a point cloud too: given the reference's samples as the cloud it
    is asked to halve the 4 cm and to cut the 2 deg (0.035 rad) to 0.01 rad, that is, to have aligned at all (the fitness at
    the fine threshold of 3 cm says little here: 3 000 samples of 63 m^2 lie 14 cm apart)."""
    from miso_amd.grid_opt.utils import utils_ncd, utils_scannet, utils_sdf
    v, tri = ic.shape_mesh()
    truth = ic.pose(2.0, 0.04)
    gt, moved = utils_sdf.TriangleMesh(v, tri), utils_sdf.TriangleMesh(ic.apply64(np.linalg.inv(truth), v), tri)
    points, iters = 3000, 100
    aligned, result = utils_scannet.align_mesh_to_ref(moved, gt, num_points=points, normals='knn')
    device = torch.device("cuda:0")
    src = _host(utils_scannet._sampled(moved, points, 0, device, False)[0])
    tgt = _host(utils_scannet._sampled(gt, points, 1, device, False)[0])
    nrm = kc.knn_normals64(tgt, tgt, kc.knn64(tgt, tgt, 30)[1])[0]
    coarse = ic.icp_loop64(src, tgt, nrm, 0.02 * 15, None, "point_to_plane", None, iters)[0]
    T64 = ic.icp_loop64(src, tgt, nrm, 0.02 * 1.5, coarse, "point_to_plane", 1e-2, iters)[0]
    dt64, dr64 = ic.pose_error(T64, truth)
    dt, dr = ic.pose_error(result.transformation, truth)
    print(f"align_mesh_to_ref(normals='knn'): {result}; translation error {dt:.3e} m (float64 loop {dt64:.3e}), "
          f"rotation error {dr:.3e} rad (float64 loop {dr64:.3e})")
    assert dt <= 2 * dt64 and dr <= 2 * dr64
    assert aligned is not moved and np.abs(aligned.vertices - ic.apply64(result.transformation, moved.vertices)).max() < 1e-9
    with pytest.raises(ValueError, match="Unknown normals"):
        utils_scannet.align_mesh_to_ref(moved, gt, normals='vertex')
    _, ncd = utils_ncd.align_mesh_to_ref(moved, gt, num_points=points)
    assert np.array_equal(ncd.transformation, result.transformation)                    # the same samples, the same passes
    _, cloud = utils_ncd.align_mesh_to_ref(moved, tgt, num_points=points, ref_format='pointcloud')
    ct, cr = ic.pose_error(cloud.transformation, truth)
    print(f"utils_ncd.align_mesh_to_ref(ref_format='pointcloud'): {cloud}; {ct:.3e} m, {cr:.3e} rad")
    assert np.isfinite(cloud.transformation).all() and cloud.fitness > 0 and ct < 0.02 and cr < 0.01
    with pytest.raises(ValueError, match="Unknown reference format"):
        utils_ncd.align_mesh_to_ref(moved, gt, ref_format='voxels')
