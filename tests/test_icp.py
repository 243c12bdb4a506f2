"""ICP on the GPU (csrc/icp.hip, ops.icp_transform / icp_sums / IcpWorkspace / NearestIndex.normals,
utils_registration.registration_icp, utils_scannet.align_mesh_to_ref, tools/eval_mesh.py --align, align/icp.py) against the
float64 restatements of tests/icp_cases.py.  What the fixtures must satisfy for these comparisons to be fair is asserted
on the CPU in tests/test_icp_host.py."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import icp_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24, U52 = 2.0 ** -24, 2.0 ** -52
ORIGIN = (2.0, 1.5, 1.25)
KIND_LOSS = [("point_to_plane", None), ("point_to_plane", ic.SUMS_TUKEY_K), ("point_to_point", None),
             ("point_to_point", ic.SUMS_TUKEY_K)]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def _host(t):
    return t.detach().cpu().numpy()


def _search(src, tgt):
    """(moved, d2, idx) on the device for src at the identity pose: the kernels' own p' and correspondences"""
    from miso_amd import ops
    moved = ops.icp_transform(_dev(src), np.eye(4))
    d2, idx, _ = ops.NearestIndex(_dev(tgt)).query(moved)
    return moved, d2, idx


def _check_sums(got, moved, d2, idx, tgt, normals, max_dist, kind, k, n_rows):
    """every entry within n 2^-52 sum|terms| of the exactly added float64 terms; the count exactly"""
    want, absum, inl = ic.sums64(_host(moved), _host(d2), _host(idx), tgt, normals, max_dist, kind,
                                 k if kind == "point_to_plane" else None, ORIGIN)
    got = _host(got)
    assert got.shape == (ic.SUMS,) and got[0] == inl.sum() == want[0]
    bound = n_rows * U52 * absum
    worst = np.abs(got - want) - bound
    assert (worst <= 0).all(), (kind, k, np.argmax(worst), got[np.argmax(worst)], want[np.argmax(worst)])
    assert (got[absum == 0.0] == 0.0).all()
    return want, inl


# --------------------------------------------------------------------------- 1. transform
@pytest.mark.gpu
def test_transform_is_within_the_rounding_of_its_five_operations():
    from miso_amd import ops
    f = ic.fixture()
    for T in (f["pose"], np.linalg.inv(f["pose"]), ic.pose(170.0, 3.0)):
        want, mag = ic.transform64(T, f["src"])
        got = ops.icp_transform(_dev(f["src"]), T)
        assert got.dtype == torch.float32 and got.shape == (5000, 3) and got.is_contiguous()
        assert (np.abs(_host(got).astype(np.float64) - want) <= 8 * U24 * mag).all()
        wide = torch.full((5000, 5), 7.0, device="cuda")
        wide[:, 1:4] = _dev(f["src"])
        out = torch.empty((5000, 3), device="cuda")
        assert ops.icp_transform(wide[:, 1:4], T, out=out) is out and torch.equal(out, got)      # read in place, same bits
    assert torch.equal(ops.icp_transform(_dev(f["src"]), np.eye(4)), _dev(f["src"]))
    assert ops.icp_transform(torch.empty((0, 3), device="cuda"), np.eye(4)).shape == (0, 3)


# --------------------------------------------------------------------------- 2. sums
@pytest.fixture(scope="module")
def searched():
    f = ic.fixture()
    return _search(f["src"], f["tgt"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,k", KIND_LOSS)
def test_sums_against_float64(searched, kind, k):
    from miso_amd import ops
    f = ic.fixture()
    moved, d2, idx = searched
    got = ops.icp_sums(moved, d2, idx, _dev(f["tgt"]), _dev(f["normals"]), max_dist=ic.SUMS_MAX_DIST, kind=kind, tukey_k=k,
                       origin=ORIGIN)
    want, inl = _check_sums(got, moved, d2, idx, f["tgt"], f["normals"], ic.SUMS_MAX_DIST, kind, k, 5000)
    # the inliers are those of the float64 search (test_icp_host.py: no pair sits at the threshold)
    d64 = np.sqrt(ic.nearest64(f["src"], f["tgt"])[0])
    assert np.array_equal(inl, d64 <= ic.SUMS_MAX_DIST) and 1500 < inl.sum() < 4000
    if kind == "point_to_plane" and k is not None:
        plain = ic.sums64(_host(moved), _host(d2), _host(idx), f["tgt"], f["normals"], ic.SUMS_MAX_DIST, kind, None)[0]
        assert 0.0 < want[29] < plain[29] and 0.0 < want[22] < plain[22]            # some weights 0, some not
    if kind == "point_to_point" and k is not None:                                   # no kernel on point-to-point
        again = ops.icp_sums(moved, d2, idx, _dev(f["tgt"]), None, max_dist=ic.SUMS_MAX_DIST, kind=kind, origin=ORIGIN)
        assert _host(again).tobytes() == _host(got).tobytes()


@pytest.mark.gpu
def test_a_pair_exactly_at_max_dist_is_an_inlier():
    """`<=`: of the three placed pairs the one at exactly 0.25 and the one a step inside count, the one a step beyond
    does not"""
    from miso_amd import ops
    src, tgt, max_dist = ic.placed_pairs()
    moved = ops.icp_transform(_dev(src), np.eye(4))
    d2, idx = ops.nearest_all_pairs(moved, _dev(tgt))
    assert _host(idx).tolist() == [0, 1, 2] and _host(d2)[0] == 0.0625 and _host(d2)[1] > 0.0625 > _host(d2)[2]
    got = _host(ops.icp_sums(moved, d2, idx, _dev(tgt), None, max_dist=max_dist, kind="point_to_point"))
    want = ic.sums64(src, _host(d2), _host(idx), tgt, None, max_dist, "point_to_point")[0]
    assert got[0] == 2.0 and got[1] == float(_host(d2)[0]) + float(_host(d2)[2]) and np.array_equal(got, want)
    work = ops.IcpWorkspace(_dev(src), ops.NearestIndex(_dev(tgt)))
    assert work.step(np.eye(4), max_dist, "point_to_point")[0] == 2.0
    assert work.step(np.eye(4), 0.25 + 2e-7, "point_to_point")[0] == 3.0        # (an fp32 step at 1.25 is 1.2e-7)


# --------------------------------------------------------------------------- 3. shapes where a reduction goes wrong
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097, 512 * 256 + 257])
def test_sums_at_every_block_shape(n):
    """one lane, one wavefront and one block, each less and more than full; 17 blocks; and more rows than the 512 x 256
    lanes of the largest grid, where a lane adds several pairs"""
    from miso_amd import ops
    f = ic.fixture()
    src = np.tile(f["src"], (n // 5000 + 1, 1))[:n]
    moved, d2, idx = _search(src, f["tgt"])
    for kind, k in (("point_to_plane", ic.SUMS_TUKEY_K), ("point_to_point", None)):
        got = ops.icp_sums(moved, d2, idx, _dev(f["tgt"]), _dev(f["normals"]), max_dist=ic.SUMS_MAX_DIST, kind=kind,
                           tukey_k=k, origin=ORIGIN)
        _check_sums(got, moved, d2, idx, f["tgt"], f["normals"], ic.SUMS_MAX_DIST, kind, k, max(n, 1))
        if n == 0:
            assert (_host(got) == 0.0).all()


@pytest.mark.gpu
def test_sums_edge_cases_and_determinism(searched):
    from miso_amd import ops
    f = ic.fixture()
    tgt, nrm = _dev(f["tgt"]), _dev(f["normals"])
    moved, d2, idx = searched
    args = dict(max_dist=ic.SUMS_MAX_DIST, kind="point_to_plane", tukey_k=ic.SUMS_TUKEY_K, origin=ORIGIN)
    first = _host(ops.icp_sums(moved, d2, idx, tgt, nrm, **args))
    # all rows outliers
    for kind in ("point_to_plane", "point_to_point"):
        assert (_host(ops.icp_sums(moved, d2, idx, tgt, nrm, max_dist=1e-9, kind=kind)) == 0.0).all()
    # Tukey with every |r| > k: the pairs are counted, their weights are zero
    got = _host(ops.icp_sums(moved, d2, idx, tgt, nrm, max_dist=ic.SUMS_MAX_DIST, kind="point_to_plane", tukey_k=1e-9))
    assert got[0] == first[0] > 0 and got[1] == first[1] > 0 and (got[2:] == 0.0).all()
    want = ic.sums64(_host(moved), _host(d2), _host(idx), f["tgt"], f["normals"], ic.SUMS_MAX_DIST, "point_to_plane", 1e-9)[0]
    assert (want[2:] == 0.0).all()
    # a NaN source row finds no target (idx = -1) and is skipped
    src = f["src"].copy()
    inlier_row = int(np.nonzero(_host(d2) <= ic.SUMS_MAX_DIST ** 2)[0][3])
    src[inlier_row, 1] = np.nan
    m2, dd2, i2 = _search(src, f["tgt"])
    assert _host(i2)[inlier_row] == -1 and np.isinf(_host(dd2)[inlier_row])
    got = ops.icp_sums(m2, dd2, i2, tgt, nrm, **args)
    _check_sums(got, m2, dd2, i2, f["tgt"], f["normals"], ic.SUMS_MAX_DIST, "point_to_plane", ic.SUMS_TUKEY_K, 5000)
    assert _host(got)[0] == first[0] - 1 and np.isfinite(_host(got)).all()
    # two calls, a workspace of its own each: the same bits; and on a side stream
    assert _host(ops.icp_sums(moved, d2, idx, tgt, nrm, **args)).tobytes() == first.tobytes()
    work = ops.IcpWorkspace(_dev(f["src"]), ops.NearestIndex(tgt), nrm)
    eager = work.step(np.eye(4), ic.SUMS_MAX_DIST, "point_to_plane", ic.SUMS_TUKEY_K)
    assert eager.tobytes() == first.tobytes() and eager.dtype == np.float64
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = work.step(np.eye(4), ic.SUMS_MAX_DIST, "point_to_plane", ic.SUMS_TUKEY_K)
    side.synchronize()
    assert on_side.tobytes() == first.tobytes()


# --------------------------------------------------------------------------- 4. normals
NORMALS_ASSERTED = 1e-6     # rad; see test_normals_against_eigh


def _angles(a, b):
    """angle between the lines of a and b, rows; by the cross product: no cancellation at small angles"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.arcsin(np.minimum(np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)), 1.0))


@pytest.mark.gpu
def test_normals_against_eigh():
    """Counts equal normals64's exactly.  Where the eigen-gap (l1 - l0) / l2 is at least 0.05 the angle to
    numpy.linalg.eigh's eigenvector of the same neighbour set is asserted below NORMALS_ASSERTED = 1e-6 rad.  Measured on
    the MI355X: worst angle 4.0e-8 rad over the 5 998 such points of the fixture -- the fp32 rounding of the three
    components written (the float64 solver itself is far below it).  A hundred times the measured value would be 4.0e-6;
    nothing looser than 1e-6 rad is asserted, so 1e-6 it is.  Elsewhere only a finite unit vector is asked for."""
    from miso_amd import ops
    f = ic.fixture()
    want, counts, gaps = ic.normals_reference()
    index = ops.NearestIndex(_dev(f["tgt"]))
    normals, got_counts = index.normals(radius=ic.NORMALS_RADIUS)
    assert normals.dtype == torch.float32 and normals.shape == (6000, 3) and got_counts.dtype == torch.int32
    assert np.array_equal(_host(got_counts), counts)
    n = _host(normals).astype(np.float64)
    assert np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    clear = gaps >= 0.05
    worst = _angles(n[clear], want[clear]).max()
    print(f"normals: worst angle {worst:.3e} rad over {clear.sum()} points with an eigen-gap >= 0.05")
    assert worst <= NORMALS_ASSERTED
    # another cloud against the index, and the default radius
    q = f["src"][:500]
    want_q, counts_q, gaps_q = ic.normals64(f["tgt"], q, ic.NORMALS_RADIUS)
    nq, cq = index.normals(_dev(q), radius=ic.NORMALS_RADIUS)
    assert np.array_equal(_host(cq), counts_q) and _angles(_host(nq)[gaps_q >= 0.05], want_q[gaps_q >= 0.05]).max() <= NORMALS_ASSERTED
    radius = ops.NN_NORMAL_SPACINGS * index.spacing
    assert 0.3 < radius < 0.5
    _, counts_d, _ = ic.normals64(f["tgt"], f["tgt"][:300], radius)
    assert np.array_equal(_host(index.normals()[1])[:300], counts_d)


@pytest.mark.gpu
def test_normals_fall_back_to_z():
    """fewer than three neighbours, or neighbours on a line: (0, 0, 1) and the count; a patch in the plane x = 5: (+-1, 0, 0)"""
    from miso_amd import ops
    k = np.arange(4) * 0.1
    patch = np.stack([np.full(16, 5.0), *[g.ravel() for g in np.meshgrid(k, k, indexing="ij")]], axis=1)
    line = np.array([[20.0, 0, 0], [20.1, 0, 0], [20.2, 0, 0]])
    tgt = np.concatenate([patch, [[10.0, 10.0, 10.0]], line, [[30.0, 0, 0], [30.0, 0.1, 0]]]).astype(np.float32)
    index = ops.NearestIndex(_dev(tgt), cell=0.2)
    normals, counts = (_host(t) for t in index.normals(radius=0.35))
    want_counts = ic.normals64(tgt, tgt, 0.35)[1]
    assert np.array_equal(counts, want_counts) and counts[16] == 1 and counts[17:20].tolist() == [3, 3, 3] and counts[20] == 2
    assert (normals[16:] == [0.0, 0.0, 1.0]).all()
    assert np.abs(np.abs(normals[:16, 0]) - 1.0).max() < 1e-6 and np.abs(normals[:16, 1:]).max() < 1e-6
    far, far_counts = index.normals(_dev(np.array([[100.0, 0, 0], [np.nan, 0, 0]])), radius=0.35)
    assert _host(far_counts).tolist() == [0, 0] and (_host(far) == [0.0, 0.0, 1.0]).all()
    empty = ops.NearestIndex(torch.empty((0, 3), device="cuda"))
    n0, c0 = empty.normals(_dev(tgt), radius=0.35)
    assert (_host(c0) == 0).all() and (_host(n0) == [0.0, 0.0, 1.0]).all()


# --------------------------------------------------------------------------- 5, 6. recovery
def _coarse_and_fine(f, kind, index=None):
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_registration as reg
    tgt, nrm = _dev(f["tgt"]), _dev(f["normals"])
    index = index or ops.NearestIndex(tgt)
    coarse = reg.registration_icp(_dev(f["src"]), index, tgt, nrm, ic.COARSE, np.eye(4), kind=kind)
    fine = reg.registration_icp(_dev(f["src"]), index, tgt, nrm, ic.FINE, coarse.transformation, kind=kind,
                                loss=reg.TukeyLoss(ic.TUKEY_K))
    return coarse, fine


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["point_to_plane", "point_to_point"])
def test_recovery_exact_case(kind):
    """The source is 5 000 of the target's own rows moved by the inverse of a 3 deg / 5 cm pose: at the optimum every
    residual is zero, what remains is the fp32 rounding of p' at 4 m (about 5e-7); the bound is ten times that with room
    for conditioning."""
    f = ic.exact_fixture()
    coarse, fine = _coarse_and_fine(f, kind)
    dt, dr = ic.pose_error(fine.transformation, f["pose"])
    print(f"{kind}: coarse {coarse}, fine {fine}, translation error {dt:.3e} m, rotation error {dr:.3e} rad")
    assert dt <= 1e-5 and dr <= 1e-5
    assert fine.fitness == 1.0 and coarse.fitness == 1.0 and fine.inlier_rmse < 1e-6
    assert fine.transformation.dtype == np.float64 and fine.transformation.shape == (4, 4) and 1 <= coarse.iterations <= 30


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["point_to_plane", "point_to_point"])
def test_recovery_independent_samplings(kind):
    """Source and target are independent samplings of the shape, the target with its face normals.  The GPU run is held
    to the truth, not to itself: it and icp_loop64 (float64, all-pairs) on the same clouds both land within twice what
    icp_loop64 reaches on the CPU (icp_cases.INDEPENDENT_REACHED; the margin covers correspondences flipped by fp32 p')."""
    f = ic.fixture()
    coarse, fine = _coarse_and_fine(f, kind)
    T64, fitness64, _, _, _ = ic.loop64("independent", kind)
    reached = ic.INDEPENDENT_REACHED[kind]
    for name, T in (("gpu", fine.transformation), ("float64", T64)):
        dt, dr = ic.pose_error(T, f["pose"])
        print(f"{kind} {name}: translation error {dt:.3e} m, rotation error {dr:.3e} rad")
        assert dt <= 2 * reached[0] and dr <= 2 * reached[1], name
    assert abs(fine.fitness - fitness64) < 0.01 and coarse.fitness == 1.0


# --------------------------------------------------------------------------- 7. meshes and submaps
def _meshes():
    from miso_amd.grid_opt.utils import utils_sdf
    v, tri = ic.shape_mesh()
    moved = utils_sdf.TriangleMesh(ic.apply64(np.linalg.inv(ic.pose(2.0, 0.04)), v), tri)
    return utils_sdf.TriangleMesh(v, tri), moved


def _tool():
    spec = importlib.util.spec_from_file_location("eval_mesh_tool", os.path.join(ROOT, "tools", "eval_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


# F-score at 1 cm of two samplings of 20 000 points of the fixture shape, measured in float64 on the CPU (ops.nearest
# replaced by icp_cases.nearest64, tools/eval_mesh.py otherwise as it is): 8.97 for the shape against itself, 1.45 with
# one of them moved by 2 deg / 4 cm.  An alignment is worth 7.5 points.  The test asks for 5.5: less the 1 point the first
# assertion allows, and 1 point for the device's other random stream (the deviation of a 9 % share of 20 000 is 0.2).
ALIGN_GAIN_MEASURED, ALIGN_GAIN_ASSERTED = 7.5, 5.5


@pytest.mark.gpu
def test_align_mesh_to_ref_and_the_eval_tool(tmp_path):
    from miso_amd.grid_opt.utils import utils_scannet
    gt, moved = _meshes()
    before = moved.vertices.copy()
    aligned, result = utils_scannet.align_mesh_to_ref(moved, gt, num_points=20000)
    assert np.array_equal(moved.vertices, before) and aligned is not moved              # a copy is returned
    dt, dr = ic.pose_error(result.transformation, ic.pose(2.0, 0.04))
    print(f"align_mesh_to_ref: {result}, translation error {dt:.3e} m, rotation error {dr:.3e} rad")
    assert dt < 2e-3 and dr < 1e-3 and np.abs(aligned.vertices - gt.vertices).max() < 8e-3
    _, point = utils_scannet.align_mesh_to_ref(moved, gt, constraint_type='point_to_point', num_points=20000)
    assert ic.pose_error(point.transformation, ic.pose(2.0, 0.04))[0] < 2e-2
    with pytest.raises(ValueError, match="Unknown constraint type"):
        utils_scannet.align_mesh_to_ref(moved, gt, constraint_type='plane')
    # the tool, from PLY files
    tool = _tool()
    gt.export_ply(str(tmp_path / "gt.ply"))
    moved.export_ply(str(tmp_path / "pred.ply"))
    common = ["--gt", str(tmp_path / "gt.ply"), "--points", "20000", "--voxel", "0.02", "--threshold", "0.01"]
    same = tool.main(["--pred", str(tmp_path / "gt.ply"), *common])
    plain = tool.main(["--pred", str(tmp_path / "pred.ply"), *common])
    with_align = tool.main(["--pred", str(tmp_path / "pred.ply"), *common, "--align", "--out", str(tmp_path / "m.json")])
    print("F-score at 1 cm: unmoved", same['F-score (%)'], "moved", plain['F-score (%)'], "aligned", with_align['F-score (%)'])
    assert with_align['F-score (%)'] >= same['F-score (%)'] - 1.0
    assert with_align['F-score (%)'] - plain['F-score (%)'] >= ALIGN_GAIN_ASSERTED
    assert json.loads((tmp_path / "m.json").read_text())['F-score (%)'] == pytest.approx(with_align['F-score (%)'])


@pytest.mark.gpu
def test_align_submap_pair_on_the_golden_atlas():
    import fusion_cases as fc
    from test_grid_opt_mirror import _OneBatch, make_atlas_two_kf
    from miso_amd.grid_opt.align import icp
    atlas = make_atlas_two_kf("cuda:0")
    mi, gt = fc.fusion_batch()

    class OnDevice(_OneBatch):
        def __getitem__(self, i):
            a, b = super().__getitem__(i)
            return {k: v.to("cuda:0") for k, v in a.items()}, {k: v.to("cuda:0") for k, v in b.items()}

    data = OnDevice(mi, gt)
    pts = icp.get_points_for_submap(atlas, data, 1, num_batches=1, trunc_dist=0.05)
    assert pts.ndim == 2 and pts.shape[1] == 3 and 20 < pts.shape[0] < 200 and pts.is_cuda
    before = [(r.detach().clone(), t.detach().clone()) for r, t in zip(atlas.rotation_corrections, atlas.translation_corrections)]
    # (the batch is points drawn in a volume with random SDF values, not a surface: thresholds of 4.5 m and 1.8 m keep most
    # pairs in, so that the six unknowns are determined; what is asked of the result is that it is a pose)
    kw = dict(voxel_size=0.3, threshold_factor_fine=6, num_batches=1, trunc_dist=0.05)
    result, info, times = icp.align_submap_pair(atlas, data, 0, 1, update_grid_atlas=False, **kw)
    print(f"align_submap_pair: {pts.shape[0]} points of submap 1, {result}")
    assert np.isfinite(result.transformation).all() and result.fitness > 0 and np.isfinite(result.inlier_rmse)
    assert np.allclose(result.transformation[:3, :3] @ result.transformation[:3, :3].T, np.eye(3), atol=1e-5)      # (the atlas' poses are fp32)
    assert info.shape == (6, 6) and np.isfinite(info).all() and np.allclose(info, info.T) and info[3, 3] >= 1
    assert set(times) == {'cpu_time_sec', 'gpu_time_sec'}
    for s in range(3):
        assert torch.equal(atlas.rotation_corrections[s], before[s][0]) and torch.equal(atlas.translation_corrections[s], before[s][1])
    result, _, _ = icp.align_submap_pair(atlas, data, 0, 1, update_grid_atlas=True, **kw)
    for s in (0, 2):
        assert torch.equal(atlas.rotation_corrections[s], before[s][0]) and torch.equal(atlas.translation_corrections[s], before[s][1])
    assert not torch.equal(atlas.translation_corrections[1], before[1][1])
    assert torch.isfinite(atlas.rotation_corrections[1]).all() and torch.isfinite(atlas.translation_corrections[1]).all()
    _, _, _ = icp.align_submap_pair(atlas, data, 0, 1, constraint_type='point_to_point', update_grid_atlas=False, **kw)
