"""Mesh metrics of grid_opt/utils/utils_eval.py (compute_chamfer_metrics, nn_correspondance, sample_points_from_mesh, the
filters), utils_sdf.read_ply and tools/eval_mesh.py.

CPU: the arithmetic of the metrics with ops.nearest replaced, in this file only, by a float64 all-pairs search; the
sampler's distribution; the PLY reader; the oriented box.  GPU: the same metrics through the HIP search, and the tool."""
import contextlib
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import nn_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ['MAE_accuracy (cm)', 'MAE_completeness (cm)', 'Chamfer_L1 (cm)', 'Chamfer_L2 (cm)', 'Precision (%)', 'Recall (%)',
        'F-score (%)']                                                   # the reference's, in its order


def nearest64(src, tgt, cell=None):
    """ops.nearest's contract on any device in float64: (d2 rounded to fp32, lowest index of the minimum), (inf, -1)
    without a match"""
    s, t = src.detach().cpu().to(torch.float64), tgt.detach().cpu().to(torch.float64)
    n, m = s.shape[0], t.shape[0]
    d2 = torch.full((n,), float("inf"), dtype=torch.float64)
    idx = torch.full((n,), -1, dtype=torch.int64)
    if m:
        for a in range(0, n, 1024):
            q = s[a:a + 1024]
            # (the direct form, no matrix product; argmin returns the first, i.e. lowest, index of the minimum)
            j = torch.cdist(q, t, compute_mode="donot_use_mm_for_euclid_dist").argmin(dim=1)
            diff = q - t[j]
            d2[a:a + 1024], idx[a:a + 1024] = (diff[:, 0] ** 2 + diff[:, 1] ** 2) + diff[:, 2] ** 2, j
    return d2.to(torch.float32).to(src.device), idx.to(src.device)


@contextlib.contextmanager
def float64_search():
    """ops.nearest = nearest64 inside the block; a search over the same two live arrays is done once"""
    from miso_amd import ops
    real, memo = ops.nearest, {}

    def remembered(src, tgt, cell=None):
        key = (src.data_ptr(), tuple(src.shape), tgt.data_ptr(), tuple(tgt.shape))
        if key not in memo:
            memo[key] = (src, tgt, nearest64(src, tgt))                  # (the arrays are kept alive with their key)
        return memo[key][2]

    ops.nearest = remembered
    try:
        yield
    finally:
        ops.nearest = real


@functools.lru_cache(maxsize=None)
def sphere_clouds():
    """20 000 surface samples each of icospheres (5120 faces) of radius 0.50 (the prediction) and 0.52, fp32"""
    from miso_amd.grid_opt.utils import utils_eval
    out = []
    for radius, seed in ((0.50, 11), (0.52, 12)):
        v, f = nc.icosphere(radius, 4)
        assert len(f) == 5120
        pts, _, _ = utils_eval.sample_surface(torch.from_numpy(v), torch.from_numpy(f), 20000,
                                              torch.Generator().manual_seed(seed))
        out.append(np.ascontiguousarray(pts.numpy(), dtype=np.float32))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _sphere_metrics_float64():
    from miso_amd.grid_opt.utils import utils_eval
    pred, gt = (torch.from_numpy(a) for a in sphere_clouds())
    with float64_search():
        return {th: utils_eval.compute_chamfer_metrics(pred, gt, threshold=th) for th in (0.05, 0.01)}


def sphere_metrics_float64(threshold):
    return _sphere_metrics_float64()[threshold]


def plane(n=40, spacing=0.05, z=0.0):
    k = np.arange(n) * spacing
    x, y = np.meshgrid(k, k, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(n * n, z)], axis=1).astype(np.float32)


# --------------------------------------------------------------------------- CPU
def test_chamfer_metrics_of_two_spheres():
    """Radius 0.50 against 0.52: every distance is at least |dr| less the sag of a chord (an icosphere's faces lie up to
    0.52 (1 - cos(edge / 2)) ~ 0.5 mm inside the sphere) and at most sqrt(0.02^2 + s^2) with the sample spacing
    s ~ sqrt(4 pi 0.52^2 / 20000) = 1.3 cm."""
    at5, at1 = sphere_metrics_float64(0.05), sphere_metrics_float64(0.01)
    assert list(at5) == KEYS and list(at1) == KEYS
    for m in (at5, at1):
        assert 1.9 <= m['MAE_accuracy (cm)'] <= 2.6 and 1.9 <= m['MAE_completeness (cm)'] <= 2.6
    assert at5['Precision (%)'] == 100.0 and at5['Recall (%)'] == 100.0
    assert at5['F-score (%)'] == pytest.approx(100.0, rel=1e-9)
    assert at1['Precision (%)'] == 0.0 and at1['Recall (%)'] == 0.0 and at1['F-score (%)'] == 0.0
    assert at5['Chamfer_L1 (cm)'] == pytest.approx(0.5 * (at5['MAE_accuracy (cm)'] + at5['MAE_completeness (cm)']), rel=1e-12)


def test_chamfer_metrics_closed_form_on_a_shifted_plane(monkeypatch):
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_eval
    monkeypatch.setattr(ops, "nearest", nearest64)
    delta = 0.03
    gt, pred = plane(z=0.0), plane(z=delta)
    d = float(np.float32(delta))
    want = {'MAE_accuracy (cm)': 100 * d, 'MAE_completeness (cm)': 100 * d, 'Chamfer_L1 (cm)': 100 * d,
            'Chamfer_L2 (cm)': 100 * np.sqrt(d), 'Precision (%)': 100.0, 'Recall (%)': 100.0,
            'F-score (%)': 2 * 100.0 * 100.0 / (200.0 + 1e-8)}
    got = utils_eval.compute_chamfer_metrics(pred, gt, threshold=0.05)
    assert list(got) == KEYS
    for k in KEYS:
        assert got[k] == pytest.approx(want[k], rel=1e-6), k
    # the same through tensors
    got_t = utils_eval.compute_chamfer_metrics(torch.from_numpy(pred), torch.from_numpy(gt), threshold=0.05)
    assert got_t == got
    # `<`, not `<=`: at a threshold equal to the distance nothing counts
    at = utils_eval.compute_chamfer_metrics(pred, gt, threshold=float(np.sqrt(np.float32(np.float32(delta) ** 2))))
    assert at['Precision (%)'] == 0.0 and at['Recall (%)'] == 0.0
    # 10 % of the prediction 1 m away: dropped from the accuracy (beyond truncation_acc), and no ground-truth point's
    # neighbour, so the completeness does not move either
    rng = np.random.default_rng(5)
    outliers = plane(z=delta)[rng.choice(1600, 160, replace=False)] + np.array([0.0, 0.0, 1.0], dtype=np.float32)
    with_out = utils_eval.compute_chamfer_metrics(np.concatenate([pred, outliers]), gt, threshold=0.05)
    for k in KEYS:
        assert with_out[k] == pytest.approx(want[k], rel=1e-6), k
    # ... while a truncation that keeps them moves the accuracy only
    kept = utils_eval.compute_chamfer_metrics(np.concatenate([pred, outliers]), gt, threshold=0.05, truncation_acc=2.0)
    assert kept['MAE_accuracy (cm)'] > 10.0 and kept['MAE_completeness (cm)'] == pytest.approx(100 * d, rel=1e-6)
    assert kept['Precision (%)'] == pytest.approx(100.0 * 1600 / 1760, rel=1e-12)
    # an empty prediction
    none = utils_eval.compute_chamfer_metrics(np.zeros((0, 3), dtype=np.float32), gt, threshold=0.05)
    assert list(none) == KEYS
    assert none['MAE_accuracy (cm)'] == np.inf and none['MAE_completeness (cm)'] == np.inf
    assert none['Chamfer_L1 (cm)'] == np.inf and none['Chamfer_L2 (cm)'] == np.inf
    assert none['Precision (%)'] == 0 and none['Recall (%)'] == 0 and none['F-score (%)'] == 0


def test_nn_correspondance_lists_and_truncation(monkeypatch):
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_eval
    monkeypatch.setattr(ops, "nearest", nearest64)
    tgt = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], dtype=np.float64)
    src = np.array([[0.1, 0, 0], [0.9, 0, 0], [0, 5, 0], [0.5, 0, 0]], dtype=np.float64)
    idx, dist = utils_eval.nn_correspondance(src, tgt)
    assert isinstance(idx, list) and isinstance(dist, list) and idx == [0, 1, 2, 0]          # the tie goes to index 0
    assert dist == pytest.approx([0.1, 0.1, 3.0, 0.5], rel=1e-6)
    idx, dist = utils_eval.nn_correspondance(src, tgt, truncation=0.5)                         # no mask without remove_far
    assert len(idx) == 4
    idx, dist = utils_eval.nn_correspondance(src, tgt, truncation=0.5, remove_far=True)       # `<=`
    assert idx == [0, 1, 0] and dist == pytest.approx([0.1, 0.1, 0.5], rel=1e-6)


def test_surface_samples_follow_the_area_and_lie_in_their_triangle():
    from miso_amd.grid_opt.utils import utils_eval, utils_sdf
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 2], [0, 2, 1.5]], dtype=np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    v[3:] = v[3] + (v[3:] - v[3]) * np.sqrt(3.0 * area[0] / area[1])      # areas 1 : 3
    n = 40000
    pts, face, bary = utils_eval.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, torch.Generator().manual_seed(3))
    pts, face, bary = pts.numpy(), face.numpy(), bary.numpy()
    assert abs((face == 0).mean() - 0.25) <= 0.011                       # 5 sigma of the binomial: 5 sqrt(.25 .75 / n)
    assert (bary >= 0.0).all() and (bary <= 1.0).all() and np.abs(bary.sum(axis=1) - 1.0).max() < 1e-12
    normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    off = np.abs(((pts - v[f[face, 0]]) * normal[face]).sum(axis=1))
    assert off.max() <= 1e-6
    # uniform inside a face: the mean of the barycentric coordinates is 1/3 each (sigma = sqrt(1 / 18 / n))
    assert np.abs(bary[face == 1].mean(axis=0) - 1.0 / 3.0).max() < 5 * np.sqrt(1.0 / 18.0 / (0.75 * n))
    mesh = utils_sdf.TriangleMesh(v, f)
    a = utils_eval.sample_points_from_mesh(mesh, mesh_sample_point=5000, voxel_down_sample_res=0, seed=7)
    b = utils_eval.sample_points_from_mesh(mesh, mesh_sample_point=5000, voxel_down_sample_res=0, seed=7)
    c = utils_eval.sample_points_from_mesh(mesh, mesh_sample_point=5000, voxel_down_sample_res=0, seed=8)
    assert isinstance(a, np.ndarray) and a.shape == (5000, 3) and (a == b).all() and not (a == c).all()
    cloud = utils_eval.sample_points_from_mesh(mesh, input_format='pointcloud', voxel_down_sample_res=0)
    assert np.allclose(cloud, v)
    with pytest.raises(ValueError):
        utils_eval.sample_points_from_mesh(mesh, input_format='volume')


def test_centroid_down_sample_on_a_dyadic_lattice():
    """Points k / 8, k = 0..7 per axis, voxels of 1/4 from the origin min - 1/8: per axis the groups {0}, {1,2}, {3,4},
    {5,6}, {7}, so 125 voxels whose centroids are products of (0, 3/16, 7/16, 11/16, 7/8) -- all exact in binary."""
    from miso_amd.grid_opt.utils import utils_eval, utils_geometry, utils_sdf
    k = np.arange(8) / 8.0
    pts = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(0)
    pts = pts[rng.permutation(len(pts))]
    out = utils_geometry.voxel_centroid_down_sample(torch.from_numpy(pts), 0.25).numpy()
    axis = np.array([0.0, 3 / 16, 7 / 16, 11 / 16, 7 / 8])
    want = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)
    assert out.shape == (125, 3)
    assert (out[np.lexsort(out.T[::-1])] == want[np.lexsort(want.T[::-1])]).all()
    via = utils_eval.sample_points_from_mesh(utils_sdf.TriangleMesh(pts, np.zeros((0, 3))), input_format='pointcloud',
                                             voxel_down_sample_res=0.25)
    assert via.shape == (125, 3) and (via[np.lexsort(via.T[::-1])] == want[np.lexsort(want.T[::-1])]).all()
    assert utils_geometry.voxel_centroid_down_sample(torch.zeros(0, 3), 0.25).shape == (0, 3)


def test_read_ply_formats(tmp_path):
    from miso_amd.grid_opt.utils import utils_sdf
    v, f = nc.icosphere(0.5, 1)
    mesh = utils_sdf.TriangleMesh(v, f)
    mesh.export_ply(str(tmp_path / "own.ply"))
    back = utils_sdf.read_ply(str(tmp_path / "own.ply"))
    assert (back.triangles == f).all() and (back.vertices == v.astype(np.float32).astype(np.float64)).all()
    # ascii, colours between and behind the coordinates, a comment, an int-counted face list with a property behind it
    (tmp_path / "a.ply").write_text(
        "ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty float x\nproperty uchar red\n"
        "property float y\nproperty float z\nproperty uchar green\nproperty uchar blue\nproperty double quality\n"
        "element face 2\nproperty list uchar int vertex_indices\nproperty uchar flags\nend_header\n"
        "0 255 0 0 0 0 0.5\n1 0 0 0 255 0 0.25\n0 0 1 0 0 255 1e-3\n0 9 0 1.5 1 2 -2\n3 0 1 2 7\n3 0 2 3 9\n")
    a = utils_sdf.read_ply(tmp_path / "a.ply")
    assert (a.vertices == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]]).all() and (a.triangles == [[0, 1, 2], [0, 2, 3]]).all()
    # binary little endian with ScanNet's layout: float xyz, uchar rgba; faces uchar-counted int lists
    vert = np.zeros(4, dtype=[('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('r', 'u1'), ('g', 'u1'), ('b', 'u1'), ('a', 'u1')])
    vert['x'], vert['y'], vert['z'], vert['r'] = [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.5], 200
    face = np.zeros(2, dtype=[('n', 'u1'), ('idx', '<i4', (3,))])
    face['n'], face['idx'] = 3, [[0, 1, 2], [0, 2, 3]]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
              "element face 2\nproperty list uchar int vertex_indices\nend_header\n")
    (tmp_path / "b.ply").write_bytes(header.encode() + vert.tobytes() + face.tobytes())
    b = utils_sdf.read_ply(str(tmp_path / "b.ply"))
    assert (b.vertices == a.vertices).all() and (b.triangles == a.triangles).all()
    # double coordinates, short extras, ushort-counted uint lists
    vert = np.zeros(3, dtype=[('nx', '<i2'), ('x', '<f8'), ('y', '<f8'), ('z', '<f8')])
    vert['x'], vert['y'] = [0, 1, 0], [0, 0, 1]
    face = np.zeros(1, dtype=[('n', '<u2'), ('idx', '<u4', (3,))])
    face['n'], face['idx'] = 3, [[2, 1, 0]]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty short nx\nproperty double x\n"
              "property double y\nproperty double z\nelement face 1\nproperty list ushort uint vertex_index\nend_header\n")
    (tmp_path / "d.ply").write_bytes(header.encode() + vert.tobytes() + face.tobytes())
    d = utils_sdf.read_ply(tmp_path / "d.ply")
    assert (d.vertices == [[0, 0, 0], [1, 0, 0], [0, 1, 0]]).all() and (d.triangles == [[2, 1, 0]]).all()
    # a point cloud: no face element
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
    (tmp_path / "c.ply").write_bytes(header.encode() + np.arange(9, dtype='<f4').tobytes())
    c = utils_sdf.read_ply(tmp_path / "c.ply")
    assert (c.vertices == np.arange(9).reshape(3, 3)).all() and c.triangles.shape == (0, 3)
    (tmp_path / "ca.ply").write_text("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\n"
                                     "property float z\nend_header\n1 2 3\n4 5 6\n")
    assert (utils_sdf.read_ply(tmp_path / "ca.ply").vertices == [[1, 2, 3], [4, 5, 6]]).all()
    # refusals: a quad (ascii and binary), big endian, a list on the vertices, an unskippable element, not a PLY
    (tmp_path / "q.ply").write_text("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                                    "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
                                    "0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    quad = np.zeros(1, dtype=[('n', 'u1'), ('idx', '<i4', (4,))])
    quad['n'] = 4
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
              "element face 1\nproperty list uchar int vertex_indices\nend_header\n")
    (tmp_path / "qb.ply").write_bytes(header.encode() + np.zeros(3, dtype='<f4').tobytes() + quad.tobytes())
    (tmp_path / "be.ply").write_bytes(header.replace("little", "big").encode() + bytes(12 + 13))
    (tmp_path / "vl.ply").write_text("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                                     "property list uchar int neighbours\nend_header\n0 0 0 1 0\n")
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
              "element edge_loops 1\nproperty list uchar int loop\nend_header\n")
    (tmp_path / "el.ply").write_bytes(header.encode() + bytes(12 + 5))
    (tmp_path / "no.ply").write_text("solid stl\n")
    for name in ("q.ply", "qb.ply", "be.ply", "vl.ply", "el.ply", "no.ply"):
        with pytest.raises(ValueError):
            utils_sdf.read_ply(tmp_path / name)


def test_box_mesh_is_the_surface_of_its_box():
    from miso_amd.grid_opt.utils import utils_eval, utils_sdf
    bound = np.array([[0.0, 8.0], [-1.0, 5.0], [0.5, 3.5]])
    mesh = utils_sdf.box_mesh(bound)
    v, f = mesh.vertices, mesh.triangles
    assert v.shape == (8, 3) and f.shape == (12, 3)
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    assert area.sum() == pytest.approx(2 * (8 * 6 + 6 * 3 + 3 * 8))
    pts = utils_eval.sample_points_from_mesh(mesh, mesh_sample_point=4000, voxel_down_sample_res=0, seed=1)
    on_face = (np.abs(pts[:, :, None] - bound[None, :, :]) < 1e-9).any(axis=(1, 2))
    inside = ((pts >= bound[:, 0] - 1e-9) & (pts <= bound[:, 1] + 1e-9)).all(axis=1)
    assert on_face.all() and inside.all()
    for a in range(3):                                                 # every face gets its share
        for side in range(2):
            assert (np.abs(pts[:, a] - bound[a, side]) < 1e-9).sum() > 200


def test_oriented_box_and_filters():
    from miso_amd.grid_opt.utils import utils_eval
    ang = 0.7
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    centre, extent = np.array([1.0, -2.0, 0.5]), np.array([2.0, 1.0, 0.5])
    box = utils_eval.OrientedBox(centre, R, extent)
    pts, inside = [centre], [True]
    for a in range(3):
        for sign in (-1.0, 1.0):
            for eps, ok in ((-1e-3, True), (1e-3, False)):             # just inside and just outside every face
                pts.append(centre + R[:, a] * sign * (0.5 * extent[a] + eps))
                inside.append(ok)
    pts = np.asarray(pts)
    got = box.get_point_indices_within_bounding_box(pts)
    assert got == [i for i, ok in enumerate(inside) if ok]
    assert (utils_eval.filter_points_by_oriented_bound(pts, box) == pts[got]).all()
    # the PCA box of a rotated slab contains every point and has the slab's extents, longest first
    rng = np.random.default_rng(2)
    cloud = centre + (rng.uniform(-0.5, 0.5, (4000, 3)) * extent) @ R.T
    pca = utils_eval.OrientedBox.from_points(cloud)
    assert len(pca.get_point_indices_within_bounding_box(cloud * (1 - 1e-12) + centre * 1e-12)) == 4000
    assert np.allclose(pca.extent, extent, atol=0.06) and np.linalg.det(pca.R) == pytest.approx(1.0)
    grown = utils_eval.OrientedBox.from_points(cloud, buffer=0.1)
    assert np.allclose(grown.extent, pca.extent + 0.2)
    # the axis-aligned filter keeps its borders; the SDF filter applies the lower threshold only (as upstream)
    p = np.array([[0, 0, 0], [1, 1, 1], [1.0001, 0, 0], [0.5, 0.5, 0.5]])
    assert (utils_eval.filter_points_by_bound(p, [[0, 1], [0, 1], [0, 1]]) == p[[0, 1, 3]]).all()
    sdf = lambda q: q[:, 0] - 0.75                                      # noqa: E731
    assert (utils_eval.filter_points_by_gt_sdf(p, sdf, min_sdf=0.0, max_sdf=0.1) == p[[1, 2]]).all()


# --------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_device_metrics_equal_the_float64_run():
    """The spheres of the CPU test through ops.nearest on the device: the counts (precision, recall) are exact, the means
    agree to 1e-6 relative (an fp32 d2 is within 2^-21 of the true one)."""
    from miso_amd.grid_opt.utils import utils_eval
    pred, gt = sphere_clouds()
    for threshold in (0.05, 0.01):
        want = sphere_metrics_float64(threshold)
        for clouds in ((pred, gt), (torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())):
            got = utils_eval.compute_chamfer_metrics(*clouds, threshold=threshold)
            assert list(got) == KEYS
            assert got['Precision (%)'] == want['Precision (%)'] and got['Recall (%)'] == want['Recall (%)']
            for k in KEYS:
                assert got[k] == pytest.approx(want[k], rel=1e-6), k
    idx, dist = utils_eval.nn_correspondance(pred[:500], gt, truncation=0.5, remove_far=True)
    with float64_search():
        idx64, dist64 = utils_eval.nn_correspondance(pred[:500], gt, truncation=0.5, remove_far=True)
    assert idx == idx64 and dist == pytest.approx(dist64, rel=1e-6)


@pytest.mark.gpu
def test_eval_mesh_tool_writes_the_seven_metrics(tmp_path):
    from miso_amd.grid_opt.utils import utils_sdf
    for radius, name in ((0.50, "pred.ply"), (0.52, "gt.ply")):
        utils_sdf.TriangleMesh(*nc.icosphere(radius, 3)).export_ply(str(tmp_path / name))
    spec = importlib.util.spec_from_file_location("eval_mesh_tool", os.path.join(ROOT, "tools", "eval_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "metrics.json"
    tool.main(["--pred", str(tmp_path / "pred.ply"), "--gt", str(tmp_path / "gt.ply"), "--points", "20000", "--voxel", "0.02",
               "--threshold", "0.05", "--out", str(out)])
    got = json.loads(out.read_text())
    assert list(got) == KEYS and all(np.isfinite(v) for v in got.values())
    assert 1.5 <= got['MAE_accuracy (cm)'] <= 3.0 and got['Precision (%)'] == 100.0
