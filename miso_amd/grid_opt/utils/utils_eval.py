"""Trajectory error metrics the alignment demo prints (reference: grid_opt/utils/utils_eval.py:110-147, which wraps the
``evo`` package).  ``evo`` is not a dependency here: the absolute pose error after a rigid (Umeyama, no scale)
alignment is ~40 lines of numpy.  Same call signature and the same ``get_all_statistics()`` keys as evo's APE.

Mesh metrics (reference :14-108): ``nn_correspondance``, ``sample_points_from_mesh``, the three point filters and
``compute_chamfer_metrics`` with the reference's names and signatures.  The reference leans on pytorch3d (knn_points),
trimesh and Open3D; here the nearest-neighbour search is ``ops.nearest`` (csrc/nn.hip, HIP device only), sampling and
the centroid down-sample are torch ops, and ``OrientedBox`` stands in for the Open3D box the demo crops with."""
import enum

import numpy as np
import torch

from . import utils_geometry
from . import utils_sdf
from miso_amd import ops


class PoseRelation(enum.Enum):
    """The members of evo.core.metrics.PoseRelation the reference uses (demo/align_submaps.py:134-137)."""
    full_transformation = "full transformation"
    translation_part = "translation part"
    rotation_part = "rotation part"
    rotation_angle_rad = "rotation angle in radians"
    rotation_angle_deg = "rotation angle in degrees"


def _relation_name(pose_relation) -> str:
    return getattr(pose_relation, "name", str(pose_relation))      # ours or evo's enum: same member names


def umeyama_rigid(src: np.ndarray, dst: np.ndarray):
    """R (3,3), t (3,) minimising sum |R src_i + t - dst_i|^2 (Umeyama 1991 without scale)."""
    mu_s, mu_d = src.mean(axis=0), dst.mean(axis=0)
    cov = (dst - mu_d).T @ (src - mu_s) / src.shape[0]
    U, _, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    return R, mu_d - R @ mu_s


class APE:
    """Absolute pose error of a trajectory against a reference one, per pose; statistics like evo's APE."""

    def __init__(self, pose_relation=PoseRelation.translation_part):
        self.pose_relation = pose_relation
        self.error = np.zeros(0)

    def process_data(self, data):
        ref, est = data                                           # lists of 4x4
        rel = _relation_name(self.pose_relation)
        errs = []
        for P, Q in zip(ref, est):
            E = np.linalg.inv(P) @ Q
            if rel == "translation_part":
                errs.append(np.linalg.norm(E[:3, 3]))
            elif rel == "rotation_part":
                errs.append(np.linalg.norm(E[:3, :3] - np.eye(3)))
            elif rel == "full_transformation":
                errs.append(np.linalg.norm(E - np.eye(4)))
            elif rel in ("rotation_angle_rad", "rotation_angle_deg"):
                ang = np.arccos(np.clip((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))
                errs.append(np.degrees(ang) if rel.endswith("deg") else ang)
            else:
                raise ValueError(f"unsupported pose relation {self.pose_relation}")
        self.error = np.asarray(errs, dtype=np.float64)

    def get_all_statistics(self):
        e = self.error
        return {"rmse": float(np.sqrt(np.mean(e ** 2))), "mean": float(np.mean(e)), "median": float(np.median(e)),
                "std": float(np.std(e)), "min": float(np.min(e)), "max": float(np.max(e)), "sse": float(np.sum(e ** 2))}


def get_evo_trajectory(R, t):
    """(n,3,3), (n,3[,1]) tensors -> list of 4x4 numpy poses (the reference returns an evo PosePath3D)."""
    return [utils_geometry.pose_matrix(R[i], t[i].reshape(3, 1)).detach().cpu().numpy().astype(np.float64)
            for i in range(R.shape[0])]


def evo_trajectory_error(R1, t1, R2, t2, pose_relation=PoseRelation.translation_part, align: bool = True) -> APE:
    """Reference :125-147: optionally align trajectory 2 to trajectory 1 rigidly, then the absolute pose error."""
    path1, path2 = get_evo_trajectory(R1, t1), get_evo_trajectory(R2, t2)
    if align:
        Ra, ta = umeyama_rigid(np.stack([P[:3, 3] for P in path2]), np.stack([P[:3, 3] for P in path1]))
        A = np.eye(4)
        A[:3, :3], A[:3, 3] = Ra, ta
        path2 = [A @ P for P in path2]
    ape = APE(pose_relation)
    ape.process_data((path1, path2))
    return ape


# --------------------------------------------------------------------------- mesh metrics (reference :14-108)
def _device():
    return torch.device("cuda:0" if torch.cuda.is_available() else "cpu")


def _cloud_tensor(points) -> torch.Tensor:
    """numpy array or tensor -> (N, 3) fp32 on the HIP device (ops.nearest refuses a CPU tensor: there is no fallback)"""
    t = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32))
    return t.detach().to(device=_device(), dtype=torch.float32).reshape(-1, 3)


def _nn_distances(src, tgt, truncation=None, remove_far=False):
    """(nearest index, distance = sqrt(d2) in fp32) of every src point among tgt, as tensors; with ``remove_far`` only
    the pairs with distance <= truncation."""
    d2, idx = ops.nearest(_cloud_tensor(src), _cloud_tensor(tgt))
    dist = torch.sqrt(d2)
    if truncation is not None and remove_far:
        keep = dist <= truncation
        dist, idx = dist[keep], idx[keep]
    return idx, dist


def nn_correspondance(src_points, tgt_points, truncation=None, remove_far=False):
    """Reference :14-36: -> (nn_idx_list, dist_list), Python lists as upstream."""
    idx, dist = _nn_distances(src_points, tgt_points, truncation, remove_far)
    return idx.cpu().numpy().tolist(), dist.cpu().numpy().tolist()


def compute_chamfer_metrics(verts_pred, verts_trgt, threshold=0.01, truncation_acc=0.50, truncation_com=0.50):
    """Reference :74-108, particulars kept: prediction -> ground-truth distances beyond ``truncation_acc`` are dropped
    while ground truth -> prediction distances are all kept (``truncation_com`` is passed with remove_far=False
    upstream, so it has no effect); means in float64 over fp32 distances; precision / recall with ``<``;
    Chamfer_L2 is the root of the mean of DISTANCES; an empty set gives inf means and 0 precision / recall.
    Takes numpy arrays or tensors; the distances stay tensors until the seven numbers are formed."""
    _, dist_p = _nn_distances(verts_pred, verts_trgt, truncation_acc, True)       # pred -> GT
    _, dist_r = _nn_distances(verts_trgt, verts_pred, truncation_com, False)      # GT -> pred

    def mean_and_share(d):
        if d.numel() == 0:
            return np.inf, 0
        d64 = d.to(torch.float64)
        return float(d64.mean().item()), float((d64 < threshold).to(torch.float64).mean().item()) * 100.0

    dist_p_mean, precision = mean_and_share(dist_p)
    dist_r_mean, recall = mean_and_share(dist_r)
    chamfer_l1 = 0.5 * (dist_p_mean + dist_r_mean)
    chamfer_l2 = np.sqrt(0.5 * (dist_p_mean + dist_r_mean))
    fscore = 2 * precision * recall / (precision + recall + 1e-8)
    return {
        'MAE_accuracy (cm)': dist_p_mean * 100,
        'MAE_completeness (cm)': dist_r_mean * 100,
        'Chamfer_L1 (cm)': chamfer_l1 * 100,
        'Chamfer_L2 (cm)': chamfer_l2 * 100,
        'Precision (%)': precision,
        'Recall (%)': recall,
        'F-score (%)': fscore,
    }


def sample_surface(vertices: torch.Tensor, triangles: torch.Tensor, count: int, generator=None):
    """``count`` points on a triangle mesh: faces drawn with probability proportional to their area, uniform barycentric
    coordinates inside a face (the square-root map).  -> (points (count, 3), face index (count,), barycentric (count, 3))
    on the device of ``vertices``; computed in float64."""
    v = vertices.to(torch.float64)
    a, b, c = (v[triangles[:, k]] for k in range(3))
    area = 0.5 * torch.linalg.norm(torch.cross(b - a, c - a, dim=1), dim=1)
    cdf = torch.cumsum(area, dim=0)
    u = torch.rand((count, 3), dtype=torch.float64, device=v.device, generator=generator)
    face = torch.searchsorted(cdf, u[:, 0] * cdf[-1], right=True).clamp_(max=triangles.shape[0] - 1)
    s = torch.sqrt(u[:, 1])
    bary = torch.stack((1.0 - s, s * (1.0 - u[:, 2]), s * u[:, 2]), dim=1)
    pts = bary[:, 0:1] * a[face] + bary[:, 1:2] * b[face] + bary[:, 2:3] * c[face]
    return pts, face, bary


def sample_points_from_mesh(mesh_file, mesh_sample_point=1000000, voxel_down_sample_res=0.02, input_format='mesh',
                            seed=0):
    """Reference :38-50.  ``mesh_file``: a PLY path or a utils_sdf.TriangleMesh.  'mesh': ``mesh_sample_point`` surface
    samples (sample_surface, torch's generator seeded with ``seed``); 'pointcloud': the vertices.  Then, for
    ``voxel_down_sample_res`` > 0, Open3D's voxel_down_sample (utils_geometry.voxel_centroid_down_sample).  Runs on the
    device when there is one.  -> (N, 3) numpy float64 array.  Neither the random stream nor the order of the output is
    trimesh's or Open3D's: the same mesh gives a different, equally distributed cloud."""
    mesh = utils_sdf.read_ply(mesh_file) if isinstance(mesh_file, (str, bytes)) or hasattr(mesh_file, '__fspath__') \
        else mesh_file
    dev = _device()
    verts = torch.from_numpy(np.asarray(mesh.vertices, dtype=np.float64)).to(dev)
    if input_format == 'mesh':
        tris = torch.from_numpy(np.asarray(mesh.triangles, dtype=np.int64)).to(dev)
        if tris.shape[0] == 0:
            raise ValueError("sample_points_from_mesh: the mesh has no triangles (input_format='pointcloud'?)")
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        points, _, _ = sample_surface(verts, tris, int(mesh_sample_point), gen)
    elif input_format == 'pointcloud':
        points = verts
    else:
        raise ValueError(f"Unknown input format {input_format}!")
    if voxel_down_sample_res > 0:
        points = utils_geometry.voxel_centroid_down_sample(points, voxel_down_sample_res)
    return points.cpu().numpy()


def filter_points_by_bound(points, bound):
    """Reference :52-58: the points inside the axis-aligned ``bound`` (3, 2), borders included."""
    mask = (
        (points[:, 0] >= bound[0][0]) & (points[:, 0] <= bound[0][1]) &
        (points[:, 1] >= bound[1][0]) & (points[:, 1] <= bound[1][1]) &
        (points[:, 2] >= bound[2][0]) & (points[:, 2] <= bound[2][1])
    )
    return points[mask]


class OrientedBox:
    """What filter_points_by_oriented_bound needs of open3d.geometry.OrientedBoundingBox: ``center`` (3,), ``R`` (3, 3)
    whose columns are the box axes, ``extent`` (3,) full edge lengths."""

    def __init__(self, center, R, extent):
        self.center = np.asarray(center, dtype=np.float64).reshape(3)
        self.R = np.asarray(R, dtype=np.float64).reshape(3, 3)
        self.extent = np.asarray(extent, dtype=np.float64).reshape(3)

    @classmethod
    def from_points(cls, points, buffer=0.0):
        """The box along the principal axes of ``points`` (PCA of the covariance) that contains them all, grown by
        ``buffer`` on every side.  NOT Open3D's minimal oriented box (get_minimal_oriented_bounding_box searches the
        convex hull for the smallest volume): for a room scan it is close, in general it is larger."""
        p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        mean = p.mean(axis=0)
        _, vecs = np.linalg.eigh(np.cov((p - mean).T))
        R = vecs[:, ::-1].copy()
        if np.linalg.det(R) < 0:
            R[:, 2] = -R[:, 2]
        local = (p - mean) @ R
        lo, hi = local.min(axis=0) - buffer, local.max(axis=0) + buffer
        return cls(mean + R @ (0.5 * (lo + hi)), R, hi - lo)

    def get_point_indices_within_bounding_box(self, points):
        local = (np.asarray(points, dtype=np.float64).reshape(-1, 3) - self.center) @ self.R
        return np.nonzero((np.abs(local) <= 0.5 * self.extent).all(axis=1))[0].tolist()


def filter_points_by_oriented_bound(points, obb):
    """Reference :60-66; ``obb``: anything with get_point_indices_within_bounding_box (an OrientedBox, an Open3D box)."""
    valid_indices = obb.get_point_indices_within_bounding_box(points)
    return points[valid_indices, :]


def filter_points_by_gt_sdf(points, gt_sdf_func, min_sdf=-1e5, max_sdf=1e5):
    """Reference :68-72 (only the lower threshold is applied there, and here)."""
    sdf_vals = gt_sdf_func(points)[:, None].astype(np.float32).flatten()
    return points[sdf_vals > min_sdf, :]
