"""ScanNet scene metadata and the RGB-D dataset factory the demos call (reference:
grid_opt/utils/utils_scannet.py:10-113).  ``create_scannet_dataset`` builds the device-resident ``PosedSdfRgbd`` of
miso_amd.grid_opt.datasets.sdf_rgbd from the same files the reference reads (``<root>/scene<id>/scene<id>.txt``,
``frames/pose/*.pose.txt``, ``frames/depth/*.depth.pgm``).  ``align_mesh_to_ref`` (reference :115-156, an Open3D
registration pipeline) is the second step of the demo's mesh grading: coarse and fine ICP of the reconstruction onto the
ground truth, here on ops.NearestIndex and the kernels of csrc/icp.hip (utils_registration.registration_icp).
utils_ncd.align_mesh_to_ref shares its two passes (``icp_coarse_then_fine``)."""
import copy
import logging
from dataclasses import dataclass
from os.path import join

import numpy as np
import torch

from miso_amd.grid_opt.datasets.sdf_rgbd import PosedSdfRgbd
from miso_amd.grid_opt.utils.utils_data import CameraParameters

logger = logging.getLogger(__name__)


@dataclass
class SceneMetadata:
    bound: list
    name: str
    path: str
    intrinsics_file: str
    gt_mesh: str
    num_kfs: int
    anchor_kfs: list


# (bound, num_kfs, anchor_kfs) per scene, reference :21-64
_SCENES = {
    '0000_00': ([[-0.02, 10.38], [-0.01, 8.74], [-0.01, 3.03]], 372, [0, 124, 255]),
    '0011_00': ([[1.50, 7.50], [-0.05, 8.25], [-0.05, 2.70]], 159, [0, 73, 86, 121]),
    '0024_00': ([[0.00, 7.20], [-0.05, 8.05], [-0.05, 2.50]], 227, [0, 30, 84, 101, 131]),
    '0207_00': ([[1.00, 9.00], [0.00, 7.10], [-0.10, 2.90]], 133, [0, 35]),
}


def scannet_scenes():
    out = {}
    for sid, (bound, num_kfs, anchors) in _SCENES.items():
        root = f"./data/ScanNet/scene{sid}_mipsfusion"
        out[sid] = SceneMetadata(name=sid, path=root, intrinsics_file=f"{root}/scene{sid}.txt",
                                 gt_mesh=f"/home/hanwen/data/ScanNet/scans/scene{sid}/scene{sid}_vh_clean.ply",
                                 bound=[list(b) for b in bound], num_kfs=num_kfs, anchor_kfs=list(anchors))
    return out


def get_scannet_metadata(file):
    """``key = value`` lines of a ScanNet scene file -> dict of strings."""
    info = {}
    with open(file, 'r') as f:
        for line in f.read().splitlines():
            parts = line.split(' = ')
            if len(parts) == 2:
                info[parts[0]] = parts[1]
    return info


def get_scannet_cam_intrinsics(file) -> CameraParameters:
    info = get_scannet_metadata(file)
    return CameraParameters(depth_scale=1000.0, fx=float(info['fx_depth']), fy=float(info['fy_depth']),
                            cx=float(info['mx_depth']), cy=float(info['my_depth']), H=int(info['depthHeight']),
                            W=int(info['depthWidth']))


def create_scannet_dataset(scannet_root: str, scene_id: str, trunc_dist: float = 0.15, frame_downsample: int = 15,
                           n_rays: int = 200, n_surf_samples: int = 8, n_strat_samples: int = 19,
                           voxel_size: float = None, device='cuda:0', padded=False) -> PosedSdfRgbd:
    """Reference :85-113, same defaults.  ``device`` / ``padded`` are additions (the frames live on the device;
    padded batches let the trainer replay one captured step, see PosedSdfRgbd).  ``voxel_size`` (the ScanNet demo maps with
    0.01 and tracks with 0.05) down-samples every batch on the device (ops.voxel_down_sample); it needs a GPU ``device``."""
    scene_name = f"scene{scene_id}"
    scene_file = join(scannet_root, scene_name, f"{scene_name}.txt")
    info = get_scannet_metadata(scene_file)
    return PosedSdfRgbd(dataset_root=join(scannet_root, scene_name), num_input_frames=int(info['numColorFrames']),
                        cam_params=get_scannet_cam_intrinsics(scene_file), frame_downsample=frame_downsample,
                        n_rays=n_rays, min_depth=0.07, max_depth=12.0, n_surf_samples=n_surf_samples,
                        n_strat_samples=n_strat_samples, trunc_dist=trunc_dist, voxel_size=voxel_size, device=device,
                        padded=padded)


def _as_mesh(mesh):
    from miso_amd.grid_opt.utils import utils_sdf
    return utils_sdf.read_ply(mesh) if isinstance(mesh, (str, bytes)) or hasattr(mesh, '__fspath__') else mesh


def _sampled(mesh, count, seed, device, want_normals):
    """``count`` fp32 surface samples of a TriangleMesh on ``device`` and, if asked, the unit normals of the sampled faces"""
    from miso_amd.grid_opt.utils import utils_eval
    verts = torch.from_numpy(np.asarray(mesh.vertices, dtype=np.float64)).to(device)
    tris = torch.from_numpy(np.asarray(mesh.triangles, dtype=np.int64)).to(device)
    if tris.shape[0] == 0:
        raise ValueError("align_mesh_to_ref: a mesh without triangles")
    gen = torch.Generator(device=device).manual_seed(int(seed))
    points, face, _ = utils_eval.sample_surface(verts, tris, int(count), gen)
    normals = None
    if want_normals:
        a, b, c = (verts[tris[face, k]] for k in range(3))
        normals = torch.nn.functional.normalize(torch.cross(b - a, c - a, dim=1), dim=1).to(torch.float32)
    return points.to(torch.float32).contiguous(), normals


def icp_coarse_then_fine(src, tgt, normals, constraint_type, voxel_size, threshold_factor_coarse, threshold_factor_fine, num_iters,
                         index=None):
    """The two passes the reference's align_mesh_to_ref functions share (utils_scannet.py:140-151, utils_ncd.py:72-83): a
    coarse ICP with the L2 loss at ``voxel_size * threshold_factor_coarse`` from the identity, then a fine one with
    TukeyLoss(k=1e-2) at ``voxel_size * threshold_factor_fine`` from the coarse result, on one ops.NearestIndex over
    ``tgt``.  -> the fine RegistrationResult"""
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_registration as reg
    index = ops.NearestIndex(tgt) if index is None else index
    coarse = reg.registration_icp(src, index, tgt, normals, voxel_size * threshold_factor_coarse, np.eye(4),
                                  kind=constraint_type, loss=None, max_iteration=num_iters)
    fine = reg.registration_icp(src, index, tgt, normals, voxel_size * threshold_factor_fine, coarse.transformation,
                                kind=constraint_type, loss=reg.TukeyLoss(k=1e-2), max_iteration=num_iters)
    logger.debug(f"Finetuned ICP result: {fine}\n{fine.transformation}")
    return fine


def align_mesh_to_ref(est_mesh, ref_mesh, constraint_type='point_to_plane', voxel_size=0.02, threshold_factor_coarse=15,
                      threshold_factor_fine=1.5, num_iters=100, num_points=1000000, seed=0, normals='faces'):
    """Reference :115-156, same defaults: ``num_points`` surface samples of each mesh (utils_eval.sample_surface, seeds
    ``seed`` and ``seed + 1``), a coarse ICP with the L2 loss at ``voxel_size * threshold_factor_coarse`` from the identity,
    then a fine one with TukeyLoss(k=1e-2) at ``voxel_size * threshold_factor_fine`` from the coarse result.  One
    ops.NearestIndex over the reference's samples serves both passes.  ``est_mesh`` / ``ref_mesh``: utils_sdf.TriangleMesh
    objects or PLY paths.

    ``normals``, the target normals of 'point_to_plane': 'faces' (the default) takes the FACE NORMALS of the sampled
    triangles, which are exact; 'knn' estimates them from the reference's samples with the 30 nearest neighbours, as the
    reference does (``estimate_normals()``, utils_registration.estimate_normals here).  Other differences from the
    reference, on purpose: the samples are not Open3D's; the input mesh is left alone and no viewer is opened.
    -> (a copy of ``est_mesh`` moved by the fine result, that RegistrationResult; its ``transformation`` is T_ref_est)."""
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_registration as reg
    if constraint_type not in ('point_to_plane', 'point_to_point'):
        raise ValueError(f"Unknown constraint type {constraint_type}")
    if normals not in ('faces', 'knn'):
        raise ValueError(f"Unknown normals {normals}")
    est, ref = _as_mesh(est_mesh), _as_mesh(ref_mesh)
    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    plane = constraint_type == 'point_to_plane'
    src, _ = _sampled(est, num_points, seed, device, False)
    tgt, tgt_normals = _sampled(ref, num_points, seed + 1, device, plane and normals == 'faces')
    index = ops.NearestIndex(tgt)
    if plane and normals == 'knn':
        tgt_normals = reg.estimate_normals(tgt, index=index)
    fine = icp_coarse_then_fine(src, tgt, tgt_normals, constraint_type, voxel_size, threshold_factor_coarse,
                                threshold_factor_fine, num_iters, index)
    return copy.deepcopy(est).apply_transform(fine.transformation), fine
