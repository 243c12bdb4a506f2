"""Newer College mesh grading: ``align_mesh_to_ref`` (reference: grid_opt/utils/utils_ncd.py:46-89, an Open3D registration
pipeline), the ICP of a reconstruction onto a reference that is either a mesh or a POINT CLOUD (the dataset's ground
truth is a laser scan).  It is built from utils_scannet's pieces: the surface samples, one ops.NearestIndex over the
reference's points and the coarse-then-fine passes of utils_registration.registration_icp.

A point cloud has no faces, so the target normals of 'point_to_plane' are estimated from the reference's points with the
30 nearest neighbours (utils_registration.estimate_normals, csrc/knn.hip), which is what the reference's
``estimate_normals()`` does for both formats; 'mesh' does the same here, where utils_scannet.align_mesh_to_ref defaults
to the sampled faces' normals.

Not built: ``create_ncd_dataset`` (PosedSdf3DLidar's file reader is not part of this project) and ``evaluate_mapping``
(it crops with Open3D's minimal oriented bounding box; tools/eval_mesh.py grades with a PCA box)."""
import copy
import logging

import numpy as np
import torch

from miso_amd.grid_opt.utils import utils_geometry
from miso_amd.grid_opt.utils.utils_scannet import _as_mesh, _sampled, icp_coarse_then_fine

logger = logging.getLogger(__name__)

POINTCLOUD_VOXEL = 0.01        # reference :58: a point-cloud reference is down-sampled to 1 cm voxels


def align_mesh_to_ref(est_mesh, ref_mesh, constraint_type='point_to_plane', voxel_size=0.02, threshold_factor_coarse=15,
                      threshold_factor_fine=1.5, num_iters=100, ref_format='mesh', num_points=1000000, seed=0):
    """Reference :46-89, same defaults.  ``est_mesh``: a utils_sdf.TriangleMesh or a PLY path.  ``ref_mesh``: for
    ``ref_format='mesh'`` the same, sampled at ``num_points`` points; for ``'pointcloud'`` an (M, 3) array or tensor, a
    TriangleMesh whose vertices are the cloud, or a PLY path, down-sampled to the centroids of 1 cm voxels.
    ``num_points`` and ``seed`` (of the surface samples) are additions; the input mesh is left alone.
    -> (a copy of ``est_mesh`` moved by the fine result, that RegistrationResult; its ``transformation`` is T_ref_est)."""
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_registration as reg
    if constraint_type not in ('point_to_plane', 'point_to_point'):
        raise ValueError(f"Unknown constraint type {constraint_type}")
    if ref_format not in ('mesh', 'pointcloud'):
        raise ValueError(f"Unknown reference format {ref_format}!")
    est = _as_mesh(est_mesh)
    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    src, _ = _sampled(est, num_points, seed, device, False)
    if ref_format == 'mesh':
        tgt, _ = _sampled(_as_mesh(ref_mesh), num_points, seed + 1, device, False)
    else:
        cloud = ref_mesh if isinstance(ref_mesh, (np.ndarray, torch.Tensor)) else _as_mesh(ref_mesh).vertices
        cloud = torch.as_tensor(np.asarray(cloud) if not isinstance(cloud, torch.Tensor) else cloud).to(device).reshape(-1, 3)
        tgt = utils_geometry.voxel_centroid_down_sample(cloud, POINTCLOUD_VOXEL).to(torch.float32).contiguous()
    index = ops.NearestIndex(tgt)
    normals = reg.estimate_normals(tgt, index=index) if constraint_type == 'point_to_plane' else None
    fine = icp_coarse_then_fine(src, tgt, normals, constraint_type, voxel_size, threshold_factor_coarse,
                                threshold_factor_fine, num_iters, index)
    return copy.deepcopy(est).apply_transform(fine.transformation), fine
