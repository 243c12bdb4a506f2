"""Pairwise submap alignment by ICP on the near-surface samples (reference: grid_opt/align/icp.py:14-118, an Open3D
pipeline).  Here the clouds stay on the device: Open3D's voxel_down_sample is utils_geometry.voxel_centroid_down_sample,
its estimate_normals is ops.NearestIndex.normals on the down-sampled target (by default a RADIUS search of
NN_NORMAL_SPACINGS point spacings; ``normals_knn=30`` is Open3D's default 30 nearest neighbours, csrc/knn.hip),
registration_icp and get_information_matrix_from_point_clouds are utils_registration's (csrc/icp.hip).

The reference reads the batch keys 'submap_idxs' / 'coords_kf' / 'keyframe_idxs', which none of its current datasets
write; this module reads what they write and what align/miso.py reads: 'sample_frame_ids' and 'coords_frame', the submap
of a row being the owner of its keyframe.

``align_multiple_submaps`` (reference :121-201) is not built: it is Open3D's pose-graph optimiser (PoseGraph,
global_optimization with Levenberg-Marquardt and edge pruning), which has no counterpart here."""
import logging

import numpy as np
import torch

import miso_amd.grid_opt.utils.utils as utils
import miso_amd.grid_opt.utils.utils_geometry as utils_geometry
from miso_amd.grid_opt.models.grid_atlas import GridAtlas

logger = logging.getLogger(__name__)


def get_points_for_submap(grid_atlas: GridAtlas, dataset, submap_id: int, num_batches=1, trunc_dist=1e-3) -> torch.Tensor:
    """Reference :14-48: the samples of ``num_batches`` draws of ``dataset[0]`` that belong to ``submap_id`` and lie within
    ``trunc_dist`` of the surface (|sdf| < trunc_dist), in the submap's frame.  -> (K, 3) fp32 tensor on the device of the
    batch (the reference returns a numpy array for Open3D)."""
    from miso_amd.grid_opt.loss import transform_by_keyframe
    coords_list = []
    with torch.no_grad():
        for batch_id in range(num_batches):
            model_input, gt = dataset[0]
            kf_idxs = model_input['sample_frame_ids'][:, 0]
            owner = grid_atlas.submap_id_for_kf_batch(kf_ids=kf_idxs)
            rows = torch.nonzero(owner == submap_id, as_tuple=False).squeeze(1)
            if rows.numel() == 0:
                logger.warning(f"Submap {submap_id} is not in batch {batch_id}.")
                continue
            coords_submap = transform_by_keyframe(model_input['coords_frame'][rows, :], kf_idxs[rows],
                                                  lambda k: grid_atlas.updated_kf_pose_in_submap(k, submap_id))
            near = torch.abs(gt['sdf'][rows, 0]) < trunc_dist
            coords_list.append(coords_submap[near, :])
    if not coords_list:
        return torch.zeros((0, 3), dtype=torch.float32)
    return torch.cat(coords_list, dim=0).detach().to(torch.float32)


def align_submap_pair(grid_atlas: GridAtlas, dataset, src_id: int, dst_id: int, constraint_type='point_to_plane',
                      voxel_size=0.02, threshold_factor_coarse=15, threshold_factor_fine=1.5, num_iters=30, num_batches=10,
                      update_grid_atlas=True, trunc_dist=1e-3, device=None, normals_knn=None):
    """Reference :51-118, same defaults: coarse then fine ICP (both with the L2 loss, as upstream) of submap ``src_id``'s
    near-surface samples onto ``dst_id``'s, from the atlas' initial relative pose, and the information matrix of the
    result.  ``update_grid_atlas``: ``dst_id``'s pose correction is set so that its updated pose agrees with the result.
    ``trunc_dist`` (get_points_for_submap's) and ``device`` (default: the first GPU) are additions, and so is
    ``normals_knn``: None takes the target normals from the radius search, an int from that many nearest neighbours
    (30 is upstream's ``estimate_normals()``).
    -> (RegistrationResult with T_dst_src, information (6, 6) float64, {'cpu_time_sec', 'gpu_time_sec'})"""
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_registration as reg
    if constraint_type not in ('point_to_plane', 'point_to_point'):
        raise ValueError(f"Unknown constraint type {constraint_type}")
    timer = utils.PerfTimer(activate=True)
    timer.reset()
    device = torch.device("cuda:0") if device is None else torch.device(device)
    clouds = []
    for sid in (src_id, dst_id):
        pts = get_points_for_submap(grid_atlas, dataset, sid, num_batches=num_batches, trunc_dist=trunc_dist).to(device)
        clouds.append(utils_geometry.voxel_centroid_down_sample(pts, voxel_size).to(torch.float32).contiguous())
    src, dst = clouds
    index = ops.NearestIndex(dst)
    normals = index.normals(knn=normals_knn)[0] if constraint_type == 'point_to_plane' else None
    R_world_src, t_world_src = grid_atlas.initial_submap_pose(src_id)
    R_world_dst, t_world_dst = grid_atlas.initial_submap_pose(dst_id)
    T_world_src = utils_geometry.pose_matrix(R_world_src, t_world_src)
    T_world_dst = utils_geometry.pose_matrix(R_world_dst, t_world_dst)
    T_dst_src = torch.linalg.solve(T_world_dst, T_world_src).detach().cpu().numpy().astype(np.float64)
    coarse = reg.registration_icp(src, index, dst, normals, voxel_size * threshold_factor_coarse, T_dst_src,
                                  kind=constraint_type, max_iteration=num_iters)
    fine = reg.registration_icp(src, index, dst, normals, voxel_size * threshold_factor_fine, coarse.transformation,
                                kind=constraint_type, max_iteration=num_iters)
    information = reg.get_information_matrix(src, index, voxel_size * threshold_factor_fine, fine.transformation)
    if update_grid_atlas:
        T_dst_src_opt = torch.from_numpy(fine.transformation.copy()).float().to(T_world_src)
        T_world_dst_opt = T_world_src @ torch.linalg.inv(T_dst_src_opt)
        R_delta, t_delta = utils_geometry.get_pose_correction(R_world_dst, t_world_dst, T_world_dst_opt[:3, :3],
                                                              T_world_dst_opt[:3, [3]])
        grid_atlas.set_submap_pose_correction(dst_id, R_delta, t_delta)
    cpu_time, gpu_time = timer.check()
    logger.info(f"ICP {src_id}-{dst_id} ends. cpu_time={cpu_time:.2f} sec, gpu_time={gpu_time:.2f} sec.")
    return fine, information, {'cpu_time_sec': cpu_time, 'gpu_time_sec': gpu_time}


def align_multiple_submaps(grid_atlas: GridAtlas, dataset, submap_pairs=None, check_intersection=True,
                           constraint_type='point_to_plane', voxel_size=0.02, threshold_factor_coarse=15,
                           threshold_factor_fine=1.5, num_icp_iters=30, num_batches=1, set_odometry_certain=False):
    """Reference :121-201.  Not built: the pairwise edges are align_submap_pair's, but joining them is Open3D's pose-graph
    optimisation (global_optimization: Levenberg-Marquardt over the node poses with line-process edge pruning), which
    this project has no implementation of.  align/miso.py's hierarchical alignment is the multi-submap method here."""
    raise NotImplementedError("align_multiple_submaps needs a pose-graph optimiser (Open3D's global_optimization), which "
                              "is not part of this project; use align_submap_pair per pair, or align/miso.py")
