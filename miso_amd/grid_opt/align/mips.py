"""MIPS-Fusion's projected-match residual as an alignment baseline (reference: grid_opt/align/mips.py, eq. (19)-(22) of
MIPS-Fusion): a surface sample p of the source submap is mapped into the destination, q, projected onto the
destination's surface along its SDF gradient, match_dst = q - s(q) grad s(q), mapped back to the source frame and held
against p -- along the source normal ('point_to_plane') or in all three components ('point_to_point').  Both gradients
are constants of the loss here: the poses are reached through q in s(q) and through the two rigid maps.  That is what
the reference's ``with torch.no_grad():`` around its two ``autograd.grad`` calls says; as written, though, those calls
pass ``create_graph=True``, which records a graph whatever the surrounding grad mode, so the reference's own backward also
runs through grad s_dst (a second-order term of the sampler, CUDA only).  This module leaves that term out, on every
route.

Like align/vfpp.py this module reads what this project's datasets write ('sample_frame_ids', 'coords_frame', the submap
of a row being the owner of its keyframe), not the batch keys of the reference's two forms, and both ``dataset_name``
values select the one loss below: the ScanNet form's formula (surface mask, in-bound mask, mean over the rows kept).

With ``use_bound=True``, the atlas on the GPU and a decoder in the fused kernels' table ``align_multiple_submaps_mips``
runs the whole loop on the device (ops.AlignPlan(residual="mips"), csrc/pair_sdf.hip) on ONE batch drawn at the start,
where the reference draws a fresh one per pair and iteration.  On the device p - match_src is evaluated as
s M^T g with M = R_d^T R_s, which is what the reference's expression equals: DESIGN.md 4.6b."""
import logging

import torch

import miso_amd.grid_opt.utils.utils as utils
import miso_amd.grid_opt.utils.utils_geometry as utils_geometry
from miso_amd.grid_opt.align.base import *   # noqa: F401,F403
from miso_amd.grid_opt.align.base import generic_align_multiple_submaps, generic_align_submap_pair
from miso_amd.grid_opt.models.grid_atlas import GridAtlas

logger = logging.getLogger(__name__)

_DATASET_NAMES = ('ScanNet', 'SubmapSdf3D')
_CONSTRAINTS = ('point_to_plane', 'point_to_point')


def pairwise_loss_mips(grid_atlas: GridAtlas, data_loader, src_id: int, dst_id: int, residual_weight=3000,
                       use_bound=True, constraint_type='point_to_plane', device="cuda:0", surf_thresh=1e-3):
    """{'mips_{src}_{dst}': residual_weight * mean(cons^2)} over the rows of ``src_id`` with |gt sdf| < surf_thresh [and
    in dst's bound]; cons = (p - match_src) . grad s_src(p) ('point_to_plane') or p - match_src ('point_to_point', the
    mean then runs over its three components); {} with a warning when the batch holds no row of ``src_id``.
    ``surf_thresh`` is an addition: the reference hard-codes 1e-3 (its ScanNet form) and 1e-5."""
    from miso_amd.grid_opt.loss import transform_by_keyframe
    assert src_id < grid_atlas.num_submaps and dst_id < grid_atlas.num_submaps
    if constraint_type not in _CONSTRAINTS:
        raise ValueError(f"Invalid constraint type: {constraint_type}!")
    grid_src, grid_dst = grid_atlas.get_submap(src_id), grid_atlas.get_submap(dst_id)
    model_input, gt = utils.get_batch(data_loader, device)
    kf_all = model_input['sample_frame_ids'][0, :, 0]
    rows = torch.nonzero(grid_atlas.submap_id_for_kf_batch(kf_ids=kf_all) == src_id, as_tuple=False).squeeze(1)
    if rows.numel() == 0:
        logger.warning(f"No samples found for submap {src_id}!")
        return {}
    R_src, t_src = grid_atlas.updated_submap_pose(src_id, device)
    R_dst, t_dst = grid_atlas.updated_submap_pose(dst_id, device)
    with torch.no_grad():
        coords_src = transform_by_keyframe(model_input['coords_frame'][0, rows, :], kf_all[rows],
                                           lambda k: grid_atlas.updated_kf_pose_in_submap(k, src_id))
        coords_dst = utils_geometry.transfrom_points_from(utils_geometry.transform_points_to(coords_src, R_src, t_src),
                                                          R_dst, t_dst)
        mask = torch.abs(gt['sdf'][0][rows, :]) < surf_thresh
        if use_bound:
            mask = mask & utils_geometry.coords_in_bound(coords_dst, grid_dst.bound)
        keep = torch.nonzero(mask, as_tuple=False)[:, 0]
    points_src = coords_src[keep, :].detach().requires_grad_(True)
    sdfs_src = grid_src(points_src)
    (grad_src,) = torch.autograd.grad(sdfs_src, points_src, grad_outputs=torch.ones_like(sdfs_src))
    points_dst = utils_geometry.transfrom_points_from(utils_geometry.transform_points_to(points_src, R_src, t_src),
                                                      R_dst, t_dst)
    sdfs_dst = grid_dst(points_dst)
    (grad_dst,) = torch.autograd.grad(sdfs_dst, points_dst, grad_outputs=torch.ones_like(sdfs_dst), retain_graph=True)
    match_dst = points_dst - sdfs_dst * grad_dst.detach()                                    # eq. (19)
    match_src = utils_geometry.transfrom_points_from(utils_geometry.transform_points_to(match_dst, R_dst, t_dst),
                                                     R_src, t_src)
    if constraint_type == 'point_to_plane':
        cons = torch.sum((points_src - match_src) * grad_src.detach(), dim=1)                # eq. (20)
    else:
        cons = points_src - match_src
    return {f'mips_{src_id}_{dst_id}': torch.mean(cons ** 2) * residual_weight}


pairwise_loss_mips_scannet = pairwise_loss_mips


def _loss_func(dataset_name, **opts):
    if dataset_name not in _DATASET_NAMES:
        raise ValueError(f"Invalid dataset name: {dataset_name}!")

    def mips(atlas, loader, a, b):
        return pairwise_loss_mips(atlas, loader, a, b, **opts)
    return mips


def align_submap_pair_mips(grid_atlas: GridAtlas, dataset, src_id: int, dst_id: int, dataset_name='SubmapSdf3D',
                           num_iters=100, lr=1e-2, residual_weight=3000, use_bound=True,
                           constraint_type='point_to_plane', device='cuda:0', verbose=True, surf_thresh=1e-3):
    """Align ``dst_id`` to ``src_id`` by optimising dst's pose alone on the loss above (generic_align_submap_pair)."""
    loss = _loss_func(dataset_name, residual_weight=residual_weight, use_bound=use_bound,
                      constraint_type=constraint_type, device=device, surf_thresh=surf_thresh)
    return generic_align_submap_pair(grid_atlas, dataset, src_id, dst_id, ('mips', loss), num_iters=num_iters, lr=lr,
                                     verbose=verbose)


def align_multiple_submaps_mips(grid_atlas: GridAtlas, dataset, dataset_name="SubmapSdf3D", num_iters=100, lr=1e-2,
                                residual_weight=3000, use_bound=True, constraint_type="point_to_plane",
                                pose_reg_weight=0, pose_thresh_m=1.0, pose_thresh_rad=1.0, device="cuda:0", verbose=True,
                                surf_thresh=1e-3, save_iterations=False, submap_pairs=None):
    """Adam over the poses of submaps 1..S-1 on the summed pair losses (generic_align_multiple_submaps).  With the bound
    mask on, the atlas on the GPU and a decoder in the fused kernels' table the loop runs on the device on one batch
    drawn here; otherwise, and when the plan refuses the shape, op by op with a log line.  ``surf_thresh``,
    ``save_iterations`` and ``submap_pairs`` are additions."""
    from miso_amd._lib import NotCovered
    from miso_amd.grid_opt.align import miso as _miso
    if constraint_type not in _CONSTRAINTS:
        raise ValueError(f"Invalid constraint type: {constraint_type}!")
    loss = _loss_func(dataset_name, residual_weight=residual_weight, use_bound=use_bound,
                      constraint_type=constraint_type, device=device, surf_thresh=surf_thresh)
    common = dict(num_iters=num_iters, lr=lr, verbose=verbose, pose_reg_weight=pose_reg_weight,
                  pose_thresh_m=pose_thresh_m, pose_thresh_rad=pose_thresh_rad, save_iterations=save_iterations,
                  submap_pairs=submap_pairs)
    why = _miso.fused_sdf_refusal(grid_atlas, device, use_bound=use_bound)
    if why is None:
        batches = _miso.draw_batches(dataset, 1, device)

        def fused_loss(atlas, loader, a, b):
            return loss(atlas, loader, a, b)
        fused_loss.fused = dict(align_loss='L2', align_weight=residual_weight, residual="mips",
                                constraint=constraint_type, decoder=grid_atlas.get_submap(0)._fused_decoder(),
                                inputs=lambda atlas, pairs, chk: _miso.sdf_pair_inputs(
                                    atlas, batches, pairs, check_intersection=chk, surf_thresh=surf_thresh))
        try:
            return generic_align_multiple_submaps(grid_atlas, dataset, ('mips', fused_loss), **common)
        except NotCovered as exc:      # refused at plan build: nothing has run yet
            why = str(exc)
    logger.info(f"AlignMulti_mips runs op by op ({why}).")
    return generic_align_multiple_submaps(grid_atlas, dataset, ('mips', loss), **common)
