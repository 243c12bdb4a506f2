"""Fuser: the two global stages that follow submap construction (reference: grid_opt/slam/fuser.py).

``align`` registers the submaps of an atlas against each other in latent space (reference :29-54).

``fuse`` is the joint refinement after alignment (reference :57-120): every submap's features, the submap pose
corrections and the keyframe pose corrections optimised together against the SDF samples of the dataset, MisoLossFusion
through a Trainer with an external Adam of up to three parameter groups.  Upstream hands MisoLossFusion a keyword its base
class does not take (``gm_scale_sdf``, reference :102) and so never gets as far as the first step; here the loss is built
without it and the method runs.  For its duration the atlas differentiates through the one-launch backward
(GridAtlas.fused_backward -> ops.AtlasQuery.differentiable) unless the eikonal term is on with an autograd gradient,
which needs a second backward through the atlas and stays on the per-submap loop."""
import logging
import math
from copy import deepcopy

import torch
from torch.utils.data import DataLoader
from miso_amd.grid_opt.utils.utils import collate_batch_of_one

from miso_amd.grid_opt.align.miso import align_multiple_submaps_hierarchical
from miso_amd.grid_opt.loss import MisoLossFusion
from miso_amd.grid_opt.models.grid_atlas import GridAtlas
from miso_amd.grid_opt.trainer import Trainer

logger = logging.getLogger(__name__)


class Fuser:
    def __init__(self, model: GridAtlas, dataset, cfg: dict):
        assert isinstance(model, GridAtlas), "Model must be an instance of GridAtlas."
        self.model = model
        self.dataset = dataset
        self.train_loader = DataLoader(dataset, shuffle=True, batch_size=1, num_workers=0, collate_fn=collate_batch_of_one)
        self.cfg = cfg

    def align(self):
        a = self.cfg['align']
        info = align_multiple_submaps_hierarchical(
            grid_atlas=self.model, dataset=self.dataset, level_iters=a['level_iters'],
            finetune_iters=a['finetune_iters'], level_thresh=0, lr=a['learning_rate'],
            align_loss=a['loss_type'], stability_thresh=a['stability_thresh'],
            subsample_points=a['subsample_points'], latent_levels=a['latent_levels'],
            skip_finetune=a['skip_finetune'], pose_reg_weight=a['pose_reg_weight'],
            pose_thresh_m=a.get('pose_thresh_m', 10.0),
            pose_thresh_rad=math.radians(a.get('pose_thresh_deg', 45.0)),
            verbose=a.get('verbose', False), save_iterations=a.get('save_iterations', False),
            device=self.cfg.get('device', 'cuda:0'),
            finetune_fused=a.get('finetune_fused', False))      # the SDF fine-tune on the device: off unless asked for
        self.model.print_submap_pose_info()
        return info

    def fuse(self, feat_lr=1e-3, submap_pose_lr=1e-4, kf_pose_lr=1e-4, iterations=10):
        """Joint Adam refinement of all features, submap poses and keyframe poses for ``iterations`` epochs of the
        dataset (reference :57-120).  A learning rate <= 0 freezes that group."""
        model = self.model
        self.dataset.unselect_keyframes()
        for submap_id in range(model.num_submaps):
            model.unlock_submap(submap_id)
        model.unlock_submap_pose()
        param_groups = []
        for lr, params in ((feat_lr, model.params_for_all_features()),
                           (submap_pose_lr, model.params_for_all_submap_poses()),
                           (kf_pose_lr, model.params_for_all_kf_poses())):
            if lr > 0:
                param_groups.append({'params': params, 'lr': lr})
            else:
                for p in params:
                    p.requires_grad_(False)
        if len(param_groups) == 0:
            logger.warning("No parameters to optimize. Please check the learning rates.")
            return
        cfg_copy = deepcopy(self.cfg)
        cfg_map = cfg_copy['mapping']
        cfg_train = cfg_copy['train']
        cfg_train['epochs'] = iterations
        cfg_train['verbose'] = True
        loss_func = MisoLossFusion(
            weight_sdf=cfg_map['weight_sdf'], weight_eik=cfg_map['weight_eik'], weight_fs=cfg_map['weight_fs'],
            loss_type=cfg_map['loss_type'], trunc_dist=cfg_map['trunc_dist'], finite_diff_eps=cfg_map['finite_diff_eps'],
            grad_method=cfg_map['grad_method'], eik_trunc_dist=cfg_map['eik_trunc_dist'], use_stability=False)
        trainer = Trainer(cfg_train, model, loss_func, self.train_loader, None, self.cfg['device'], torch.float32)
        model.print_trainable_params()
        trainer.set_external_optimizer(torch.optim.Adam(param_groups, lr=1e-3))
        # an eikonal term differentiates d sdf / d x again: with grad_method 'autograd' that is a double backward
        double_backward = loss_func.weight_eik > 0 and loss_func.grad_method != 'finitediff'
        before = model.fused_backward
        model.fused_backward = not double_backward
        try:
            trainer.train()
        finally:
            model.fused_backward = before
        model.print_keyframe_pose_info()
        model.print_submap_pose_info()
