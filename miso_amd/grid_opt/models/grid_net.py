"""One submap: L feature grids + L stability grids + decoder + per-keyframe pose
corrections (reference: grid_opt/models/grid_net.py)."""
import logging
import math
import os

import numpy as np
import torch
import torch.nn as nn

import miso_amd.grid_opt.utils.utils as utils
import miso_amd.grid_opt.utils.utils_geometry as utils_geometry
from miso_amd import ops
from .base_net import BaseNet
from .grid_modules import FeatureGrid, HashFeatureGrid
from .modules import MLPNet

logger = logging.getLogger(__name__)

# A decoder with trainable weights keeps the fused forward and backward: GridNet.forward hands ops.sdf_fused the pack and
# the weight gradients come from the HIP weight-gradient kernel (csrc/decoder_wgrad.hip).  _FUSED_WGRAD = False (tests
# and tools set it, as their reference) restores the op-by-op route for such a decoder: query_feature +
# utils.grid_decode, torch's own autograd.
_FUSED_WGRAD = True


class GridNet(BaseNet):
    def __init__(self, cfg: dict, device='cuda:0', dtype=torch.float32, initial_features=dict()):
        super().__init__(cfg, device, dtype)
        self.initial_features = initial_features
        self.init_grid(cfg)
        self.init_decoder(cfg)
        self.init_poses(cfg)

    def save(self, ckpt_dir, ckpt_prefix):
        self.decoder.save(os.path.join(ckpt_dir, f"{ckpt_prefix}_decoder.pt"))

    # ---- construction ----------------------------------------------------------------
    def init_grid(self, cfg):
        g = cfg['grid']
        self.num_levels = g['n_levels']
        self.second_order_grid_sample = bool(g.get('second_order_grid_sample', False))
        self.fdim = g['feature_dim']
        self.grid_type = g['type']
        if self.grid_type not in ('regular', 'hash'):
            raise ValueError(f"grid type {self.grid_type!r} is outside the MI355X hot path ('regular' or 'hash')")
        # 'hash': every level is looked up through a table of at most 2^log2_hashmap_size rows (HashFeatureGrid); the
        # queries go through ops.hash_encode and every fused route declines (_fused_decoder).  grid.hash_fused (default
        # False; no meaning for 'regular'): forward() and sdf_and_gradient() of a hash net with a frozen decoder run the
        # table gather and the decoder as one launch instead (_fused_hash_decoder, ops.hash_sdf_fused), and sphere_trace()
        # the whole ray loop (ops.hash_sphere_trace)
        self.hash_fused = bool(g.get('hash_fused', False))
        level_cls, extra = FeatureGrid, {}
        if self.grid_type == 'hash':
            level_cls, extra = HashFeatureGrid, dict(log2_hashmap_size=int(g.get('log2_hashmap_size', 19)))
        self.features = nn.ModuleList()
        self.feature_stability = nn.ModuleList()
        self.bases = nn.ModuleList()
        self.cell_sizes = []
        for level in range(self.num_levels):
            cell = g['base_cell_size'] / (g['per_level_scale'] ** level)
            self.cell_sizes.append(cell)
            common = dict(d=self.d, bound=self.bound, cell_size=cell, dtype=self.dtype,
                          second_order_grid_sample=self.second_order_grid_sample, **extra)
            self.features.append(level_cls(fdim=self.fdim, name=f"feat-{level}",
                                           initial_feature=self.initial_features.get(level),
                                           init_stddev=g['init_stddev'], **common))
            self.feature_stability.append(level_cls(fdim=1, name=f"stab-{level}", initial_feature=None,
                                                    init_stddev=0.0, **common))
            self.bases.append(None)
        self.ignore_level_ = np.zeros(self.num_levels).astype(bool)

    def init_decoder(self, cfg):
        d = cfg['decoder']
        self.decoder_hidden_dim = d['hidden_dim']
        self.decoder_hidden_layers = d['hidden_layers']
        self.decoder_out_dim = d['out_dim']
        self.pos_invariant = d['pos_invariant']
        self.decoder_fixed = d['fix']
        self.decoder_type = d['type']
        in_dim = self.num_levels * self.fdim + (0 if self.pos_invariant else self.d)
        if self.decoder_type == 'mlp':
            self.decoder = MLPNet(input_dim=in_dim, output_dim=self.decoder_out_dim,
                                  hidden_dim=self.decoder_hidden_dim, hidden_layers=self.decoder_hidden_layers,
                                  bias=True, pretrained_path=d.get('pretrained_model'),
                                  no_optimize=self.decoder_fixed)
        elif self.decoder_type == 'none':
            self.decoder = None
        else:
            raise ValueError(f"Unknown decoder type: {self.decoder_type}")

    def init_poses(self, cfg):
        self.num_poses = cfg['pose']['num_poses']
        self.optimize_pose = cfg['pose']['optimize']
        self.rotation_corrections = nn.Parameter(torch.zeros(self.num_poses, 3, device=self.device),
                                                 requires_grad=self.optimize_pose)
        self.translation_corrections = nn.Parameter(torch.zeros(self.num_poses, 3, 1, device=self.device),
                                                    requires_grad=self.optimize_pose)
        self.pose_estimates_known = [False] * self.num_poses
        self.register_buffer('Rwk', utils_geometry.identity_rotations(self.num_poses).to(self.device))
        self.register_buffer('twk', torch.zeros(self.num_poses, 3, 1, device=self.device))
        self.locked_pose_indices = set()
        self._pose_key_to_id = dict()

    # ---- level / lock management -------------------------------------------------------
    def ignore_level(self, l):
        self.ignore_level_[l] = True

    def include_level(self, l):
        self.ignore_level_[l] = False

    def lock_level(self, l):
        self.features[l].lock()
        self.feature_stability[l].lock()

    def unlock_level(self, l):
        self.features[l].unlock()
        self.feature_stability[l].unlock()

    def lock_feature(self):
        for l in range(self.num_levels):
            self.lock_level(l)

    def unlock_feature(self):
        for l in range(self.num_levels):
            self.unlock_level(l)

    def lock_pose(self):
        self.rotation_corrections.requires_grad_(False)
        self.translation_corrections.requires_grad_(False)
        self.lock_all_pose_indices()

    def unlock_pose(self):
        self.rotation_corrections.requires_grad_(True)
        self.translation_corrections.requires_grad_(True)
        self.unlock_all_pose_indices()

    def lock_pose_index(self, pose_index: int):
        self.locked_pose_indices.add(pose_index)

    def lock_all_pose_indices(self):
        self.locked_pose_indices = set(range(self.num_poses))

    def unlock_pose_index(self, pose_index: int):
        self.locked_pose_indices.remove(pose_index)

    def unlock_all_pose_indices(self):
        self.locked_pose_indices.clear()

    # ---- keyframe poses ------------------------------------------------------------------
    def pose_correction(self, kf_id: int):
        r = self.rotation_corrections[[kf_id], :]        # (1,3)
        t = self.translation_corrections[kf_id, :, :]    # (3,1)
        if kf_id in self.locked_pose_indices:
            r, t = r.clone().detach(), t.clone().detach()
        return r, t

    def set_initial_kf_pose(self, kf_id: int, Rwk: torch.Tensor, twk: torch.Tensor, kf_key=None):
        assert Rwk.shape == (3, 3) and twk.shape == (3, 1)
        assert kf_id < self.num_poses, f"KF ID {kf_id} exceeds the number of poses {self.num_poses}!"
        self.pose_estimates_known[kf_id] = True
        self.Rwk[kf_id] = Rwk.to(self.Rwk)
        self.twk[kf_id] = twk.to(self.twk)
        with torch.no_grad():
            self.rotation_corrections[kf_id].zero_()
            self.translation_corrections[kf_id].zero_()
        if kf_key is not None:
            self._pose_key_to_id[kf_key] = kf_id
            self.__dict__['_pose_keys_version'] = self.__dict__.get('_pose_keys_version', 0) + 1

    def pose_key_to_id(self, kf_key):
        assert kf_key in self._pose_key_to_id, f"Key {kf_key} not found in pose key to ID mapping!"
        return self._pose_key_to_id[kf_key]

    def initial_kf_pose(self, kf_id: int):
        assert self.pose_estimates_known[kf_id], f"Initial pose estimate for KF {kf_id} is not available!"
        return self.Rwk[kf_id], self.twk[kf_id]

    def initial_kf_pose_in_world(self, kf_id: int):
        return self.initial_kf_pose(kf_id)

    def initial_kf_pose_from_key(self, kf_key):
        return self.initial_kf_pose(self.pose_key_to_id(kf_key))

    def updated_kf_pose(self, kf_id: int):
        R, t = self.initial_kf_pose_in_world(kf_id)
        dr, dt = self.pose_correction(kf_id)
        return utils_geometry.apply_pose_correction(R, t, dr, dt)

    def updated_kf_pose_in_world(self, kf_id: int):
        return self.updated_kf_pose(kf_id)

    def updated_kf_poses_all(self):
        """All keyframe poses at once, (P,3,3) and (P,3,1): updated_kf_pose for every index with ONE
        batched exponential map; locked indices are detached exactly as pose_correction does."""
        from miso_amd.so3 import so3_exp_map
        dr, dt = self.rotation_corrections, self.translation_corrections
        # without a graph to build (no_grad, or every index locked) the result only changes when a pose
        # tensor is written: keep it (the exponential map is ~20 tiny launches per call)
        static = (not torch.is_grad_enabled() or len(self.locked_pose_indices) >= self.num_poses
                  or not (dr.requires_grad or dt.requires_grad))
        if static:
            key = (dr._version, dt._version, self.Rwk._version, self.twk._version, dr.data_ptr(), self.Rwk.data_ptr())
            hit = self.__dict__.get('_kf_pose_cache')
            if hit is not None and hit[0] == key:
                return hit[1], hit[2]
            with torch.no_grad():
                R, t = self.Rwk @ so3_exp_map(dr.detach()), self.twk + dt.detach()
            self.__dict__['_kf_pose_cache'] = (key, R, t)
            return R, t
        if self.locked_pose_indices:
            if len(self.locked_pose_indices) >= self.num_poses:
                dr, dt = dr.detach(), dt.detach()
            else:
                locked = torch.zeros(self.num_poses, dtype=torch.bool, device=dr.device)
                locked[list(self.locked_pose_indices)] = True
                dr = torch.where(locked[:, None], dr.detach(), dr)
                dt = torch.where(locked[:, None, None], dt.detach(), dt)
        return self.Rwk @ so3_exp_map(dr), self.twk + dt

    def kf_key_index_table(self, prefix='KF'):
        """LongTensor t with t[k] = pose index of key f'{prefix}{k}' (-1: unknown), on the model's
        device, rebuilt when the key set changes: maps a batch's frame ids to poses without a
        host round trip."""
        # (the key set only changes through set_initial_kf_pose: its counter + the dict's length stand for the contents
        # between changes -- building the signature below walks every key, 50 us per call at 100 keyframes)
        quick = (prefix, self.__dict__.get('_pose_keys_version', 0), len(self._pose_key_to_id), self.Rwk.device)
        hit = self.__dict__.get('_kf_table')
        if hit is not None and len(hit) > 2 and hit[2] == quick:
            return hit[1]
        items = [(int(k[len(prefix):]), v) for k, v in self._pose_key_to_id.items()
                 if isinstance(k, str) and k.startswith(prefix) and k[len(prefix):].isdigit()]
        sig = (prefix, tuple(sorted(items)), str(self.Rwk.device))
        hit = self.__dict__.get('_kf_table')
        if hit is None or hit[0] != sig:
            t = torch.full((max([k for k, _ in items], default=-1) + 2,), -1, dtype=torch.long)
            for k, v in items:
                t[k] = v
            hit = (sig, t.to(self.Rwk.device))
        hit = (hit[0], hit[1], quick)
        self.__dict__['_kf_table'] = hit
        return hit[1]

    def updated_kf_pose_from_key(self, kf_key):
        return self.updated_kf_pose(self.pose_key_to_id(kf_key))

    def print_kf_pose_info(self):
        rot = torch.linalg.norm(self.rotation_corrections, dim=1).max()
        tran = torch.linalg.norm(self.translation_corrections.squeeze(2), dim=1).max()
        logger.info(f"GridNet KF pose corrections: max_rot={math.degrees(rot):.3f}deg, max_tran={tran:.3f}m.")

    def print_feature_info(self):
        for l in range(self.num_levels):
            logger.info(f"Level {l} norm: {self.features[l].norm():.2f}")

    def zero_features(self):
        for grid in self.features:
            grid.zero_features()

    def randn_features(self, std):
        for grid in self.features:
            grid.randn_features(std)

    # ---- queries (the hot path) ----------------------------------------------------------
    def _check_coords(self, x):
        assert x.ndim == 2, f"Invalid input coords shape {x.shape}!"
        assert x.shape[-1] == self.d

    def query_feature(self, x: torch.Tensor):
        self._check_coords(x)
        return utils.grid_interp_regular(self.features, x, self.ignore_level_)

    def query_stability(self, x: torch.Tensor):
        self._check_coords(x)
        return utils.grid_interp_regular(self.feature_stability, x, None)

    def _fused_decoder(self, trainable=False):
        """DecoderPack if encode+decode can run as one kernel for this model, else None.  trainable=True (forward() only):
        a decoder with trainable weights qualifies too -- ops.sdf_fused then forms their gradients in HIP."""
        if self.decoder is None or not self.pos_invariant or not isinstance(self.decoder, MLPNet):
            return None
        if self.grid_type != 'regular':      # the fused kernels address dense levels: forward is encode + MLPNet
            return None
        pack = self.decoder.decoder_pack(trainable=trainable)
        if pack is None:
            return None
        feats = [g.feature for g in self.features]
        meta = self.features[0].grid_meta(self.ignore_level_)
        return pack if ops.sdf_fused_supported(feats, meta, pack) else None

    def _hash_args(self, detach=False):
        """(tables, meta, dims, log2) of a hash net as the ops.hash_* calls take them"""
        grids = list(self.features)
        return ([g.feature.detach() if detach else g.feature for g in grids], grids[0].grid_meta(self.ignore_level_),
                [g.dims for g in grids], grids[0].log2_hashmap_size)

    def _fused_hash_decoder(self):
        """DecoderPack if grid.hash_fused is on and table gather + decoder can run as one kernel for this model
        (ops.hash_sdf_fused: a hash grid, a position-invariant MLPNet with a frozen pack, tensors on the device, a shape
        the kernels cover), else None.  _fused_decoder() stays None for a hash grid: the routes that ask it address
        dense levels."""
        if not getattr(self, 'hash_fused', False) or self.grid_type != 'hash':
            return None
        if self.decoder is None or not self.pos_invariant or not isinstance(self.decoder, MLPNet):
            return None
        pack = self.decoder.decoder_pack()
        if pack is None:
            return None
        return pack if ops.hash_sdf_supported(*self._hash_args(), pack) else None

    def forward(self, x: torch.Tensor, noise_std=0):
        self._check_coords(x)
        pack = self._fused_decoder(trainable=_FUSED_WGRAD) if x.is_cuda else None
        hpack = self._fused_hash_decoder() if pack is None and x.is_cuda else None
        if pack is not None:
            meta = self.features[0].grid_meta(self.ignore_level_)
            pred = ops.sdf_fused(x, [g.feature for g in self.features], meta, pack)
        elif hpack is not None:
            pred = ops.hash_sdf_fused(x, *self._hash_args(), hpack)
        else:
            feats = self.query_feature(x)
            pred = utils.grid_decode(feats, x, self.decoder, self.pos_invariant)
        if noise_std > 0:
            pred = pred + torch.randn(pred.shape, device=x.device) * noise_std
        return pred

    def sphere_trace(self, origins: torch.Tensor, directions: torch.Tensor, min_dist=1e-3, max_dist=5e1, max_iters=100,
                     epsilon=1e-5, **extras):
        """utils_sdf.sphere_tracing(self, ...) in ONE launch: this grid as a one-submap atlas with an identity pose row
        and no bound test, which is forward() bit for bit (ops.AtlasQuery.trace; extras: want_sdf, want_steps,
        grad_step).  A hash net with grid.hash_fused on: ops.hash_sphere_trace over its tables, the same loop around
        the field of its fused forward().  -> (points (N,3), mask (N,1) bool, extras dict); None when autograd is on, the
        tensors are on the host or neither fused decoder covers this model: utils_sdf.sphere_tracing then runs its loop."""
        if torch.is_grad_enabled() or not (origins.is_cuda and directions.is_cuda):
            return None
        pack = self._fused_decoder()
        if pack is None:
            hpack = self._fused_hash_decoder()
            if hpack is None or not ops.hash_trace_supported(*self._hash_args(), hpack):
                return None
            return ops.hash_sphere_trace(*self._hash_args(detach=True), hpack, origins, utils.normalize_last_dim(directions),
                                         min_dist=min_dist, max_dist=max_dist, max_iters=max_iters, epsilon=epsilon, **extras)
        q = self.__dict__.setdefault('_trace_query', ops.AtlasQuery())
        ident = self.__dict__.get('_trace_ident')
        if ident is None or ident.device != origins.device:
            ident = torch.tensor([[1., 0., 0., 0., 1., 0., 0., 0., 1., 0., 0., 0.]], device=origins.device)
            self.__dict__['_trace_ident'] = ident
        feats = [g.feature.detach() for g in self.features]
        meta = self.features[0].grid_meta(self.ignore_level_)
        return q.trace([feats], [meta], ident, pack, origins, utils.normalize_last_dim(directions), min_dist=min_dist,
                       max_dist=max_dist, max_iters=max_iters, epsilon=epsilon, no_bound=True, **extras)

    def sdf_and_gradient(self, x: torch.Tensor):
        """(sdf (N,1), d sdf / d x (N,3)), both detached: what the tracker's Gauss-Newton step needs
        (reference tracker.py:176-181 runs a forward and an autograd backward for it).  With the fused
        decoder this is two launches and no autograd graph -- in particular no gradient is formed
        for the feature grids, which autograd would produce whenever they are unlocked."""
        self._check_coords(x)
        pack = self._fused_decoder() if x.is_cuda else None
        if pack is not None:
            feats = [g.feature.detach() for g in self.features]
            meta = self.features[0].grid_meta(self.ignore_level_)
            xd = x.detach().contiguous()
            sdf, mask = ops.sdf_fwd_raw(xd, feats, meta, pack, True)
            gx, _ = ops.sdf_bwd_raw(xd, feats, meta, pack, torch.ones_like(sdf), mask, True, [False] * len(feats))
            return sdf, gx
        hpack = self._fused_hash_decoder() if x.is_cuda else None
        if hpack is not None:      # the same two calls over the tables: no autograd graph, no table gradient
            args = self._hash_args(detach=True)
            xd = x.detach().contiguous()
            sdf, mask = ops.hash_sdf_fwd_raw(xd, *args, hpack, True)
            gx, _, _ = ops.hash_sdf_bwd_raw(xd, *args, hpack, torch.ones_like(sdf), mask, True, [False] * len(args[0]))
            return sdf, gx
        xr = x.detach().clone().requires_grad_(True)
        if self.grid_type == 'hash' and x.is_cuda:
            # forward() with the tables detached: autograd.grad below asks for x alone, but the encode's backward cannot see
            # that and would zero-fill and scatter a gradient for every unlocked table, to have it dropped
            grids = list(self.features)
            feats = ops.hash_encode(xr, [g.feature.detach() for g in grids], grids[0].grid_meta(self.ignore_level_),
                                    [g.dims for g in grids], grids[0].log2_hashmap_size)
            sdf = utils.grid_decode(feats, xr, self.decoder, self.pos_invariant)
        else:
            sdf = self(xr)
        (gx,) = torch.autograd.grad(sdf, xr, torch.ones_like(sdf))
        return sdf.detach(), gx.detach()

    # ---- parameter groups ------------------------------------------------------------------
    def params_for_poses(self):
        return [self.rotation_corrections, self.translation_corrections]

    def params_for_features(self, stop_level=None):
        stop_level = self.num_levels if stop_level is None else stop_level
        assert stop_level <= self.num_levels
        params = []
        for l in range(stop_level):
            params += list(self.features[l].parameters())
        return params

    def params_at_level(self, level):
        params = []
        levels = [level] if level < self.num_levels else range(self.num_levels)
        for l in levels:
            params += list(self.features[l].parameters())
            params += list(self.feature_stability[l].parameters())
        if not self.decoder_fixed:
            params += list(self.decoder.parameters())
        if self.optimize_pose:
            params += self.params_for_poses()
        return params
