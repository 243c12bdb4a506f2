"""Pure-PyTorch CPU restatement of MISO's encode/decode hot path.

TEST INFRASTRUCTURE ONLY -- see ``oracle/__init__.py``.  The product package
``miso_amd`` never imports this module; ``tests/``, ``__graft_entry__.smoke()``
and ``bench.py``'s ``cpu_baseline`` leg use it as the checker.

Parity status
-------------
* ``encode_stock`` / ``sdf_stock`` are the reference's own op sequence
  (``normalize_coordinates`` -> per-level ``F.grid_sample`` -> ``cat`` ->
  ``nn.Sequential``) restated with stock torch ops; they are pinned against the
  imported reference through the golden vectors in ``tests/golden`` (generated
  by ``tools/make_goldens.py`` in the build container).
* ``trilinear_gather`` is an explicit 8-corner restatement that is differentiable
  to any order (ATen has no double backward for ``grid_sampler_3d``); it is
  pinned against ``F.grid_sample`` (value + first derivatives), against
  ``torch.autograd.gradgradcheck`` in fp64, and against the known-answer inputs
  of the reference's ``third_party/cuda_gridsample_grad2/test3d.py:17-35``.  With ``border`` padding it follows
  ATen's set-grad convention: no coordinate gradient at or beyond either clip limit.
* ``grid_sample_bwd2_aten`` is the second backward of the sampler from ATen calls alone (exact first backward plus
  differences within a cell); ``trilinear_bwd2`` is the same by autograd through ``trilinear_gather``.  The two agree
  to 1e-9 where the first applies, and the restatement is pinned to the reference's ``naive_gridsample.py`` off the
  faces (``tests/golden/grad2_naive.npz``).
* ``so3_exp_map`` / ``hat`` restate pytorch3d (un-vendored, unpinned
  ``git+https://github.com/facebookresearch/pytorch3d.git`` in the reference's
  ``environment.yaml:114``).  pytorch3d is absent from the image, so that
  boundary is **parity unpinned**: it is pinned only by our own goldens.

Every function cites the reference file:line (relative to the MISO repo) it
follows.  All functions are dtype-generic (fp32 for parity, fp64 for
gradcheck / error measurement).
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F


# --------------------------------------------------------------------------- #
# Coordinates
# --------------------------------------------------------------------------- #
def normalize_coordinates(x: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """grid_opt/utils/utils.py:22-51 -- map metres to [-1, 1] per axis."""
    bmin = bound[:, 0].view(1, -1)
    bmax = bound[:, 1].view(1, -1)
    return 2 * (x - bmin) / (bmax - bmin) - 1


def denormalize_coordinates(xn: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """grid_opt/utils/utils.py:53-82."""
    bmin = bound[:, 0].view(1, -1)
    bmax = bound[:, 1].view(1, -1)
    return (xn + 1) / 2 * (bmax - bmin) + bmin


def _unnormalize(c: torch.Tensor, size: int, align_corners: bool) -> torch.Tensor:
    """ATen ``grid_sampler_unnormalize`` (the op behind grid_modules.py:86-94)."""
    if align_corners:
        return ((c + 1) / 2) * (size - 1)
    return ((c + 1) * size - 1) / 2


# --------------------------------------------------------------------------- #
# Trilinear sampling
# --------------------------------------------------------------------------- #
def grid_sample_stock(feature: torch.Tensor, xn: torch.Tensor,
                      align_corners: bool = False,
                      padding_mode: str = "zeros") -> torch.Tensor:
    """The reference's exact call shape, grid_opt/models/grid_modules.py:86-94.

    feature (1,C,Z,Y,X), xn (N,3) normalised -> (N,C).
    """
    n = xn.shape[0]
    out = F.grid_sample(feature, xn.reshape(1, n, 1, 1, 3), mode="bilinear",
                        align_corners=align_corners, padding_mode=padding_mode)
    return out[0, :, :, 0, 0].transpose(0, 1)


def trilinear_gather(feature: torch.Tensor, xn: torch.Tensor,
                     align_corners: bool = False,
                     padding_mode: str = "zeros") -> torch.Tensor:
    """Explicit 8-corner trilinear sample, differentiable to any order.

    Same semantics as ATen ``grid_sampler_3d`` (bilinear): weights are
    ``(i0+1-ix)`` / ``(ix-i0)`` products, out-of-range corners contribute zero
    (``zeros``) or coordinates are clipped first (``border``); corner naming and
    weights as in third_party/cuda_gridsample_grad2/gridsample_cuda.cu:302-342.

    For FINITE grids: an out-of-range corner's clamped neighbour is multiplied by a 0 mask, so a NaN or inf vertex
    there would reach rows that ATen (and the kernels) keep finite; ``trilinear_first64`` selects instead.
    """
    assert feature.ndim == 5 and feature.shape[0] == 1
    assert padding_mode in ("zeros", "border")
    _, c, d, h, w = feature.shape
    flat = feature.reshape(c, d * h * w)
    coords = []
    for axis, size in ((0, w), (1, h), (2, d)):
        i = _unnormalize(xn[:, axis], size, align_corners)
        if padding_mode == "border":
            # ATen clip_coordinates_set_grad (gridsample_cuda.cu:297-299): the clipped coordinate carries no
            # gradient at either limit or beyond it (torch.clamp would pass it through at the limits themselves)
            clip = (i <= 0) | (i >= size - 1)
            i = torch.where(clip, i.detach().clamp(0, size - 1), i)
        coords.append(i)
    ix, iy, iz = coords
    x0 = torch.floor(ix).detach()
    y0 = torch.floor(iy).detach()
    z0 = torch.floor(iz).detach()
    out = 0
    for dz in (0, 1):
        wz = (iz - z0) if dz else (z0 + 1 - iz)
        zi = z0 + dz
        for dy in (0, 1):
            wy = (iy - y0) if dy else (y0 + 1 - iy)
            yi = y0 + dy
            for dx in (0, 1):
                wx = (ix - x0) if dx else (x0 + 1 - ix)
                xi = x0 + dx
                inb = ((xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                       & (zi >= 0) & (zi < d))
                lin = (zi.clamp(0, d - 1) * h + yi.clamp(0, h - 1)) * w + xi.clamp(0, w - 1)
                vals = flat[:, lin.long()].transpose(0, 1)           # (N,C)
                wgt = (wx * wy * wz) * inb.to(feature.dtype)
                out = out + vals * wgt.unsqueeze(1)
    return out


def encode_stock(features: Sequence[torch.Tensor], bound: torch.Tensor,
                 x: torch.Tensor,
                 ignore_level: Optional[Sequence[bool]] = None) -> torch.Tensor:
    """grid_opt/utils/utils.py:143-164 (level loop + cat) with
    FeatureGrid.interpolate (grid_modules.py:72-95) inlined, stock ATen ops."""
    feats = []
    for lvl, f in enumerate(features):
        xn = normalize_coordinates(x, bound.to(x))
        v = grid_sample_stock(f, xn)
        if ignore_level is not None and ignore_level[lvl]:
            v = torch.zeros_like(v)
        feats.append(v)
    return torch.cat(feats, dim=1)


def encode_gather(features: Sequence[torch.Tensor], bound: torch.Tensor,
                  x: torch.Tensor,
                  ignore_level: Optional[Sequence[bool]] = None) -> torch.Tensor:
    """Same as ``encode_stock`` on the any-order-differentiable restatement."""
    feats = []
    for lvl, f in enumerate(features):
        xn = normalize_coordinates(x, bound.to(x))
        v = trilinear_gather(f, xn)
        if ignore_level is not None and ignore_level[lvl]:
            v = torch.zeros_like(v)
        feats.append(v)
    return torch.cat(feats, dim=1)


# --------------------------------------------------------------------------- #
# Second backward of the sampler (gridsample_grad2.grad2_3d), two independent ways
# --------------------------------------------------------------------------- #
def trilinear_bwd2(feature, xn, gout, ggx=None, ggf=None, align_corners=False, padding_mode="zeros"):
    """Double backward of ``trilinear_gather`` by autograd: with cotangents ``ggx`` (N,3) of grad_x and ``ggf``
    (shape of feature) of grad_feature, returns (gg_out (N,C), g_x (N,3), g_feature) -- the three outputs of
    gridsample_grad2.grad2_3d.  Valid everywhere (lattice planes and border clip limits included: the one-sided
    floor / set-grad conventions of ATen are built into the restatement)."""
    f = feature.detach().requires_grad_(True)
    x = xn.detach().requires_grad_(True)
    go = gout.detach().requires_grad_(True)
    out = trilinear_gather(f, x, align_corners, padding_mode)
    gf, gx = torch.autograd.grad(out, [f, x], go, create_graph=True)
    s = 0
    if ggx is not None:
        s = s + (gx * ggx).sum()
    if ggf is not None:
        s = s + (gf * ggf).sum()
    if not torch.is_tensor(s) or not s.requires_grad:
        return torch.zeros_like(gout), torch.zeros_like(xn), torch.zeros_like(feature)
    r = torch.autograd.grad(s, [go, x, f], allow_unused=True)
    return tuple(torch.zeros_like(t) if g is None else g for g, t in zip(r, (gout, xn, feature)))


def fd_safe(xn, sizes_xyz, align_corners, margin=1e-3):
    """(N,) bool: every unnormalised coordinate lies at least ``margin`` index units from an integer (cell planes
    and both clip limits are integers) and is finite -- where ``grid_sample_bwd2_aten``'s differences stay in a cell."""
    ok = torch.ones(xn.shape[0], dtype=torch.bool, device=xn.device)
    for axis, size in enumerate(sizes_xyz):
        i = _unnormalize(xn[:, axis].double(), size, align_corners)
        ok &= torch.isfinite(i) & ((i - torch.round(i)).abs() >= margin)
    return ok


def _fd5(fn, h):
    """d/dt fn(t) at 0, five-point stencil: exact up to rounding for polynomials of degree <= 4 (the trilinear
    interpolant and its gradient are of degree <= 3 along a line that stays in one cell)."""
    return (8 * (fn(h) - fn(-h)) - (fn(2 * h) - fn(-2 * h))) / (12 * h)


def grid_sample_bwd2_aten(feature, xn, gout, ggx=None, ggf=None, padding_mode="zeros", align_corners=False,
                          step=2.0 ** -12):
    """The second backward of the sampler from ATen alone: ``F.grid_sample`` and its first backward, fp64.

    With E(f; x) the sample and phi(x) = <gout, E(feature; x)>:
      gg_out    = D_ggx E(feature; x) + E(ggf; x)
      g_x       = D_ggx grad_x phi(x) + grad_x <gout, E(ggf; x)>            (the Hessian of phi is symmetric)
      g_feature = D_ggx grad_feature phi(x)
    where D_ggx is the derivative along each point's ggx, taken by a five-point difference of exact ATen calls along
    the unit direction (step ``step`` index units on the finest axis) and scaled by |ggx|.  The interpolant is
    multilinear within a cell, so the difference is exact up to rounding wherever the stencil stays in one cell:
    the returned mask ``fd_safe`` marks those points (1e-3 index units from every integer); elsewhere the values are
    not an oracle.  Returns (gg_out, g_x, g_feature, safe), fp64."""
    feature, xn, gout = feature.double(), xn.double(), gout.double()
    _, c, d, h, w = feature.shape
    n = xn.shape[0]
    scale = max([(s - 1) / 2 if align_corners else s / 2 for s in (w, h, d)] + [1e-30])
    hn = step / scale                                           # normalised step: <= ``step`` index units per axis
    if ggx is not None:
        ggx = ggx.double()
        nrm = ggx.norm(dim=1, keepdim=True)
        u = torch.where(nrm > 0, ggx / torch.where(nrm > 0, nrm, torch.ones_like(nrm)), torch.zeros_like(ggx))
    gg_out = torch.zeros(n, c, dtype=torch.float64)
    g_x = torch.zeros(n, 3, dtype=torch.float64)
    g_f = torch.zeros_like(feature)

    def E(f, x):
        return grid_sample_stock(f, x, align_corners, padding_mode)

    def vjp(f, x, go, wrt_f):
        f_ = f.detach().requires_grad_(wrt_f)
        x_ = x.detach().requires_grad_(not wrt_f)
        out = E(f_, x_)
        (g,) = torch.autograd.grad(out, [f_ if wrt_f else x_], go)
        return g

    if ggx is not None:
        gg_out = gg_out + nrm * _fd5(lambda t: E(feature, xn + t * u), hn)
        g_x = g_x + nrm * _fd5(lambda t: vjp(feature, xn + t * u, gout, False), hn)
        g_f = g_f + _fd5(lambda t: vjp(feature, xn + t * u, gout * nrm, True), hn)
    if ggf is not None:
        gg_out = gg_out + E(ggf.double(), xn)
        g_x = g_x + vjp(ggf.double(), xn, gout, False)
    return gg_out, g_x, g_f, fd_safe(xn, (w, h, d), align_corners)


def _encode_bwd2(one, features, bound, x, gout, ggx, ggf, ignore_level):
    x = x.double()
    bound = bound.double().to(x.device)
    xn = normalize_coordinates(x, bound)
    sc = (2 / (bound[:, 1] - bound[:, 0])).view(1, 3)          # d xn / d x
    n = x.shape[0]
    gg_out = torch.zeros(n, gout.shape[1], dtype=torch.float64)
    g_x = torch.zeros(n, 3, dtype=torch.float64)
    g_f, safe = [], torch.ones(n, dtype=torch.bool)
    c0 = 0
    for l, f in enumerate(features):
        c = f.shape[1]
        if ignore_level is not None and ignore_level[l]:
            g_f.append(torch.zeros_like(f, dtype=torch.float64))
        else:
            r = one(f, xn, gout[:, c0:c0 + c], None if ggx is None else ggx.double() * sc,
                    None if ggf is None else ggf[l])
            gg_out[:, c0:c0 + c] = r[0]
            g_x += r[1] * sc
            g_f.append(r[2])
            if len(r) > 3:
                safe &= r[3]
        c0 += c
    return gg_out, g_x, g_f, safe


def encode_bwd2_aten(features, bound, x, gout, ggx=None, ggf=None, ignore_level=None):
    """``grid_sample_bwd2_aten`` in the encode form (metres, levels concatenated, zeros padding, align_corners=False):
    (gg_out (N,F), g_x (N,3) per metre, [g_feature per level], safe (N,)) in fp64.  ``ggf``: per level or None."""
    return _encode_bwd2(lambda f, xn, go, e, gg: grid_sample_bwd2_aten(f, xn, go, e, gg, "zeros", False),
                        features, bound, x, gout, ggx, ggf, ignore_level)


def encode_bwd2_gather(features, bound, x, gout, ggx=None, ggf=None, ignore_level=None):
    """The same three outputs by autograd through ``trilinear_gather`` (any dtype of the inputs: fp64 for the oracle,
    fp32 to measure what a float32 evaluation of the formula costs).  Returns (gg_out, g_x, [g_feature])."""
    dt = features[0].dtype
    x = x.to(dt)
    bound = bound.to(dt).to(x.device)
    xn = normalize_coordinates(x, bound)
    sc = (2 / (bound[:, 1] - bound[:, 0])).view(1, 3)
    n = x.shape[0]
    gg_out = torch.zeros(n, gout.shape[1], dtype=dt)
    g_x = torch.zeros(n, 3, dtype=dt)
    g_f = []
    c0 = 0
    for l, f in enumerate(features):
        c = f.shape[1]
        if ignore_level is not None and ignore_level[l]:
            g_f.append(torch.zeros_like(f))
        else:
            r = trilinear_bwd2(f, xn, gout[:, c0:c0 + c].to(dt), None if ggx is None else ggx.to(dt) * sc,
                               None if ggf is None or ggf[l] is None else ggf[l].to(dt), False, "zeros")
            gg_out[:, c0:c0 + c] = r[0]
            g_x += r[1] * sc
            g_f.append(r[2])
        c0 += c
    return gg_out, g_x, g_f


# --------------------------------------------------------------------------- #
# Decoder
# --------------------------------------------------------------------------- #
def mlp_forward(feats: torch.Tensor, weights: Sequence[torch.Tensor],
                biases: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
    """grid_opt/models/modules.py:16-21,31-32: Linear/ReLU chain, no activation
    after the last Linear.  ``weights[i]`` is (out,in) like ``nn.Linear.weight``."""
    h = feats
    last = len(weights) - 1
    for i, (w, b) in enumerate(zip(weights, biases)):
        h = F.linear(h, w, b)
        if i != last:
            h = torch.relu(h)
    return h


def decoder_params(state_dict) -> Tuple[List[torch.Tensor], List[Optional[torch.Tensor]]]:
    """Split an ``MLPNet`` state-dict (keys ``network.{0,2,4,..}.{weight,bias}``,
    modules.py:16-21) into ordered weight / bias lists."""
    idx = sorted({int(k.split(".")[1]) for k in state_dict if k.startswith("network.")})
    ws = [state_dict[f"network.{i}.weight"] for i in idx]
    bs = [state_dict.get(f"network.{i}.bias") for i in idx]
    return ws, bs


def sdf_stock(features, bound, x, weights, biases, ignore_level=None):
    """GridNet.forward, grid_opt/models/grid_net.py:306-325 (pos_invariant)."""
    return mlp_forward(encode_stock(features, bound, x, ignore_level), weights, biases)


def sdf_gather(features, bound, x, weights, biases, ignore_level=None):
    return mlp_forward(encode_gather(features, bound, x, ignore_level), weights, biases)


# --------------------------------------------------------------------------- #
# Losses on the hot path
# --------------------------------------------------------------------------- #
def miso_loss_regression(pred, targ, valid_mask=None, sample_weights=None, loss_type="L1"):
    """grid_opt/loss.py:594-635 -- mean over ALL rows including masked ones."""
    n = pred.shape[0]
    if valid_mask is None:
        valid_mask = torch.ones((n, 1)).to(pred)
    if sample_weights is None:
        sample_weights = torch.ones((n, 1)).to(pred)
    if loss_type == "L2":
        v = torch.sum((pred - targ) ** 2, dim=1, keepdim=True)
    elif loss_type == "L1":
        v = torch.sum(torch.abs(pred - targ), dim=1, keepdim=True)
    elif loss_type == "Cosine":
        v = 1.0 - F.cosine_similarity(pred, targ, dim=1, eps=1e-8).unsqueeze(1)
    else:
        raise ValueError(loss_type)
    v = torch.where(valid_mask == 1, v, torch.zeros_like(v))
    return torch.mean(sample_weights * v)


def miso_loss_free_space(pred_sdf, gt_sdf, gt_sdf_sign, trunc_dist):
    """grid_opt/loss.py:668-700."""
    up = torch.where(gt_sdf_sign == 1, F.relu(pred_sdf - gt_sdf), torch.zeros_like(pred_sdf))
    lo = torch.where(gt_sdf_sign == 1, F.relu(trunc_dist - pred_sdf), torch.zeros_like(pred_sdf))
    return torch.mean(torch.maximum(up, lo))


# --------------------------------------------------------------------------- #
# Rigid-body maps (pose-Jacobian path)
# --------------------------------------------------------------------------- #
def hat(v: torch.Tensor) -> torch.Tensor:
    """pytorch3d.transforms.so3.hat restated (parity unpinned, see header):
    (B,3) -> (B,3,3) skew matrices."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    o = torch.zeros_like(x)
    return torch.stack([torch.stack([o, -z, y], -1),
                        torch.stack([z, o, -x], -1),
                        torch.stack([-y, x, o], -1)], -2)


def so3_exp_map(log_rot: torch.Tensor, eps: float = 1e-4) -> torch.Tensor:
    """pytorch3d.transforms.so3_exp_map restated (parity unpinned): Rodrigues
    with theta = sqrt(clamp(|w|^2, eps)).  Call sites in the reference:
    grid_opt/utils/utils_geometry.py:99, grid_opt/models/grid_net.py:7."""
    nrms = (log_rot * log_rot).sum(1)
    theta = torch.clamp(nrms, eps).sqrt()
    inv = 1.0 / theta
    fac1 = inv * theta.sin()
    fac2 = inv * inv * (1.0 - theta.cos())
    k = hat(log_rot)
    k2 = torch.bmm(k, k)
    eye = torch.eye(3, dtype=log_rot.dtype, device=log_rot.device)[None]
    return fac1[:, None, None] * k + fac2[:, None, None] * k2 + eye


def apply_pose_correction(R, t, R_delta, t_delta):
    """grid_opt/utils/utils_geometry.py:78-99: (R Exp(dr), t + dt)."""
    return torch.matmul(R, so3_exp_map(R_delta)[0]), t + t_delta


def transform_points_to(points_src, R_dst_src, t_dst_src):
    """grid_opt/utils/utils_geometry.py:214-225."""
    return points_src @ R_dst_src.T + t_dst_src.T


def transfrom_points_from(points_dst, R_dst_src, t_dst_src):
    """grid_opt/utils/utils_geometry.py:227-240 (sic: upstream spelling)."""
    return transform_points_to(points_dst, R_dst_src.T, -R_dst_src.T @ t_dst_src)


def transform_by_keyframe_loop(coords_frame, frame_ids, R_all, t_all):
    """The reference's per-keyframe loop (grid_opt/loss.py:763-774; same shape in loss_isdf.py:52-61 and
    align/miso.py:44-53): for every keyframe id present, the rows carrying it are mapped by
    transform_points_to with that keyframe's pose.  R_all (K,3,3), t_all (K,3,1)."""
    out = coords_frame.clone()
    for k in torch.unique(frame_ids).tolist():
        rows = torch.nonzero(frame_ids == k, as_tuple=False).squeeze(1)
        out[rows] = transform_points_to(coords_frame[rows], R_all[k], t_all[k])
    return out


def coords_in_bound(coords, bound):
    """grid_opt/utils/utils_geometry.py:11-27 -- inclusive box test, (N,1) bool."""
    return ((coords >= bound[:, 0]) & (coords <= bound[:, 1])).all(dim=1).unsqueeze(1)


def pairwise_latent_loss(feats_src, bound_src, feats_dst, bound_dst, coords_from,
                         R_src, t_src, R_dst, t_dst, level, fdim,
                         align_weight=3000.0, align_loss="L2", encode=encode_stock):
    """grid_opt/align/miso.py:116-211 on plain tensors (use_bound=True, no
    stability / truncation pruning, no subsampling)."""
    end_ch = fdim * (level + 1)
    world = transform_points_to(coords_from, R_src, t_src)
    coords_to = transfrom_points_from(world, R_dst, t_dst)
    mask = coords_in_bound(coords_to, bound_dst.to(coords_to))
    if torch.count_nonzero(mask) == 0:
        return torch.tensor(0)
    idx = torch.nonzero(mask, as_tuple=False)[:, 0]
    p_from = coords_from[idx]
    p_to = coords_to[idx]
    f_from = encode(feats_src, bound_src, p_from)[:, :end_ch]
    f_to = encode(feats_dst, bound_dst, p_to)[:, :end_ch]
    diff = f_from - f_to
    if align_loss == "L2":
        return torch.mean(diff ** 2) * align_weight
    if align_loss == "L1":
        return torch.mean(torch.linalg.vector_norm(diff, dim=1)) * align_weight
    raise ValueError(align_loss)


def lm_normal_equations(coords_frame, R, grad_world, sdf_pred, sdf_gt, loss_type="L2", gm_scale=0.1):
    """J (N,6), H = J^T W J, g = J^T W r of Tracker.lm_step (grid_opt/slam/tracker.py:176-196;
    weights :139-146; hat = pytorch3d.transforms.so3.hat, restated in `hat` above)."""
    Rx = coords_frame @ R.T
    cT = torch.bmm(hat(Rx), grad_world.unsqueeze(-1)).squeeze(-1)
    J = torch.cat((cT @ R, grad_world), dim=1)
    r = (sdf_pred - sdf_gt).reshape(-1, 1)
    if loss_type == "L2":
        w = torch.ones_like(r)
    elif loss_type == "GM":
        w = gm_scale / (gm_scale + r ** 2) ** 2
    else:
        raise ValueError(loss_type)
    return J, J.T @ (w * J), J.T @ (w * r)


# --------------------------------------------------------------------------- #
# Sample generation (the step that feeds the path).  Random draws are inputs.
# --------------------------------------------------------------------------- #
def ray_dirs_camera(H: int, W: int, fx, fy, cx, cy) -> torch.Tensor:
    """grid_opt/utils/utils_sample.py:10-30, depth_type 'z': (H,W,3) directions ((c-cx)/fx, (r-cy)/fy, 1)."""
    cols = torch.arange(W, dtype=torch.float32)[None, :].expand(H, W)
    rows = torch.arange(H, dtype=torch.float32)[:, None].expand(H, W)
    return torch.stack(((cols - cx) / fx, (rows - cy) / fy, torch.ones(H, W)), dim=-1)


def rgbd_sdf_samples(depth, T_WC, R_wk, t_wk, intrinsics, pix_b, pix_h, pix_w, u, g, *, min_depth,
                     dist_behind_surf, trunc_dist, n_strat, n_surf, normals=None, frame_ids=None):
    """PosedSdfRgbd.getitem_sdf, grid_opt/datasets/sdf_rgbd.py:381-483, with the random draws passed in.

    ``u`` (>= n1, n_strat) and ``g`` (>= n1, n_surf-1) are consumed by the n1 rays that survive the first filter
    (the reference draws them after that filter, utils_sample.py:241,284).  Returns the two dictionaries of
    :472-481 plus ``pc_world``, ``z_vals`` and the two ray counts."""
    B, H, W = depth.shape
    dirs = ray_dirs_camera(H, W, *intrinsics)
    d = depth[pix_b, pix_h, pix_w].reshape(-1)                      # utils_sample.py:156-157
    keep = d != 0
    if normals is not None:                                         # :160-166
        keep = keep & ~torch.isnan(normals[pix_b, pix_h, pix_w, 0])
    d, b, h, w = d[keep], pix_b[keep], pix_h[keep], pix_w[keep]
    n1 = d.numel()
    T = T_WC[b]
    dc = dirs[h, w]
    dw = (T[:, :3, :3] * dc[:, None, :]).sum(dim=-1)                # origin_dirs_W, :33-38
    org = T[:, :3, 3]
    far = d + dist_behind_surf                                      # sdf_rgbd.py:268
    span = (far - min_depth)[:, None]                               # stratified_sample, utils_sample.py:212-222
    edges = torch.linspace(0, 1, n_strat + 1)[None, :].repeat(n1, 1) * span + min_depth
    z = edges[:, :-1] + u[:n1] * (span / n_strat)                   # :241-244
    if n_surf == 1:                                                 # :278-281
        z = torch.cat((d[:, None], z), dim=1)
    elif n_surf > 1:                                                # :283-297
        near = torch.clamp(d[:, None] + g[:n1], torch.full((n1, 1), float(min_depth)), far[:, None])
        z = torch.cat((d[:, None], near, z), dim=1)
    pc = org[:, None, :] + dw[:, None, :] * z[:, :, None]           # :300
    sdf = dc.norm(dim=-1)[:, None] * (d[:, None] - z)               # bounds_ray, sdf_rgbd.py:525-528
    ok = ~torch.isnan(pc).reshape(n1, -1).any(dim=1)                # :416-424
    pc, sdf, b, z = pc[ok], sdf[ok], b[ok], z[ok]
    S = z.shape[1]
    ids = (b if frame_ids is None else frame_ids[b])[:, None].expand(-1, S).reshape(-1)   # :427-432
    world = pc.reshape(-1, 3)
    rb = b[:, None].expand(-1, S).reshape(-1)
    Rk, tk = R_wk[rb], t_wk.reshape(-1, 3)[rb]
    t_inv = -(Rk.transpose(1, 2) @ tk[:, :, None])[:, :, 0]         # transfrom_points_from, utils_geometry.py:227-240
    coords = (world[:, None, :] @ Rk)[:, 0, :] + t_inv              # x R + t_inv^T   (:436-445)
    sdf = sdf.reshape(-1, 1)
    sign = torch.zeros_like(sdf)                                    # :452-455
    sign[sdf < -trunc_dist] = -1
    sign[sdf > trunc_dist] = 1
    inputs = {"coords_frame": coords, "sample_frame_ids": ids[:, None].long(), "weights": torch.ones_like(sdf)}
    gt = {"sdf": sdf, "sdf_valid": sdf.abs() < trunc_dist, "sdf_signs": sign}
    return inputs, gt, {"pc_world": world, "z_vals": z, "n_first": n1, "n_kept": int(ok.sum())}


def lidar_distance_weight(dists, max_range, scale=0.8):
    """PosedSdf3DLidar.distance_weight_func, grid_opt/datasets/sdf_3d_lidar.py:205-211."""
    return 1 + scale * 0.5 - (dists / max_range) * scale


def lidar_frame_samples(pts_world, R_wf, t_wf, g_near, u_free, u_behind, *, near_surface_n, near_surface_std,
                        free_space_n, behind_surface_n, trunc_dist, min_dist_ratio, max_range):
    """One frame of PosedSdf3DLidar.sample_frames, grid_opt/datasets/sdf_3d_lidar.py:214-347 (after the
    sub-sampling permutation :233-237), draws passed in: g_near (n*near_n,1) standard normals, u_free
    (n*free_n,1) and u_behind (n*behind_n,1) uniforms.  fp64 like the reference's numpy, cast at :340-345."""
    p = pts_world.double()
    eye = t_wf.reshape(1, 3).double()
    dist = (p - eye).norm(dim=1, keepdim=True)                       # :240
    pts, sdfs, wts, sgn = [p], [torch.zeros_like(dist)], [lidar_distance_weight(dist, max_range)], [torch.zeros_like(dist)]

    def along(rep, d_new):
        rp = p.repeat_interleave(rep, dim=0)
        direc = rp - eye
        direc = direc / (direc.norm(dim=1, keepdim=True) + 1e-8)
        return eye + direc * d_new

    if near_surface_n > 0:                                           # :252-265
        rd = dist.repeat_interleave(near_surface_n, dim=0)
        dn = rd + g_near.double() * near_surface_std
        pts.append(along(near_surface_n, dn))
        sdfs.append((rd - dn).float().double())
        wts.append(lidar_distance_weight(rd, max_range))
        sgn.append(torch.zeros_like(rd))
    if free_space_n > 0:                                             # :270-285
        rd = dist.repeat_interleave(free_space_n, dim=0)
        span = torch.clamp((1.0 - trunc_dist / rd) - min_dist_ratio, min=1e-2)
        disp = ((min_dist_ratio + u_free.double() * span) - 1.0) * rd
        pts.append(along(free_space_n, rd + disp))
        sdfs.append((-disp.float()).double())
        wts.append(torch.ones_like(rd))
        sgn.append(torch.ones_like(rd))
    if behind_surface_n > 0:                                         # :290-302
        rd = dist.repeat_interleave(behind_surface_n, dim=0)
        disp = near_surface_std + u_behind.double() * (4 * near_surface_std - 2 * near_surface_std)
        pts.append(along(behind_surface_n, rd + disp))
        sdfs.append((-disp.float()).double())
        wts.append(torch.ones_like(rd))
        sgn.append(-torch.ones_like(rd))
    world = torch.cat(pts).float()                                   # :307-323
    sdf = torch.cat(sdfs).float()
    frame = transfrom_points_from(world, R_wf.float(), t_wf.reshape(3, 1).float())
    return {"points_frame": frame, "points_world_gt": world, "sdfs": sdf,
            "sdfs_valid": (sdf.abs() < trunc_dist).float(), "signs": torch.cat(sgn).float(),
            "weights": torch.cat(wts).float()}


# --------------------------------------------------------------------------- #
# Latent alignment at the kernel's own fp32 coordinates (pair_latent.hip, align.hip)
# --------------------------------------------------------------------------- #
def index32(xn32, size, align_corners=False):
    """The kernel's axis_from_norm on an fp32 normalised coordinate (common.hpp), fp32 step by step.  Without
    OCML_BASIC_ROUNDED_OPERATIONS HIP's __fmul_rn / __fsub_rn are plain operators, and the compiler contracts
    (xn + 1) * size - 1 into one fma: a single rounding, replayed here through the exact fp64 product."""
    one = torch.tensor(1.0, dtype=torch.float32)
    a = xn32 + one
    if align_corners:
        return (a * torch.tensor(0.5, dtype=torch.float32)) * torch.tensor(float(size - 1), dtype=torch.float32)
    return (a.double() * size - 1).float() * torch.tensor(0.5, dtype=torch.float32)


def norm32(x32, bound):
    """axis_norm's fp32 normalisation of metres (common.hpp): 2 (x - bmin) / len - 1, rounded after each step.
    bound: (3,2) rows [min, max]."""
    b = torch.as_tensor(bound, dtype=torch.float32)
    return (torch.tensor(2.0, dtype=torch.float32) * (x32 - b[:, 0])) / (b[:, 1] - b[:, 0]) - \
        torch.tensor(1.0, dtype=torch.float32)


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64, the sum rounds there and again to fp32 -- a double
    rounding that differs from one fma in about 1 case of 2^29."""
    return (a.double() * b.double() + c.double()).float()


def src_to_dst32(p, Rs, ts, Rd, td, bound=None):
    """pair_latent.hip src_to_dst in fp32, operation by operation: w_r = fma(Rs[r,2], z, fma(Rs[r,1], y, Rs[r,0] x))
    + ts_r, d = w - td, q_c = fma(Rd[2,c], d_2, fma(Rd[1,c], d_1, Rd[0,c] d_0)).  The source writes these with
    __fmaf_rn / __fmul_rn / __fadd_rn / __fsub_rn; the gfx950 code of overlap_count_kernel (hipcc -O3 -S) is
    v_mul_f32, two v_fmac_f32, v_add_f32 (ts), v_subrev_f32 (td) per row of Rs and v_mul / v_fma (v_pk_fma_f32 for
    two columns) in this order for Rd^T: nothing is contracted or reassociated beyond what the source writes.
    p (N,3), R (3,3), t (3,) fp32 -> d (N,3), q (N,3) fp32 and, with a (3,2) bound, the inclusive in-bound mask.
    A count that differs from the kernel's by one: look at that vertex for the double rounding of _fma32 first."""
    f = lambda t: torch.as_tensor(t, dtype=torch.float32).reshape(-1)
    p = p.to(torch.float32)
    Rs, ts, Rd, td = f(Rs).view(3, 3), f(ts), f(Rd).view(3, 3), f(td)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    d = torch.stack([(_fma32(Rs[r, 2], pz, _fma32(Rs[r, 1], py, Rs[r, 0] * px)) + ts[r]) - td[r] for r in range(3)], 1)
    q = torch.stack([_fma32(Rd[2, c], d[:, 2], _fma32(Rd[1, c], d[:, 1], Rd[0, c] * d[:, 0])) for c in range(3)], 1)
    if bound is None:
        return d, q
    b = torch.as_tensor(bound, dtype=torch.float32)
    return d, q, ((q >= b[:, 0]) & (q <= b[:, 1])).all(1)


def _trilinear_jet(feature, ix, dtype):
    """Value (N,C) and index-space derivative (N,C,3) of the zero-padded trilinear interpolant in the cell of
    floor(ix) (ATen's convention), plus sum_corners |v| (N,C): ix (N,3) fp64 index coordinates (x, y, z)."""
    _, c, d, h, w = feature.shape
    flat = feature.detach().reshape(c, d * h * w).to(dtype)
    i0 = torch.floor(ix)
    fr = (ix - i0).to(dtype)
    i0 = i0.clamp(-2, max(w, h, d) + 1).long()
    n = ix.shape[0]
    val = torch.zeros(n, c, dtype=dtype)
    der = torch.zeros(n, c, 3, dtype=dtype)
    mag = torch.zeros(n, c, dtype=dtype)
    for k in range(8):
        o = (k & 1, (k >> 1) & 1, k >> 2)
        xi, yi, zi = i0[:, 0] + o[0], i0[:, 1] + o[1], i0[:, 2] + o[2]
        inb = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (zi >= 0) & (zi < d)
        lin = ((zi.clamp(0, d - 1) * h + yi.clamp(0, h - 1)) * w + xi.clamp(0, w - 1))
        v = flat[:, lin].t() * inb.to(dtype)[:, None]
        wt = [fr[:, a] if o[a] else 1 - fr[:, a] for a in range(3)]
        sg = [1.0 if o[a] else -1.0 for a in range(3)]
        val += v * (wt[0] * wt[1] * wt[2])[:, None]
        der[:, :, 0] += v * (sg[0] * wt[1] * wt[2])[:, None]
        der[:, :, 1] += v * (sg[1] * wt[0] * wt[2])[:, None]
        der[:, :, 2] += v * (sg[2] * wt[0] * wt[1])[:, None]
        mag += v.abs()
    return val, der, mag


# --------------------------------------------------------------------------- #
# The sampled value and its first coordinate gradient at the kernel's own fp32 index coordinate (trilinear.hpp)
# --------------------------------------------------------------------------- #
def mult32(bound_axis, size, align_corners=False):
    """The kernel's d ix / d x on one axis as an fp32 scalar tensor, rounded where axis_norm / axis_from_norm round:
    fl(fl(2 / len) * (0.5 * size)), 0.5 * (size - 1) under align_corners (0.5 * size is exact).  A binned batch forms
    the same number as gscale * mult (gscale = fl(2 / len) on the host, mult = 0.5 * size).  bound_axis: (min, max), or
    None for normalised coordinates (mult alone, exact)."""
    half = torch.tensor(0.5, dtype=torch.float32) * torch.tensor(float(size - 1 if align_corners else size),
                                                                 dtype=torch.float32)
    if bound_axis is None:
        return half
    lo, hi = (torch.tensor(float(v), dtype=torch.float32) for v in bound_axis)
    return (torch.tensor(2.0, dtype=torch.float32) / (hi - lo)) * half


def sample_index32(x32, bound, sizes_xyz, align_corners=False, padding_mode="zeros"):
    """One level's index coordinate and d ix / d x as the kernels form them (axis_norm, axis_from_norm), carried to fp64
    exactly: x32 (N,3) fp32 metres -- normalised coordinates where ``bound`` is None -- -> (ix (N,3), mult (N,3)) fp64.
    ``border`` padding replays the clip in fp32: ix <= 0 -> 0, ix >= size - 1 -> size - 1, and mult = 0 at and beyond
    both limits (ATen's clip_coordinates_set_grad).  A NaN coordinate stays NaN (no comparison holds)."""
    xn = x32 if bound is None else norm32(x32, bound)
    ix, mult = [], []
    for a, size in enumerate(sizes_xyz):
        i = index32(xn[:, a], size, align_corners).double()
        m = mult32(None if bound is None else bound[a], size, align_corners).double().expand(i.shape[0]).clone()
        if padding_mode == "border":
            clip = (i <= 0) | (i >= size - 1)
            i = torch.where(clip, i.clamp(0, size - 1), i)
            m = torch.where(clip, torch.zeros_like(m), m)
        ix.append(i)
        mult.append(m)
    return torch.stack(ix, 1), torch.stack(mult, 1)


def _trilinear_jet_select(feature, ix):
    """_trilinear_jet in fp64 with out-of-range corners SELECTED to zero (torch.where), as ATen skips them
    (within_bounds_3d): a NaN or inf vertex reaches exactly the rows that have it as an in-range corner of their
    cell, whatever its weight (0 x NaN = NaN there), and no other.  A row with a non-finite index coordinate has no
    corner in range (axis_cell).  -> value (N,C), d value / d ix (N,C,3), sum_k |v_k| w_k (N,C), sum_k |v_k| over the
    in-range corners (N,C), sum_k |v_k| x the other two axes' weights (N,C,3)."""
    _, c, d, h, w = feature.shape
    flat = feature.detach().reshape(c, d * h * w).double()
    ix = ix.double()
    bad = ~torch.isfinite(ix).all(1)
    ix = torch.where(bad[:, None], torch.full_like(ix, -4.0), ix)
    i0 = torch.floor(ix)
    fr = ix - i0
    i0 = i0.clamp(-2, max(w, h, d) + 1).long()
    n = ix.shape[0]
    zero = torch.zeros((), dtype=torch.float64)
    val, yw, yc = (torch.zeros(n, c, dtype=torch.float64) for _ in range(3))
    der, yd = (torch.zeros(n, c, 3, dtype=torch.float64) for _ in range(2))
    for k in range(8):
        o = (k & 1, (k >> 1) & 1, k >> 2)
        xi, yi, zi = i0[:, 0] + o[0], i0[:, 1] + o[1], i0[:, 2] + o[2]
        inb = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (zi >= 0) & (zi < d)
        lin = ((zi.clamp(0, d - 1) * h + yi.clamp(0, h - 1)) * w + xi.clamp(0, w - 1))
        v = torch.where(inb[:, None], flat[:, lin].t(), zero)
        wt = [fr[:, a] if o[a] else 1 - fr[:, a] for a in range(3)]
        sg = [1.0 if o[a] else -1.0 for a in range(3)]
        w3 = (wt[0] * wt[1] * wt[2])[:, None]
        val += v * w3
        yw += v.abs() * w3
        yc += v.abs()
        for a, (p, q) in enumerate(((1, 2), (0, 2), (0, 1))):
            der[:, :, a] += v * (sg[a] * wt[p] * wt[q])[:, None]
            yd[:, :, a] += v.abs() * (wt[p] * wt[q])[:, None]
    return val, der, yw, yc, yd


class First64(NamedTuple):
    """trilinear_first64's answer.  value (N,F) and grad_x (N,3); the absolute-value yardsticks of each:
    value_w = sum_k |v_k| w_k and value_c = sum_k |v_k| over the in-range corners (N,F);
    grad_w = sum_levels |mult| sum_c |gF_c| sum_k |v_ck| x (the other two axes' weights) and
    grad_c = sum_levels |mult| sum_k sum_c |gF_c| |v_ck| (N,3)."""
    value: torch.Tensor
    grad_x: torch.Tensor
    value_w: torch.Tensor
    value_c: torch.Tensor
    grad_w: torch.Tensor
    grad_c: torch.Tensor


def trilinear_first64(features, ix, gout, mults):
    """The multi-level trilinear sample and its first coordinate gradient in fp64.  features: the levels (1,C,Z,Y,X);
    ix: per level the (N,3) index coordinates (x, y, z) -- sample_index32's, the kernel's own, so that a row on a cell
    plane is in the same cell on both sides -- or None for an ignored level (zero columns, nothing in grad_x); gout
    (N,F) the cotangent of the value; mults: per level (N,3) d ix / d x (the gscale x mult of the kernels; 0 on an axis
    the border clip holds).  The cell is the one of floor(ix) (ATen's); out-of-range corners are selected to zero, so
    non-finite grid values propagate as in ATen (_trilinear_jet_select).  Rows with a non-finite index coordinate are
    zero in both outputs."""
    n = gout.shape[0]
    F_ = sum(int(f.shape[1]) for f in features)
    value, value_w, value_c = (torch.zeros(n, F_, dtype=torch.float64) for _ in range(3))
    grad_x, grad_w, grad_c = (torch.zeros(n, 3, dtype=torch.float64) for _ in range(3))
    foff = 0
    for f, i, m in zip(features, ix, mults):
        c = int(f.shape[1])
        if i is not None:
            val, der, yw, yc, yd = _trilinear_jet_select(f, i)
            g = gout[:, foff:foff + c].double()
            m = m.double()
            value[:, foff:foff + c], value_w[:, foff:foff + c], value_c[:, foff:foff + c] = val, yw, yc
            grad_x += m * (g[:, :, None] * der).sum(1)
            grad_w += m.abs() * (g.abs()[:, :, None] * yd).sum(1)
            grad_c += m.abs() * (g.abs() * yc).sum(1)[:, None]
        foff += c
    return First64(value, grad_x, value_w, value_c, grad_w, grad_c)


def pair_latent_sums64(p, fsrc, feats_dst, bound, pose, loss_type="L2", ignore_mask=0, dtype=torch.float64,
                       exact=False, level_sign=None):
    """The 24 sums of miso_pair_latent (torch_ops.pair_latent_fwd_bwd: [0] sum term, [1] in-bound count, [2:5] sum g,
    [5+3a+b] sum d_a g_b, [14+3a+b] sum (Rd g)_a p_b) evaluated at the kernel's own fp32 mapped coordinates.

    p (N,3) fp32 source vertices, fsrc (N, >= F) source features, feats_dst the destination levels (1,C,Z,Y,X),
    bound (3,2), pose (24,) = R_s, t_s, R_d, t_d.  The in-bound set is src_to_dst32's; the normalised and index
    coordinates are norm32 / index32 of that q, carried to fp64 exactly; from there on everything is ``dtype``
    (fp64: the oracle; fp32: what a careful fp32 implementation at the same coordinates computes, summed in fp32 over
    runs of 8 vertices like a kernel lane).  Returns (sums (24,) fp64, A (24,) fp64): A is the same sum built from
    per-vertex absolute bounds -- |term|; a_i = sum_l mult_l sum_c |d term / d f_c| sum_corners |v| per axis (|d w / d ix|
    <= 1 in a cell); sum_c (|Rs||p| + |ts - td|)_a a_b for the d sums (the kernel forms them as Rs S + (ts - td) G,
    so d's terms count separately); sum_c |Rd_ac| a_c |p_b| for the last nine.  A[1] = 0: the count is exact.
    exact=True: the map, the bound test and the coordinates in fp64 from fp64 inputs instead (the formulas alone,
    for comparing with autograd through pairwise_latent_loss in fp64).
    level_sign: optional (N, levels) of +-1 multiplying each level's share of g per source vertex -- the sums a kernel
    that got a level's gradient sign wrong on those vertices would produce (for the sensitivity tests)."""
    pose = torch.as_tensor(pose, dtype=torch.float64 if exact else torch.float32).reshape(24)
    Rs, ts, Rd, td = pose[:9].view(3, 3), pose[9:12], pose[12:21].view(3, 3), pose[21:24]
    if exact:
        b64 = torch.as_tensor(bound, dtype=torch.float64)
        q = (p.double() @ Rs.T + (ts - td)) @ Rd
        m = ((q >= b64[:, 0]) & (q <= b64[:, 1])).all(1)
    else:
        b64 = torch.as_tensor(bound, dtype=torch.float32).double()
        _, q, m = src_to_dst32(p, Rs, ts, Rd, td, bound)
    idx = torch.nonzero(m).flatten()
    pi, qi = p[idx].to(torch.float64 if exact else torch.float32), q[idx]
    F_ = sum(int(f.shape[1]) for f in feats_dst)
    fs = fsrc[idx, :F_].to(dtype)
    xn = normalize_coordinates(qi, b64) if exact else norm32(qi, bound)
    fto, jac, mags, mults = [], [], [], []
    for l, f in enumerate(feats_dst):
        _, c, d, h, w = f.shape
        sizes = (w, h, d)
        ix = torch.stack([_unnormalize(xn[:, a], sizes[a], False) if exact else index32(xn[:, a], sizes[a]).double()
                          for a in range(3)], 1)
        mult = torch.tensor([sizes[a] / (b64[a, 1] - b64[a, 0]).item() for a in range(3)], dtype=dtype)
        v, dv, mg = _trilinear_jet(f, ix, dtype)
        if (ignore_mask >> l) & 1:
            v, dv, mg = torch.zeros_like(v), torch.zeros_like(dv), torch.zeros_like(mg)
        fto.append(v)
        if level_sign is not None:
            dv = dv * level_sign[idx, l].to(dtype)[:, None, None]
        jac.append(dv * mult)
        mags.append(mg[:, :, None] * mult)
    fto, jac, mags = torch.cat(fto, 1), torch.cat(jac, 1), torch.cat(mags, 1)     # (n,F), (n,F,3), (n,F,3)
    r = fs - fto
    if loss_type == "L2":
        term = (r * r).sum(1)
        dt = -2 * r
    elif loss_type == "L1":
        term = (r * r).sum(1).sqrt()
        inv = torch.where(term > 0, 1 / term, torch.zeros_like(term))            # vector_norm's backward at 0: 0
        dt = -r * inv[:, None]
    else:
        raise ValueError(loss_type)
    g = (dt[:, :, None] * jac).sum(1)                                             # (n,3) d term / d q
    a = (dt.abs()[:, :, None] * mags).sum(1)                                      # (n,3) bound on |g|
    Rs64, ts64, Rd64, td64 = Rs.double(), ts.double(), Rd.double(), td.double()
    p64 = pi.double()
    dvec = p64 @ Rs64.T + (ts64 - td64)                                           # d = Rs p + ts - td
    dabs = p64.abs() @ Rs64.abs().T + (ts64 - td64).abs()
    cnt = float(idx.numel())

    def total(x):
        """sum over vertices: fp64 directly, or fp32 over runs of 8 and then fp64"""
        x = x.reshape(x.shape[0], math.prod(x.shape[1:]))
        if dtype == torch.float64:
            return x.sum(0)
        pad = (-x.shape[0]) % 8
        x = torch.cat([x, x.new_zeros(pad, x.shape[1])]).view(-1, 8, x.shape[1])
        return x.sum(1).double().sum(0)

    g64, a64 = g, a
    sums = torch.zeros(24, dtype=torch.float64)
    A = torch.zeros(24, dtype=torch.float64)
    sums[0], A[0] = total(term)[0], total(term.abs())[0]
    sums[1] = cnt
    sums[2:5], A[2:5] = total(g64), total(a64)
    if dtype == torch.float64:
        sums[5:14] = (dvec[:, :, None] * g64[:, None, :]).sum(0).flatten()
        sums[14:23] = ((g64 @ Rd64.T)[:, :, None] * p64[:, None, :]).sum(0).flatten()
    else:       # the kernel's own decomposition: S = sum p (x) g in fp32, then Rs S + (ts - td) G and Rd S^T in fp64
        S = total(pi[:, :, None] * g[:, None, :]).view(3, 3)
        G = sums[2:5]
        sums[5:14] = (Rs64 @ S + (ts64 - td64)[:, None] * G[None, :]).flatten()
        sums[14:23] = (Rd64 @ S.T).flatten()
    a64 = a64.double()
    A[5:14] = (dabs[:, :, None] * a64[:, None, :]).sum(0).flatten()
    A[14:23] = ((a64 @ Rd64.abs().T)[:, :, None] * p64.abs()[:, None, :]).sum(0).flatten()
    return sums, A


def pair_sums_excess(got, sums, A, rel=1e-5):
    """(24,) how far each kernel sum lies beyond its bar: count exactly, the others |got - fp64| <= rel A + 1e-12.
    Positive entries are failures; NaN in ``got`` is a failure too."""
    got = torch.as_tensor(got, dtype=torch.float64).detach().cpu().reshape(24)
    ex = (got - sums).abs() - (rel * A + 1e-12)
    ex[1] = (got[1] - sums[1]).abs() if got[1] != sums[1] else -1.0
    ex[23] = got[23].abs()
    return torch.where(torch.isnan(ex), torch.full_like(ex, float("inf")), ex)


def pair_pose_grads64(sums, Rd, loss_type, n_ch, weight=1.0):
    """fp64 chain rule of ops._PairLatent on fp64 sums: loss, d/dR_s, d/dt_s, d/dR_d, d/dt_d."""
    denom = max(float(sums[1]), 1.0) * (n_ch if loss_type == "L2" else 1)
    s = weight / denom
    h = torch.as_tensor(Rd, dtype=torch.float64).reshape(3, 3) @ sums[2:5]
    return (sums[0] * s, sums[14:23].view(3, 3) * s, h.view(3, 1) * s, sums[5:14].view(3, 3) * s, -h.view(3, 1) * s)


def so3_exp_jacobian64(w):
    """d Exp(w)_ij / d w_k (3,3,3) in fp64 by autograd through so3_exp_map (its clamp of |w|^2 at 1e-4 included)."""
    w = torch.as_tensor(w, dtype=torch.float64).reshape(3)
    return torch.autograd.functional.jacobian(lambda v: so3_exp_map(v.view(1, 3))[0], w)


def so3_exp_backward64(w, G):
    """d sum(G * Exp(w)) / d w in fp64 (align.hpp so3_exp_backward)."""
    return torch.einsum("ijk,ij->k", so3_exp_jacobian64(w), torch.as_tensor(G, dtype=torch.float64).view(3, 3))


def align_epilogue64(out, cnt, pairs, S, pose, R0, params, *, loss_type="L2", align_weight=3000.0,
                     overlap_thresh=1e-2):
    """Epilogue A of align.hip in fp64 from given pair sums: per pair the normalisation, the overlap gate (decided
    on the fp32 fraction, as the kernel does), nan_to_num; per submap the sum of its pairs' cotangents, the pull-back
    through R = R0 Exp(dr) and so3_exp_map's backward.  out (P,24) fp64, cnt (P,) counts, pairs: dicts with src, dst,
    n_ch and gate_n (0: no gate); pose (S,12) the poses the sums were taken at; R0 (S,3,3); params (S,6).  Returns
    (pair losses (P,), flat (7S+1,) = 6S gradients, the loss sum, S "had a gradient" flags, and the same pull-back with
    every pair's sums and every matrix entry in absolute value (6S,): the yardstick of flat)."""
    out = torch.as_tensor(out, dtype=torch.float64).reshape(-1, 24)
    pose = torch.as_tensor(pose, dtype=torch.float64).reshape(S, 12)
    R0 = torch.as_tensor(R0, dtype=torch.float64).reshape(S, 3, 3)
    params = torch.as_tensor(params, dtype=torch.float32).reshape(S, 6)
    gR = torch.zeros(S, 3, 3, dtype=torch.float64)
    gt = torch.zeros(S, 3, dtype=torch.float64)
    aR = torch.zeros(S, 3, 3, dtype=torch.float64)
    at = torch.zeros(S, 3, dtype=torch.float64)
    had = torch.zeros(S, dtype=torch.bool)
    losses = torch.zeros(len(pairs), dtype=torch.float64)
    for i, pr in enumerate(pairs):
        o = out[i]
        denom = max(float(o[1]), 1.0) * (pr["n_ch"] if loss_type == "L2" else 1)
        val = float(o[0]) / denom
        finite = math.isfinite(float(torch.tensor(val, dtype=torch.float32)))
        gate = True
        if pr.get("gate_n", 0):
            frac = torch.tensor(float(cnt[i]), dtype=torch.float32) / torch.tensor(float(pr["gate_n"]),
                                                                                  dtype=torch.float32)
            gate = bool(frac > overlap_thresh)
        losses[i] = (float(torch.nan_to_num(torch.tensor(val, dtype=torch.float32))) * align_weight) if gate else 0.0
        s, d = int(pr["src"]), int(pr["dst"])
        had[s] |= gate
        had[d] |= gate
        if not (finite and gate):
            continue
        sc = align_weight / denom
        Rd = pose[d, :9].view(3, 3)
        h, ha = Rd @ o[2:5], Rd.abs() @ o[2:5].abs()
        gR[s] += o[14:23].view(3, 3) * sc
        gt[s] += h * sc
        gR[d] += o[5:14].view(3, 3) * sc
        gt[d] -= h * sc
        aR[s] += o[14:23].view(3, 3).abs() * sc
        aR[d] += o[5:14].view(3, 3).abs() * sc
        at[s] += ha * sc
        at[d] += ha * sc
    flat = torch.zeros(7 * S + 1, dtype=torch.float64)
    absf = torch.zeros(6 * S, dtype=torch.float64)
    for s in range(S):
        G = R0[s].T @ gR[s]
        Ga = R0[s].T.abs() @ aR[s]
        w = params[s, :3].double()
        J = so3_exp_jacobian64(w)
        flat[6 * s:6 * s + 3] = torch.einsum("ijk,ij->k", J, G)
        absf[6 * s:6 * s + 3] = torch.einsum("ijk,ij->k", J.abs(), Ga)      # the same map in absolute values
        flat[6 * s + 3:6 * s + 6] = gt[s]
        absf[6 * s + 3:6 * s + 6] = at[s]
        flat[6 * S + 1 + s] = float(had[s])
    flat[6 * S] = losses.sum()
    return losses, flat, absf


def align_epilogue_b64(flat, params, adam_m, adam_v, adam_t, *, lr=1e-2, betas=(0.9, 0.999), eps=1e-8,
                       reg_weight=0.0, reg_thresh_rad=1.0, reg_thresh_m=1.0):
    """Epilogue B of align.hip in fp64: the trust-region regulariser (grid_atlas_pose_trust_region_loss) on every
    submap, the NaN guard, and Adam on submaps 1..S-1 with a step count per submap; a submap without a gradient
    (none of its pairs passed the gate, no regulariser) keeps value, moments and count.  Returns (total loss,
    params, m, v, steps) -- the state after the step."""
    flat = torch.as_tensor(flat, dtype=torch.float64)
    prm = torch.as_tensor(params, dtype=torch.float64).clone().reshape(-1, 6)
    m = torch.as_tensor(adam_m, dtype=torch.float64).clone().reshape(-1, 6)
    v = torch.as_tensor(adam_v, dtype=torch.float64).clone().reshape(-1, 6)
    t = torch.as_tensor(adam_t).clone().to(torch.int64).reshape(-1)
    S = prm.shape[0]
    nr, nt = prm[:, :3].norm(dim=1), prm[:, 3:].norm(dim=1)
    total = float(flat[6 * S])
    if reg_weight > 0:
        total += float(reg_weight * (torch.relu(nr - reg_thresh_rad) + torch.relu(nt - reg_thresh_m)).sum())
    if math.isnan(total):
        return total, prm, m, v, t
    b1, b2 = betas
    for s in range(1, S):
        if not (reg_weight > 0 or flat[6 * S + 1 + s] > 0):
            continue
        g = flat[6 * s:6 * s + 6].clone()
        if reg_weight > 0:
            if nr[s] > reg_thresh_rad:
                g[:3] += reg_weight * prm[s, :3] / nr[s]
            if nt[s] > reg_thresh_m:
                g[3:] += reg_weight * prm[s, 3:] / nt[s]
        t[s] += 1
        m[s] = b1 * m[s] + (1 - b1) * g
        v[s] = b2 * v[s] + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** int(t[s]), 1 - b2 ** int(t[s])
        prm[s] -= lr / bc1 * m[s] / (v[s].sqrt() / math.sqrt(bc2) + eps)
    return total, prm, m, v, t


# --------------------------------------------------------------------------- #
# Keyframe tracker, stage by stage (lm.hip: miso_lm_track_step, miso_track_adam_step)
# --------------------------------------------------------------------------- #
def _t64(t):
    return torch.as_tensor(t).detach().cpu().to(torch.float64)


def track_pose64(R_base, t_base, dr, dt):
    """lm_pose_kernel in fp64: (12,) = R_base Exp(dr) row-major, then t_base + dt (apply_pose_correction; the clamp of
    |dr|^2 at 1e-4 is so3_exp_map's)."""
    R = _t64(R_base).reshape(3, 3) @ so3_exp_map(_t64(dr).reshape(1, 3), 1e-4)[0]
    return torch.cat([R.reshape(9), _t64(t_base).reshape(3) + _t64(dt).reshape(3)])


def track_transform32(x, pose12, sanitize=True):
    """lm_transform_kernel's map in fp32, operation by operation: per output axis j
    (fma(x2, R[j,2], fma(x1, R[j,1], x0 * R[j,0]))) + t_j, after torch.nan_to_num of x when ``sanitize``.
    Returns (xw (N,3) fp32, the sanitised x).  _fma32's double rounding: about 1 value in 2^29 may differ by an ulp."""
    x = torch.as_tensor(x).detach().cpu().to(torch.float32)
    if sanitize:
        x = torch.nan_to_num(x)
    p = torch.as_tensor(pose12).detach().cpu().to(torch.float32).reshape(12)
    R, t = p[:9].view(3, 3), p[9:]
    xw = torch.stack([_fma32(x[:, 2], R[j, 2], _fma32(x[:, 1], R[j, 1], x[:, 0] * R[j, 0])) + t[j] for j in range(3)], 1)
    return xw, x


def track_keep32(gt, trunc):
    """(N,) bool: the truncation filter as the kernels make it, |gt| < trunc in fp32 (trunc None: every row)."""
    gt = torch.as_tensor(gt).detach().cpu().to(torch.float32).reshape(-1)
    if trunc is None:
        return torch.ones_like(gt, dtype=torch.bool)
    return gt.abs() < torch.tensor(float(trunc), dtype=torch.float32)


def track_counts(xw, gt, ok, frame_ids, kf, trunc, bound):
    """The four counters of lm_transform_kernel, every compare in fp32: (rows kept by the truncation filter, kept rows
    inside the bound -- faces included --, kept rows with another frame id, kept rows that are not valid).  xw (N,3)
    fp32 mapped samples, gt (N,) sanitised targets, ok (N,) bool or None, frame_ids (N,) or None, bound (3,2)."""
    xw = torch.as_tensor(xw).detach().cpu().to(torch.float32)
    b = torch.as_tensor(bound, dtype=torch.float32)
    keep = track_keep32(gt, trunc)
    inb = ((xw >= b[:, 0]) & (xw <= b[:, 1])).all(1)
    n = lambda m: int((keep & m).sum())
    wrong = torch.zeros_like(keep) if frame_ids is None else torch.as_tensor(frame_ids).detach().cpu().reshape(-1) != kf
    bad = torch.zeros_like(keep) if ok is None else ~torch.as_tensor(ok).detach().cpu().reshape(-1).bool()
    return int(keep.sum()), n(inb), n(wrong), n(bad)


def _kernel_fan_in(terms, rows, dtype):
    """Sum (n,K) per-row terms over the boolean ``rows``: fp64 directly, or -- dtype fp32 -- as the reduction kernels
    of lm.hip do: row i belongs to workgroup (i // 256) % 128, a workgroup's share is summed in fp64 from fp32 terms
    and rounded to fp32, and the at most 128 shares are added in fp32 one after the other (the atomics)."""
    terms = terms.reshape(terms.shape[0], -1)
    if dtype == torch.float64:
        return terms[rows].double().sum(0)
    idx = torch.nonzero(rows).flatten()
    blk = (idx // 256) % 128
    part = torch.zeros(128, terms.shape[1], dtype=torch.float64).index_add_(0, blk, terms[idx].double()).float()
    acc = torch.zeros(terms.shape[1], dtype=torch.float32)
    for b in range(min(128, (terms.shape[0] + 255) // 256)):
        acc = acc + part[b]
    return acc.double()


def lm_sums64(x, pose12, grad, sdf, gt, keep, loss_type="L2", gm_scale=0.1, dtype=torch.float64):
    """The 29 sums of lm_normal_eq_kernel over the rows of ``keep``: the upper triangle of H = J^T W J row-major
    [0,21), g = J^T W r [21,27), sum w r^2 [27], the row count [28]; J_i = [((R x_i) x grad_i)^T R, grad_i^T],
    r = sdf - gt, w = 1 (L2) or c / (c + r^2)^2 (GM).  Inputs are the kernel's own fp32 values (sanitised x, its pose,
    its field gradient and SDF); everything from there on is ``dtype`` (fp64: the oracle; fp32: a careful fp32
    evaluation, reduced as the kernel reduces).  Returns (sums (29,), A (29,)) fp64: A is the same sum with every
    factor of every row in absolute value (|R| |x|, the cross product's six products, |c|^T |R|, |grad|, |r|) --
    what the rounding of one row is relative to.  A[28] = 0: the count is exact."""
    f = lambda t: torch.as_tensor(t).detach().cpu().to(torch.float32).to(dtype)
    x, g, sdf, gt = f(x).reshape(-1, 3), f(grad).reshape(-1, 3), f(sdf).reshape(-1), f(gt).reshape(-1)
    R = f(pose12).reshape(-1)[:9].view(3, 3)
    keep = torch.as_tensor(keep).detach().cpu().reshape(-1).bool()

    def jac(x, g, R, cross):
        y = x @ R.T
        return torch.cat((cross(y, g) @ R, g), dim=1)

    J = jac(x, g, R, lambda y, g: torch.stack([y[:, 1] * g[:, 2] - y[:, 2] * g[:, 1], y[:, 2] * g[:, 0] - y[:, 0] * g[:, 2],
                                                y[:, 0] * g[:, 1] - y[:, 1] * g[:, 0]], 1))
    Ja = jac(x.abs(), g.abs(), R.abs(),
             lambda y, g: torch.stack([y[:, 1] * g[:, 2] + y[:, 2] * g[:, 1], y[:, 2] * g[:, 0] + y[:, 0] * g[:, 2],
                                       y[:, 0] * g[:, 1] + y[:, 1] * g[:, 0]], 1))
    r = sdf - gt
    if loss_type == "L2":
        w = torch.ones_like(r)
    elif loss_type == "GM":
        d = gm_scale + r * r
        w = gm_scale / (d * d)
    else:
        raise ValueError(loss_type)
    iu = torch.triu_indices(6, 6)
    wJ, wJa = w[:, None] * J, w[:, None] * Ja

    def rows(wJ, J, r):
        return torch.cat((wJ[:, iu[0]] * J[:, iu[1]], wJ * r[:, None], (w * r * r)[:, None], torch.ones_like(r)[:, None]), 1)

    sums = _kernel_fan_in(rows(wJ, J, r), keep, dtype)
    A = _kernel_fan_in(rows(wJa, Ja, r.abs()).double(), keep, torch.float64)
    A[28] = 0.0
    return sums, A


def lm_unpack(sums):
    """(H (6,6), g (6,)) from the 29 sums: the triangle row-major, mirrored."""
    sums = _t64(sums).reshape(-1)
    iu = torch.triu_indices(6, 6)
    H = torch.zeros(6, 6, dtype=torch.float64)
    H[iu[0], iu[1]] = sums[:21]
    return H + H.triu(1).T, sums[21:27].clone()


def lm_solve64(sums, lam):
    """lm_solve_kernel in fp64: delta = -(H + lam I)^-1 g from given sums, and the infinity-norm condition number of
    H + lam I.  Returns (delta (6,), cond_inf)."""
    H, g = lm_unpack(sums)
    H = H + float(lam) * torch.eye(6, dtype=torch.float64)
    delta = torch.linalg.solve(H, -g)
    cond = torch.linalg.matrix_norm(H, float("inf")) * torch.linalg.matrix_norm(torch.linalg.inv(H), float("inf"))
    return delta, float(cond)


def track_loss64(sdf, gt, ok, n, loss_type, weight, gm_scale=0.1):
    """track_loss_kernel in fp64 (MisoLossTracking, grid_opt/loss.py:517-586): r = sdf - gt on the rows of ``ok``
    (valid and inside the truncation), 0 elsewhere; loss = weight * mean over ALL n rows of r^2 | |r| | w r^2 with the
    Geman-McClure weight w = c / (c + r^2)^2 held constant; gpred = d loss / d sdf per row, exactly 0 off ``ok`` and,
    for L1, at r = 0.  Returns (loss, gpred (n,))."""
    sdf, gt = _t64(sdf).reshape(-1), _t64(gt).reshape(-1)
    ok = torch.as_tensor(ok).detach().cpu().reshape(-1).bool()
    r = torch.where(ok, sdf - gt, torch.zeros_like(sdf))
    if loss_type == "L2":
        term, d = r * r, 2 * r
    elif loss_type == "L1":
        term, d = r.abs(), torch.sign(r)
    elif loss_type == "GM":
        w = gm_scale / (gm_scale + r * r) ** 2
        term, d = w * r * r, 2 * w * r
    else:
        raise ValueError(loss_type)
    return float(weight) * term.sum() / n, torch.where(ok, float(weight) * d / n, torch.zeros_like(d))


def track_pose_sums64(gx, x, dtype=torch.float64):
    """track_reduce_kernel: sums[3a+b] = sum_i gx_ia x_ib (d loss / d R for y = R x + t), sums[9+a] = sum_i gx_ia
    (d loss / d t), over all rows, and A, the same with |gx| and |x|.  dtype as in lm_sums64."""
    f = lambda t: torch.as_tensor(t).detach().cpu().to(torch.float32).to(dtype)
    gx, x = f(gx).reshape(-1, 3), f(x).reshape(-1, 3)
    every = torch.ones(gx.shape[0], dtype=torch.bool)
    rows = lambda g, x: torch.cat(((g[:, :, None] * x[:, None, :]).reshape(-1, 9), g), 1)
    return _kernel_fan_in(rows(gx, x), every, dtype), _kernel_fan_in(rows(gx.abs(), x.abs()).double(), every, torch.float64)


def track_pull_back64(R_base, dr, sums):
    """track_adam_kernel's chain rule in fp64: for R = R_base Exp(dr), t = t_base + dt and sums = (d loss / d R (9),
    d loss / d t (3)), G = R_base^T gR pulled through so3_exp_map's backward gives d loss / d dr; d loss / d dt = gt.
    Returns (g6 (6,), the same map with every entry of every factor in absolute value: the yardstick of g6)."""
    s = _t64(sums).reshape(-1)
    Rb = _t64(R_base).reshape(3, 3)
    gR = s[:9].view(3, 3)
    J = so3_exp_jacobian64(torch.as_tensor(dr).detach().cpu().to(torch.float32))
    g6 = torch.cat([torch.einsum("ijk,ij->k", J, Rb.T @ gR), s[9:12]])
    a6 = torch.cat([torch.einsum("ijk,ij->k", J.abs(), Rb.T.abs() @ gR.abs()), s[9:12].abs()])
    return g6, a6


def adam6_64(param, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8):
    """Step number ``t`` (1-based) of torch.optim.Adam (no amsgrad, no weight decay) in fp64 -> (param, m, v)."""
    param, g, m, v = _t64(param).reshape(-1), _t64(g).reshape(-1), _t64(m).reshape(-1), _t64(v).reshape(-1)
    b1, b2 = betas
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** int(t), 1 - b2 ** int(t)
    return param - lr / bc1 * m / (v.sqrt() / math.sqrt(bc2) + eps), m, v


# --------------------------------------------------------------------------- #
# The fused atlas query and its backward (atlas_eval.hpp, atlas.hip, atlas_bwd.hip)
# --------------------------------------------------------------------------- #
def atlas_to_submap32(x32, poses12, bounds=None):
    """The atlas kernels' frame change in fp32, operation for operation (atlas_eval.hpp, the loop of atlas_eval and
    atlas_to_submap): per submap s and axis j, with p = poses12[s] = {R_submap_world row-major, t_submap_world},
    v = x p[3j]; v = fma(y, p[3j+1], v); v = fma(z, p[3j+2], v); xl_j = v + p[9+j].
    The source writes __fmul_rn / __fmaf_rn / __fadd_rn; the gfx950 code (hipcc -O3 -S) of atlas_sdf_kernel and of
    atlas_trace_kernel is, per submap, three v_mul_f32, six v_fmac_f32 (y's three, then z's three) and three v_add_f32
    in every instantiation; atlas_sdf_bwd_kernel, in atlas_mean and again in its per-submap loop, forms row 0 with
    v_mul_f32 / two v_fmac_f32 / v_add_f32 and rows 1 and 2 as a pair with v_pk_mul_f32, two v_pk_fma_f32 and
    v_pk_add_f32 -- per component the same four operations in the same order.  Nothing is contracted with the
    translation or reassociated, and the bound test is six ordered compares (v_cmp_ge_f32 / v_cmp_le_f32), so a NaN
    coordinate is outside.
    x32 (N,3), poses12 (S,12) fp32 -> xl (S,N,3) fp32 and, with ``bounds`` (per submap (3,2) rows [min, max]), the
    inclusive in-bound mask (N,S): min <= xl <= max on every axis in fp32 (coords_in_bound).  A NaN or inf world
    coordinate gives a NaN or inf xl on every axis it reaches (inf x 0 = NaN) and is inside nothing.  A membership that
    differs from the kernel's on one row: look at that row for the double rounding of _fma32 first."""
    x = torch.as_tensor(x32, dtype=torch.float32).reshape(-1, 3)
    p = torch.as_tensor(poses12, dtype=torch.float32).reshape(-1, 12)
    xl = torch.empty(p.shape[0], x.shape[0], 3, dtype=torch.float32)
    for s in range(p.shape[0]):
        for j in range(3):
            v = x[:, 0] * p[s, 3 * j]
            v = _fma32(x[:, 1], p[s, 3 * j + 1], v)
            v = _fma32(x[:, 2], p[s, 3 * j + 2], v)
            xl[s, :, j] = v + p[s, 9 + j]
    if bounds is None:
        return xl
    b = torch.as_tensor(bounds, dtype=torch.float32).reshape(-1, 3, 2)
    inside = ((xl >= b[:, None, :, 0]) & (xl <= b[:, None, :, 1])).all(2)
    return xl, inside.t().contiguous()


def _trilinear_scatter64(shape, ix, g):
    """The transpose of _trilinear_jet_select's value: rows g (N,C) fp64 at index coordinates ix (N,3) added into a
    dense (1,C,D,H,W) fp64 gradient, vertex k of a row's cell receiving g w_k, out-of-range corners and rows with a
    non-finite ix nothing.  -> (gradient, the same sum over |g| w_k)."""
    _, c, d, h, w = shape
    ix = ix.double()
    bad = ~torch.isfinite(ix).all(1)
    ix = torch.where(bad[:, None], torch.full_like(ix, -4.0), ix)
    i0 = torch.floor(ix)
    fr = ix - i0
    i0 = i0.clamp(-2, max(w, h, d) + 1).long()
    out, mag = (torch.zeros(d * h * w, c, dtype=torch.float64) for _ in range(2))
    for k in range(8):
        o = (k & 1, (k >> 1) & 1, k >> 2)
        xi, yi, zi = i0[:, 0] + o[0], i0[:, 1] + o[1], i0[:, 2] + o[2]
        inb = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (zi >= 0) & (zi < d)
        lin = ((zi.clamp(0, d - 1) * h + yi.clamp(0, h - 1)) * w + xi.clamp(0, w - 1))
        wt = [fr[:, a] if o[a] else 1 - fr[:, a] for a in range(3)]
        term = torch.where(inb[:, None], g * (wt[0] * wt[1] * wt[2])[:, None], torch.zeros((), dtype=torch.float64))
        out.index_add_(0, lin, term)
        mag.index_add_(0, lin, term.abs())
    back = lambda t: t.t().reshape(1, c, d, h, w)
    return back(out), back(mag)


class Atlas64(NamedTuple):
    """atlas64's answer.  Every ``*_y`` is the absolute-value yardstick of the field before it: the same sums with |.| of
    every term."""
    xl: torch.Tensor            # (S,N,3) fp32: atlas_to_submap32
    inside: torch.Tensor        # (N,S) bool
    count: torch.Tensor         # (N,) int64
    feat: torch.Tensor          # (N,F) the mean feature row
    feat_y: torch.Tensor        # (N,F) sum_s value_w_s / max(count, 1)
    sdf: torch.Tensor           # (N,) the decoder on the mean
    sdf_y: torch.Tensor
    sdf_zero: torch.Tensor      # () the decoder on the zero row
    tie: torch.Tensor           # (N,) bool: a pre-activation of either layer within ``tie`` of zero
    gsdf: torch.Tensor          # (N,) the cotangent used (zero on the tie rows under zero_ties)
    dfeat: torch.Tensor         # (N,F) d mean / max(count, 1): the row every inside submap's levels receive
    dxl: torch.Tensor           # (S,N,3) d sdf-sum / d x_local per submap (zero where not inside)
    dxl_y: torch.Tensor
    gx: torch.Tensor            # (N,3) sum_s R_s^T dxl_s
    gx_y: torch.Tensor
    gposes: torch.Tensor        # (S,12) [sum_n dxl (x) x_world, sum_n dxl]
    gposes_y: torch.Tensor
    grids: list                 # per submap, per level: dense (1,C,Z,Y,X) fp64 (zeros: ignored level; None: locked)
    grids_y: list


def atlas64(features, bounds, poses12, x32, weights, biases, gsdf, ignore=None, locked=(), inside=None, tie=1e-6,
            zero_ties=False):
    """The fused atlas query (atlas.hip) and its backward (atlas_bwd.hip) in fp64.  Membership and the local coordinates
    are the fp32 restatement's (atlas_to_submap32); everything after is fp64 at the kernel's own fp32 index coordinates
    (sample_index32, _trilinear_jet_select): the masked mean over the submaps a row is inside (count 0 -> divisor 1),
    a three-linear ReLU decoder on it, and for the cotangent gsdf (N,) of the SDF: d feats_s = d mean / count for every
    submap the row is inside (the mask and the count are constants), d x_local per submap by the sampler's first
    derivative, gx = sum_s R_s^T dxl_s, gposes[s] = [sum_n dxl (x) x_world, sum_n dxl] over the rows inside s, and the
    dense level gradients.  features: per submap the levels (1,C,Z,Y,X); bounds: per submap (3,2); poses12 (S,12);
    ignore: per submap None or one bool per level (zero columns, nothing in dxl, a zero gradient); locked: the submaps
    without level gradients (None); inside: a membership (N,S) to use INSTEAD of the restatement's (planted faults);
    zero_ties: rows with a pre-activation of either layer within ``tie`` of zero carry a zero cotangent (the ReLU's
    derivative is the kernel's to choose there: the rule of tests/test_split_precision.py).
    Rows with a non-finite world coordinate are inside nothing: a zero feature row, the zero-row SDF, exactly zero
    gradients, and no term in any sum.  Yardsticks: Atlas64."""
    f64 = torch.float64
    x32 = torch.as_tensor(x32, dtype=torch.float32).reshape(-1, 3)
    poses12 = torch.as_tensor(poses12, dtype=torch.float32).reshape(-1, 12)
    S, n = poses12.shape[0], x32.shape[0]
    xl, member = atlas_to_submap32(x32, poses12, bounds)
    if inside is not None:
        member = inside
    member = member & torch.isfinite(x32).all(1)[:, None]
    count = member.sum(1)
    den = count.clamp(min=1).to(f64)[:, None]
    F_ = sum(int(f.shape[1]) for f in features[0])
    nan = torch.tensor(float("nan"), dtype=f64)
    jets = []                                   # per submap, per level: None or (c0, C, ix, mult, der, yd)
    total, total_y = torch.zeros(n, F_, dtype=f64), torch.zeros(n, F_, dtype=f64)
    for s in range(S):
        row, c0 = [], 0
        for l, f in enumerate(features[s]):
            c = int(f.shape[1])
            if ignore is not None and ignore[s] is not None and ignore[s][l]:
                row.append(None)
            else:
                ix, mult = sample_index32(xl[s], bounds[s], (f.shape[4], f.shape[3], f.shape[2]))
                ix = torch.where(member[:, s, None], ix, nan)
                val, der, yw, _, yd = _trilinear_jet_select(f, ix)
                total[:, c0:c0 + c] += val
                total_y[:, c0:c0 + c] += yw
                row.append((c0, c, ix, mult, der, yd))
            c0 += c
        jets.append(row)
    feat, feat_y = total / den, total_y / den
    W = [w.detach().to(f64) for w in weights]
    B = [torch.zeros(w.shape[0], dtype=f64) if b is None else b.detach().to(f64) for w, b in zip(W, biases)]
    assert len(W) == 3, "the fused decoders have one hidden layer pair: three linears"
    pre1 = feat @ W[0].t() + B[0]
    pre2 = torch.relu(pre1) @ W[1].t() + B[1]
    sdf = (torch.relu(pre2) @ W[2].t() + B[2])[:, 0]
    y1 = feat_y @ W[0].abs().t() + B[0].abs()
    y2 = y1 @ W[1].abs().t() + B[1].abs()
    sdf_y = (y2 @ W[2].abs().t() + B[2].abs())[:, 0]
    sdf_zero = (torch.relu(torch.relu(B[0]) @ W[1].t() + B[1]) @ W[2].t() + B[2])[0]
    sdf = torch.where(count == 0, sdf_zero, sdf)      # (one value for the zero row, whatever the batch it is summed in)
    near = torch.minimum(pre1.abs().min(1).values, pre2.abs().min(1).values) < tie
    # backward
    g = torch.as_tensor(gsdf).detach().reshape(-1).to(f64)
    if zero_ties:
        g = torch.where(near, torch.zeros_like(g), g)
    on1, on2 = (pre1 > 0).to(f64), (pre2 > 0).to(f64)
    dmean = ((((g[:, None] * W[2]) * on2) @ W[1]) * on1) @ W[0]
    dmean_y = ((((g.abs()[:, None] * W[2].abs()) * on2) @ W[1].abs()) * on1) @ W[0].abs()
    dfe, dfe_y = dmean / den, dmean_y / den
    dxl, dxl_y = torch.zeros(S, n, 3, dtype=f64), torch.zeros(S, n, 3, dtype=f64)
    grids, grids_y = [], []
    for s in range(S):
        gs, gys = [], []
        for l, f in enumerate(features[s]):
            j = jets[s][l]
            if j is None:
                gs.append(None if s in locked else torch.zeros(f.shape, dtype=f64))
                gys.append(None if s in locked else torch.zeros(f.shape, dtype=f64))
                continue
            c0, c, ix, mult, der, yd = j
            dxl[s] += mult * (dfe[:, c0:c0 + c, None] * der).sum(1)
            dxl_y[s] += mult.abs() * (dfe_y[:, c0:c0 + c, None] * yd).sum(1)
            if s in locked:
                gs.append(None), gys.append(None)
            else:
                a, b = _trilinear_scatter64(f.shape, ix, dfe[:, c0:c0 + c])
                gs.append(a), gys.append(_trilinear_scatter64(f.shape, ix, dfe_y[:, c0:c0 + c])[0])
        grids.append(gs), grids_y.append(gys)
    Rm = poses12[:, :9].to(f64).view(S, 3, 3)                        # x_local = R x_world + t
    gx = torch.einsum("sjk,snj->nk", Rm, dxl)
    gx_y = torch.einsum("sjk,snj->nk", Rm.abs(), dxl_y)
    xw = torch.where(torch.isfinite(x32), x32, torch.zeros_like(x32)).to(f64)      # (rows inside nothing add no term)
    gposes = torch.cat((torch.einsum("snj,nk->sjk", dxl, xw).reshape(S, 9), dxl.sum(1)), 1)
    gposes_y = torch.cat((torch.einsum("snj,nk->sjk", dxl_y, xw.abs()).reshape(S, 9), dxl_y.sum(1)), 1)
    return Atlas64(xl, member, count, feat, feat_y, sdf, sdf_y, sdf_zero, near, g, dfe, dxl, dxl_y, gx, gx_y, gposes, gposes_y,
                   grids, grids_y)
