"""Generate tests/golden/atlas_grad.npz by IMPORTING the reference (MISO) on CPU: the gradients of its GridAtlas, of
MisoLossFusion on an atlas, and the trajectory of Fuser.fuse's optimisation.

Runs only in the build container (needs the reference checkout, see tools/make_goldens.py, whose import recipe and
atlas builders are reused).  fp32, CPU, seed-pinned inputs from tests/golden_cases.py and tests/fusion_cases.py.

(a) ``a_*``: at gc.atlas_world_points() with the cotangent fusion_cases.cotangent(), the gradients of sum(w * atlas(x))
    with respect to x, every rotation / translation correction and every submap's level features (the features'
    non-zeros: flat index + value).
(b) ``b_<setting>_*``: MisoLossFusion.compute on fusion_cases.fusion_batch() for the settings of
    fusion_cases.LOSS_SETTINGS: the loss dict, and after backward() the gradients of the submap pose corrections, the
    keyframe pose corrections and the features (a sample of the non-zeros of each level + its sum of absolute values).
(c) ``c_<tag>_*``: Fuser.fuse.  The reference's own ``fuse`` raises before its first step (it hands MisoLossFusion the
    keyword ``gm_scale_sdf``, fuser.py:102), so its body is followed here statement by statement without that keyword:
    unlock everything, the three parameter groups, MisoLossFusion from cfg['mapping'], the reference Trainer on CPU (it
    takes the device as an argument; tensorboard's writer is stubbed as in make_goldens.gen_trainer) with an external
    Adam, FUSE_ITERS epochs.  Recorded: the total loss of every iteration (sum of the means of the loss dict, as
    Trainer.train_epoch forms it), the final pose corrections, and of the final features a sample of the entries that
    moved (drawn among those the reference's own fp32 and fp64 runs agree on: see gen_c) and, for the trajectories of
    fusion_cases.FUSE_MOVED_CHECK, the sum of absolute changes per level.

    python tools/make_fusion_goldens.py
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _features(atlas, gc):
    return [[atlas.get_submap(s).features[l].feature for l in range(gc.ATLAS["n_levels"])]
            for s in range(gc.ATLAS["n_submaps"])]


def _unlock_all(atlas):
    for s in range(atlas.num_submaps):
        atlas.unlock_submap(s)
    atlas.unlock_submap_pose()


def gen_a(GridAtlas, gc, fc, out):
    atlas = mg.build_atlas_two_kf(GridAtlas, gc)
    _unlock_all(atlas)
    x = mg.T(gc.atlas_world_points()).requires_grad_(True)
    w = mg.T(fc.cotangent())
    (w * atlas(x)).sum().backward()
    out["a_gx"] = x.grad.numpy().copy()
    out["a_gdr"] = np.stack([p.grad.numpy().copy() for p in atlas.rotation_corrections])
    out["a_gdt"] = np.stack([p.grad.numpy().copy() for p in atlas.translation_corrections])
    for s, fs in enumerate(_features(atlas, gc)):
        for l, f in enumerate(fs):
            g = f.grad.numpy().reshape(-1)
            idx = np.flatnonzero(g)
            out[f"a_gfeat_s{s}_l{l}_idx"] = idx.astype(np.int32)
            out[f"a_gfeat_s{s}_l{l}_val"] = g[idx].copy()


def _kf_pose_grads(atlas):
    return (np.stack([sm.rotation_corrections.grad.numpy().copy() for sm in atlas.submaps]),
            np.stack([sm.translation_corrections.grad.numpy().copy() for sm in atlas.submaps]))


def gen_b(GridAtlas, rloss, gc, fc, out):
    mi, gt = fc.fusion_batch()
    mi_t = {k: mg.T(v) for k, v in mi.items()}
    gt_t = {k: mg.T(v) for k, v in gt.items()}
    out["fs_signs"] = gt["sdf_signs"]
    for tag, (loss_type, w_fs) in fc.LOSS_SETTINGS.items():
        atlas = mg.build_atlas_two_kf(GridAtlas, gc)
        _unlock_all(atlas)
        lf = rloss.MisoLossFusion(loss_type=loss_type, weight_sdf=1.0, weight_eik=0.0, weight_fs=w_fs,
                                  trunc_dist=fc.TRUNC_DIST)
        d = lf.compute(atlas, mi_t, gt_t)
        out[f"b_{tag}_keys"] = np.asarray(sorted(d))
        for k, v in d.items():
            out[f"b_{tag}_loss_{k}"] = np.float64(v.item())
        sum(v.mean() for v in d.values()).backward()
        out[f"b_{tag}_gdr"] = np.stack([p.grad.numpy().copy() for p in atlas.rotation_corrections])
        out[f"b_{tag}_gdt"] = np.stack([p.grad.numpy().copy() for p in atlas.translation_corrections])
        out[f"b_{tag}_gkf_dr"], out[f"b_{tag}_gkf_dt"] = _kf_pose_grads(atlas)
        for s, fs in enumerate(_features(atlas, gc)):
            for l, f in enumerate(fs):
                g = f.grad.numpy().reshape(-1)
                idx = fc.sample_of(g)
                out[f"b_{tag}_gfeat_s{s}_l{l}_idx"] = idx.astype(np.int32)
                out[f"b_{tag}_gfeat_s{s}_l{l}_val"] = g[idx].copy()
                out[f"b_{tag}_gfeat_s{s}_l{l}_abssum"] = np.float64(np.abs(g.astype(np.float64)).sum())


class _Batch(torch.utils.data.Dataset):
    """mg._OneBatch with the floating-point rows in ``dtype``"""

    def __init__(self, mi, g, dtype):
        cast = lambda v: mg.T(v[0]).to(dtype) if v.dtype == np.float32 else mg.T(v[0])      # noqa: E731
        self.item = ({k: cast(v) for k, v in mi.items()}, {k: cast(v) for k, v in g.items()})

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.item


def _second_order_sampling():
    """The reference's sampling op for second_order_grid_sample models is its CUDA extension cuda_gridsample, which can
    be neither built nor run here; as in make_goldens.gen_second_order a module of that name backed by the oracle's
    any-order restatement (oracle.ref_torch.trilinear_gather) stands in for it."""
    import types
    if mg.ROOT not in sys.path:
        sys.path.insert(0, mg.ROOT)
    from oracle import ref_torch as R
    shim = types.ModuleType("cuda_gridsample")

    def grid_sample_3d(input, grid, padding_mode="zeros", align_corners=True):
        _, do, ho, wo, _ = grid.shape
        out = R.trilinear_gather(input, grid.reshape(-1, 3), align_corners, padding_mode)
        return out.transpose(0, 1).reshape(1, input.shape[1], do, ho, wo)

    shim.grid_sample_3d = grid_sample_3d
    shim.grid_sample_2d = None
    sys.modules["cuda_gridsample"] = shim


def _fuse_trajectory(GridAtlas, rloss, rtrainer, gc, fc, tag, dtype):
    """-> (per-iteration totals, the atlas after FUSE_ITERS iterations); dtype float64: the same run in double"""
    mi, gt = fc.fusion_batch()
    if tag in fc.FUSE_DOUBLE_BACKWARD:
        _second_order_sampling()
        plain_cfg = gc.model_cfg
        gc.model_cfg = lambda *a, **k: plain_cfg(*a, second_order=True, **k)
        try:
            atlas = mg.build_atlas_two_kf(GridAtlas, gc)
        finally:
            gc.model_cfg = plain_cfg
    else:
        atlas = mg.build_atlas_two_kf(GridAtlas, gc)
    if dtype == torch.float64:
        atlas = atlas.double()
        atlas.R_world_submap_list = [r.double() for r in atlas.R_world_submap_list]
        atlas.t_world_submap_list = [t.double() for t in atlas.t_world_submap_list]
        for sm in atlas.submaps:
            sm.bound = sm.bound.double()
            for g in sm.features:
                g.bound = g.bound.double()
    loader = torch.utils.data.DataLoader(_Batch(mi, gt, dtype), batch_size=1, shuffle=True, num_workers=0)
    with tempfile.TemporaryDirectory() as log_dir:
        cfg = fc.fuse_cfg(tag, "cpu", log_dir)
        # ---- reference fuser.py:64-118, minus dataset.unselect_keyframes() (the one-batch dataset has no selection)
        # and the gm_scale_sdf keyword
        _unlock_all(atlas)
        lrs = fc.FUSE_LRS
        param_groups = [{'params': atlas.params_for_all_features(), 'lr': lrs["feat_lr"]},
                        {'params': atlas.params_for_all_submap_poses(), 'lr': lrs["submap_pose_lr"]},
                        {'params': atlas.params_for_all_kf_poses(), 'lr': lrs["kf_pose_lr"]}]
        cfg_map, cfg_train = cfg['mapping'], cfg['train']
        cfg_train['epochs'] = fc.FUSE_ITERS
        lf = rloss.MisoLossFusion(
            weight_sdf=cfg_map['weight_sdf'], weight_eik=cfg_map['weight_eik'], weight_fs=cfg_map['weight_fs'],
            loss_type=cfg_map['loss_type'], trunc_dist=cfg_map['trunc_dist'],
            finite_diff_eps=cfg_map['finite_diff_eps'], grad_method=cfg_map['grad_method'],
            eik_trunc_dist=cfg_map['eik_trunc_dist'], use_stability=False)
        lf.use_clip = False      # harness patch: compute reads this attribute with weight_eik > 0, nothing defines it (loss.py:788)
        totals = []
        inner = lf.compute

        def compute(model, model_input, g, _inner=inner, _totals=totals):
            d = _inner(model, model_input, g)
            _totals.append(float(sum(v.mean() for v in d.values()).item()))
            return d

        lf.compute = compute
        trainer = rtrainer.Trainer(cfg_train, atlas, lf, loader, None, "cpu", dtype)
        trainer.set_external_optimizer(torch.optim.Adam(param_groups, lr=1e-3))
        trainer.train()
    assert len(totals) == fc.FUSE_ITERS
    return totals, atlas


def gen_c(GridAtlas, rloss, rtrainer, gc, fc, out):
    class _Writer:  # harness patch: tensorboard is absent from the image
        def __init__(self, *a, **k):
            pass

        def add_scalar(self, *a, **k):
            pass

    rtrainer.SummaryWriter = _Writer
    start = gc.atlas_inputs()
    for tag in fc.FUSE_MAPPING:
        totals, atlas = _fuse_trajectory(GridAtlas, rloss, rtrainer, gc, fc, tag, torch.float32)
        totals64, atlas64 = _fuse_trajectory(GridAtlas, rloss, rtrainer, gc, fc, tag, torch.float64)
        out[f"c_{tag}_loss"] = np.asarray(totals, dtype=np.float64)
        own = np.abs(np.asarray(totals) - np.asarray(totals64)) / np.abs(np.asarray(totals64))
        out[f"c_{tag}_loss_settled"] = own <= fc.FUSE_LOSS_SETTLED
        print(f"[atlas_grad] fuse '{tag}' loss: reference fp32 against its own fp64 run, relative: {own}")
        poses = lambda at: {      # noqa: E731
            "dr": np.stack([p.detach().numpy().copy() for p in at.rotation_corrections]),
            "dt": np.stack([p.detach().numpy().copy() for p in at.translation_corrections]),
            "kf_dr": np.stack([sm.rotation_corrections.detach().numpy().copy() for sm in at.submaps]),
            "kf_dt": np.stack([sm.translation_corrections.detach().numpy().copy() for sm in at.submaps])}
        p32, p64 = poses(atlas), poses(atlas64)
        for name in p32:
            # (the same rule as for the features below: components the reference's fp32 and fp64 runs do not settle are
            # marked and stay out of the comparison)
            own = np.abs(p32[name].astype(np.float64) - p64[name])
            out[f"c_{tag}_{name}"] = p32[name]
            out[f"c_{tag}_{name}_settled"] = own <= fc.FUSE_SETTLED
            print(f"[atlas_grad] fuse '{tag}' {name}: reference fp32 against its own fp64 run: max {own.max():.2e}, "
                  f"{int((own > fc.FUSE_SETTLED).sum())} of {own.size} components apart by more than {fc.FUSE_SETTLED:g}")
        unsettled, worst = 0, 0.0
        for s, (fs, fs64) in enumerate(zip(_features(atlas, gc), _features(atlas64, gc))):
            for l, (f, f64) in enumerate(zip(fs, fs64)):
                after = f.detach().numpy().reshape(-1)
                delta = after - start[s]["features"][l].reshape(-1)
                # An Adam step is the gradient over its own running magnitude: where a gradient entry is the difference of
                # nearly cancelling terms (the finite-difference eikonal term divides fp32 rounding of the SDF by 2 eps),
                # fp32 rounding decides the step.  Such entries are no check of an implementation: the reference itself
                # does not reproduce them.  The sample is drawn among the moved entries that the reference's fp32 and
                # fp64 runs settle to within FUSE_SETTLED (fusion_cases.py).
                own = np.abs(after.astype(np.float64) - f64.detach().numpy().reshape(-1))
                unsettled += int((own > fc.FUSE_SETTLED).sum())
                worst = max(worst, float(own.max()))
                idx = fc.sample_of(np.where(own <= fc.FUSE_SETTLED, delta, 0.0))
                out[f"c_{tag}_feat_s{s}_l{l}_idx"] = idx.astype(np.int32)
                out[f"c_{tag}_feat_s{s}_l{l}_val"] = after[idx].copy()
                if tag in fc.FUSE_MOVED_CHECK:
                    out[f"c_{tag}_feat_s{s}_l{l}_moved"] = np.float64(np.abs(delta.astype(np.float64)).sum())
        print(f"[atlas_grad] fuse '{tag}': reference fp32 against its own fp64 run, final features: max {worst:.2e}, "
              f"{unsettled} entries apart by more than {fc.FUSE_SETTLED:g}")


def main():
    mg.import_reference()
    import golden_cases as gc
    import fusion_cases as fc
    import grid_opt.loss as rloss
    import grid_opt.trainer as rtrainer
    from grid_opt.models.grid_atlas import GridAtlas
    torch.manual_seed(0)
    out = {}
    gen_a(GridAtlas, gc, fc, out)
    gen_b(GridAtlas, rloss, gc, fc, out)
    gen_c(GridAtlas, rloss, rtrainer, gc, fc, out)
    path = gc.golden_path("atlas_grad")
    np.savez_compressed(path, **out)
    print("[atlas_grad]", os.path.getsize(path), "bytes;",
          {k: (float(v) if np.ndim(v) == 0 else v.shape) for k, v in out.items() if k.startswith(("c_", "b_L1_loss"))})


if __name__ == "__main__":
    main()
