"""Seed-pinned inputs of the atlas-gradient / Fuser.fuse goldens (tests/golden/atlas_grad.npz), shared by the tool that
writes them from the reference (tools/make_fusion_goldens.py) and the tests that read them (test_atlas_grad_oracle.py,
test_atlas_grad.py).  The atlas, its world points and its SDF batch are those of golden_cases (ATLAS)."""
import numpy as np

import golden_cases as gc

SEED = gc.ATLAS["seed"] + 900

# (b) MisoLossFusion.compute settings: tag -> (loss_type, weight_fs); weight_eik = 0 throughout
LOSS_SETTINGS = {"L1": ("L1", 0.0), "L2": ("L2", 0.0), "L1_fs": ("L1", 0.3), "L2_fs": ("L2", 0.3)}
TRUNC_DIST = 0.15

# (c) Fuser.fuse trajectories: tag -> the cfg['mapping'] block; 4 iterations, the three learning rates below
FUSE_ITERS = 4
FUSE_LRS = dict(feat_lr=1e-3, submap_pose_lr=1e-4, kf_pose_lr=1e-4)
FUSE_MAPPING = {
    "plain": dict(weight_sdf=1.0, weight_eik=0.0, weight_fs=0.3, loss_type="L1", trunc_dist=TRUNC_DIST,
                  finite_diff_eps=1e-2, grad_method="finitediff", eik_trunc_dist=0.1, gm_scale_sdf=1.0),
    "eik_fd": dict(weight_sdf=1.0, weight_eik=0.2, weight_fs=0.3, loss_type="L1", trunc_dist=TRUNC_DIST,
                   finite_diff_eps=1e-2, grad_method="finitediff", eik_trunc_dist=0.1, gm_scale_sdf=1.0),
    "eik_ag": dict(weight_sdf=1.0, weight_eik=0.2, weight_fs=0.3, loss_type="L1", trunc_dist=TRUNC_DIST,
                   finite_diff_eps=1e-2, grad_method="autograd", eik_trunc_dist=0.1, gm_scale_sdf=1.0),
}
# trajectories whose eikonal term differentiates d sdf / d x again (a double backward through the atlas: Fuser.fuse leaves
# fused_backward off); the reference runs them on a model built with second_order_grid_sample
FUSE_DOUBLE_BACKWARD = ("eik_ag",)
# The bars the tests hold a trajectory to (test_grid_opt_mirror.py): trained parameters 3e-6 absolute, loss values 3e-5
# relative.  With an eikonal term the reference does not meet them against ITSELF: an Adam step is a gradient entry over
# its own running magnitude, so where an entry is the difference of nearly cancelling terms (the finite-difference
# quotient divides the fp32 rounding of the SDF by 2 eps) rounding decides the step.  The reference's fp32 run is up to
# 2e-3 (features), 1.8e-5 (a keyframe translation) and 5.3e-5 relative (the loss of 'eik_ag', iteration 3) away from its
# own fp64 run.  So the golden marks what the two runs settle, and only that is compared.  The cutoff is a thirtieth of the
# bar, not the bar: the one fp32 run at hand is a single draw of an entry's rounding noise.  If that noise has standard
# deviation sigma, another fp32 implementation is about sqrt(2) sigma from the reference; an entry with sigma = bar passes
# a cutoff of bar / 3 in a quarter of all cases and then misses the bar in half of them, and a few hundred such entries
# exist -- passing bar / 30 it does in 3 % of the cases.  (Seen on the CPU backend, which has the reference's own operation
# order: at a cutoff of 1e-6 an entry that was kept came out 4.4e-6 off.)  The tests assert that most of every array is kept
# (FUSE_MIN_KEPT); the sum of absolute changes over ALL entries, settled or not, is kept for 'plain' only.
FUSE_BAR, FUSE_LOSS_BAR = 3e-6, 3e-5
FUSE_SETTLED, FUSE_LOSS_SETTLED = FUSE_BAR / 30, FUSE_LOSS_BAR / 30
FUSE_MIN_KEPT = dict(poses=1 / 3, features=0.85, loss=0.5)      # share of a pose array / of SAMPLES / of the iterations
FUSE_MOVED_CHECK = ("plain",)
SAMPLES = 1024      # entries kept per tensor where a golden holds a sample of a large array


def cotangent():
    """w of golden (a): the gradients are those of sum(w * atlas(x)) at gc.atlas_world_points()"""
    return np.random.RandomState(SEED).standard_normal((gc.ATLAS["n_points"], 1)).astype(np.float32)


def fusion_batch():
    """gc.atlas_sdf_batch() with free-space signs on about a third of the rows (its own are all zero, which would leave
    the free-space term empty)."""
    mi, gt = gc.atlas_sdf_batch()
    rs = np.random.RandomState(SEED + 1)
    gt = dict(gt)
    gt["sdf_signs"] = (rs.uniform(0, 1, gt["sdf"].shape) < 0.35).astype(np.float32)
    return mi, gt


def fuse_cfg(tag, device, log_dir):
    return {"device": device, "mapping": dict(FUSE_MAPPING[tag]),
            "train": {"verbose": False, "optimizer": "adam", "learning_rate": 1e-3, "epochs": 1, "ckpt_every": -1,
                      "eval_every": -1, "eval_metric": None, "pretrained_model": None, "log_dir": log_dir}}


def sample_of(flat_ref, k=SAMPLES, seed=SEED + 2):
    """indices of up to k entries of a flat array, drawn among its non-zeros (sorted, int64)"""
    nz = np.flatnonzero(flat_ref)
    if nz.size > k:
        nz = np.sort(np.random.RandomState(seed).choice(nz, size=k, replace=False))
    return nz.astype(np.int64)
