"""grid.type 'hash' through the routes a regular GridNet takes fused: every one of them declines (or falls back) instead
of crashing, and the op-by-op route trains.  A small analytic sphere, |x| - 0.5 in [-1, 1]^3; level 0 (8^3 vertices) is
dense-indexed behind 2^10 rows, level 1 (16^3) is hashed four vertices to a row."""
import logging

import numpy as np
import pytest
import torch

import golden_cases as gc
import hash_cases as hc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = [[-1.0, 1.0]] * 3
LOG2 = 10


def _cfg(num_poses=2, optimize_pose=False):
    cfg = gc.model_cfg(BOUND, 0.25, 2.0, 2, 4, 64, num_poses=num_poses, optimize_pose=optimize_pose, init_stddev=0.01)
    cfg["grid"]["type"] = "hash"
    cfg["grid"]["log2_hashmap_size"] = LOG2
    return cfg


def _net(seed=0, **kw):
    from miso_amd.grid_opt.models.grid_net import GridNet
    torch.manual_seed(seed)
    net = GridNet(_cfg(**kw), device=DEV).to(DEV)
    net.set_initial_kf_pose(0, torch.eye(3), torch.zeros(3, 1), kf_key="KF0")
    assert [(g.dims, g.dense_indexed, tuple(g.feature.shape)) for g in net.features] == \
        [((8, 8, 8), True, (512, 4)), ((16, 16, 16), False, (1024, 4))]
    return net


def _sphere_batch(n, seed, half=False):
    """n samples of the sphere's SDF; half: only x < -0.3, so that most of level 0's rows receive no gradient"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 1.9 - 0.95
    if half:
        x[:, 0] = -0.95 + 0.6 * torch.rand(n, generator=g)
    sdf = x.norm(dim=1, keepdim=True) - 0.5
    mi = {"coords_frame": x[None].to(DEV), "sample_frame_ids": torch.zeros(1, n, 1, dtype=torch.int64, device=DEV),
          "weights": torch.ones(1, n, 1, device=DEV)}
    gt = {"sdf": sdf[None].to(DEV), "sdf_valid": torch.ones(1, n, 1, device=DEV),
          "sdf_signs": (sdf > 0.15).float()[None].to(DEV)}
    return x, mi, gt


def _trainer(net, tmp_path, lr=1e-2):
    import miso_amd.grid_opt.loss as L
    from miso_amd.grid_opt.trainer import GridTrainer
    tcfg = {"verbose": False, "optimizer": "adam", "learning_rate": lr, "epochs": 1, "ckpt_every": -1, "eval_every": -1,
            "eval_metric": None, "pretrained_model": None, "log_dir": str(tmp_path), "relchange_tol": 0,
            "max_epochs_in_level": 1000, "grid_training_mode": "joint"}
    lossf = L.MisoLossMapping(loss_type="L1", weight_sdf=1.0, weight_eik=0.0, weight_fs=0.1, trunc_dist=0.15)
    return GridTrainer(tcfg, net, lossf, None, None, DEV, torch.float32)


def test_queries_decline_the_fused_routes(monkeypatch):
    from miso_amd.grid_opt.utils.utils_sdf import extract_fields, sphere_tracing
    net = _net()
    x, _, _ = _sphere_batch(257, 1)
    xd = x.to(DEV)
    assert net._fused_decoder() is None
    with torch.no_grad():
        sdf = net(xd)
        feats, stab = net.query_feature(xd), net.query_stability(xd)
    assert sdf.shape == (257, 1) and feats.shape == (257, 8) and stab.shape == (257, 2)
    assert torch.isfinite(sdf).all() and feats.any() and not stab.any()
    # sdf_and_gradient: the autograd branch.  Its gradient against central differences of forward(), on the points that
    # stay h inside one cell of the finest level on every axis; the field still has the decoder's ReLU kinks, which a
    # few differences straddle, hence the 90th percentile and not the maximum
    from miso_amd import ops
    asked, raw = [], ops.hash_encode_bwd_raw
    monkeypatch.setattr(ops, "hash_encode_bwd_raw", lambda *a: asked.append((a[6], tuple(a[7]))) or raw(*a))
    net.unlock_feature()
    s2, gx = net.sdf_and_gradient(xd)
    assert torch.equal(s2, sdf) and gx.shape == (257, 3) and not gx.requires_grad
    assert asked == [(True, (False, False))]             # x alone: no table gradient is filled and scattered to be dropped
    h = 1e-3
    with torch.no_grad():
        fd = torch.cat([(net(xd + h * e) - net(xd - h * e)) / (2 * h) for e in torch.eye(3, device=DEV)], 1)
    frac = ((xd + 1) * 8 - 0.5) % 1
    inner = ((frac > 0.02) & (frac < 0.98)).all(1) & (xd.abs().max(1).values < 0.9)
    err = (fd - gx)[inner].abs().max(1).values
    assert inner.sum() > 150 and torch.quantile(err, 0.9) <= 0.02 * gx.abs().max() + 1e-5, torch.quantile(err, 0.9)
    # sphere tracing: the fused launch declines, the loop runs
    o = torch.tensor([[0.0, 0.0, -0.9]], device=DEV).repeat(16, 1)
    d = torch.nn.functional.normalize(torch.tensor([[0.0, 0.0, 1.0]], device=DEV) + 0.2 * torch.randn(16, 3, device=DEV), dim=1)
    with torch.no_grad():
        assert net.sphere_trace(o, d) is None
        p, hit = sphere_tracing(net, o, d, max_iters=20, max_dist=3.0)
    assert p.shape == (16, 3) and hit.shape == (16, 1) and torch.isfinite(p).all()
    b = torch.tensor(BOUND)
    u = extract_fields(b[:, 0], b[:, 1], 9, lambda q: net(q), device=DEV)
    assert u.shape == (9, 9, 9) and np.isfinite(u).all()


def test_mapping_trains_through_the_op_by_op_route(tmp_path):
    """One Trainer step with MisoLossMapping (L1 + free space): no captured step, Adam moves the rows that received a
    gradient and leaves every other row as it was; 30 steps later the loss is below the first step's."""
    net = _net()
    net.unlock_feature()
    net.lock_pose()
    tr = _trainer(net, tmp_path)
    from miso_amd.optim import DenseAdam
    assert isinstance(tr.optimizer, DenseAdam)
    x, mi, gt = _sphere_batch(2048, 2, half=True)
    before = [g.feature.detach().clone() for g in net.features]
    stab = [g.feature.detach().clone() for g in net.feature_stability]
    losses = [float(tr.train_step(mi, gt).detach())]
    assert not tr.__dict__.get("_mapping_steps") and tr._fast_plan is None, "the captured step must decline a hash grid"
    from oracle import ref_torch as R
    for l, g in enumerate(net.features):
        rows, inb, _ = hc.corner_terms32(R.sample_index32(x, BOUND, g.dims)[0], g.dims, LOG2)
        hit = torch.zeros(g.rows, dtype=torch.bool)
        hit[torch.from_numpy(rows[inb])] = True
        moved = (g.feature.detach() != before[l]).any(1).cpu()
        assert not (moved & ~hit).any(), f"level {l}: a row without a gradient moved in the first Adam step"
        assert moved[hit].float().mean() > 0.9
        if l == 0:
            assert (~hit).sum() >= 200                  # the dense-indexed level: rows of x > 0 see no sample
    for a, g in zip(stab, net.feature_stability):
        assert torch.equal(a, g.feature.detach())
    for _ in range(29):
        losses.append(float(tr.train_step(mi, gt).detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_tracker_steps_fall_back(tmp_path, caplog):
    from miso_amd.grid_opt.slam.tracker import Tracker
    net = _net(num_poses=2, optimize_pose=True)
    net.set_initial_kf_pose(1, torch.eye(3), torch.tensor([[0.02], [0.0], [-0.01]]), kf_key="KF1")
    n = 512
    x, _, _ = _sphere_batch(n, 3)
    sdf = (x.norm(dim=1, keepdim=True) - 0.5) * 0.1

    class DS(torch.utils.data.Dataset):
        def select_keyframes(self, kfs):
            pass

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return ({"coords_frame": x * 0.8, "sample_frame_ids": torch.ones(n, 1, dtype=torch.int64),
                     "weights": torch.ones(n, 1)},
                    {"sdf": sdf, "sdf_valid": torch.ones(n, 1), "sdf_signs": torch.zeros(n, 1)})

    train = {"verbose": False, "optimizer": "adam", "learning_rate": 1e-3, "epochs": 2, "ckpt_every": -1, "eval_every": -1,
             "eval_metric": None, "pretrained_model": None, "log_dir": str(tmp_path)}
    tracking = {"learning_rate": 1e-3, "verbose": False, "gm_scale_sdf": 0.1, "lm_lambda": 5.0, "lm_max_iter": 2,
                "lm_tol_deg": 0.0, "lm_tol_m": 0.0, "loss_type": "L2", "trunc_dist": 0.12, "solver": "lm"}
    trk = Tracker(net, DS(), {"device": DEV, "train": train, "tracking": tracking})
    info = trk.lm_step(1)
    assert "_lm_dev" not in trk.__dict__                         # the device-side step declined
    assert all(np.isfinite(v) for v in info.values()) and 0 < info["fov_overlap"] <= 1
    assert torch.isfinite(net.rotation_corrections).all() and net.translation_corrections[1].any()
    trk2 = Tracker(net, DS(), {"device": DEV, "train": train, "tracking": dict(tracking, solver="adam")})
    t_before = net.translation_corrections.detach().clone()
    with caplog.at_level(logging.INFO, logger="miso_amd.grid_opt.slam.tracker"):
        trk2.track_window([1], iterations=2)
    assert any("grid.type 'hash' has no fused window" in r.getMessage() for r in caplog.records)
    assert "_adam_dev" not in trk2.__dict__ and not torch.equal(t_before, net.translation_corrections.detach())


def test_two_submap_atlas_takes_the_per_submap_loop():
    from miso_amd.grid_opt.models.grid_atlas import GridAtlas
    from miso_amd.grid_opt.utils.utils_sdf import extract_fields, sphere_tracing
    torch.manual_seed(5)
    atlas = GridAtlas(_cfg(), device=DEV)
    for s, shift in enumerate((0.0, 0.8)):
        atlas.add_submap(torch.tensor(BOUND), torch.eye(3), torch.tensor([[shift], [0.0], [0.0]]), num_poses=2)
        atlas.add_kf(torch.eye(3), torch.zeros(3, 1))
    atlas = atlas.to(DEV)
    with torch.no_grad():
        atlas.get_submap(1).decoder.load_state_dict(atlas.get_submap(0).decoder.state_dict())
    ptrs = [g.feature.data_ptr() for sm in atlas.submaps for g in sm.features]
    x = (torch.rand(300, 3) * 2.6 - torch.tensor([1.0, 1.3, 1.3])).to(DEV)
    with torch.no_grad():
        assert atlas._fused_query(x) is None and atlas._fused_query(x, want_sdf=False, want_feats=True) is None
        sdf, feats = atlas(x), atlas.query_feature(x)
        # the loop's mean over the submaps that contain the point, said again from the submaps
        total, count = 0, 0
        for s, shift in enumerate((0.0, 0.8)):
            xl = x - torch.tensor([shift, 0.0, 0.0], device=DEV)
            inside = ((xl >= -1) & (xl <= 1)).all(1, keepdim=True)
            total, count = total + inside * atlas.get_submap(s).query_feature(xl), count + inside
        assert torch.allclose(feats, total / count.clamp(min=1), atol=1e-6) and (count == 2).any() and (count == 0).any()
        assert sdf.shape == (300, 1) and torch.isfinite(sdf).all()
        assert atlas.sphere_trace(x[:8], torch.ones(8, 3, device=DEV)) is None
        p, hit = sphere_tracing(atlas, x[:8], torch.ones(8, 3, device=DEV), max_iters=10, max_dist=3.0)
        assert p.shape == (8, 3) and torch.isfinite(p).all()
        assert atlas.sdf_on_lattice(*(torch.linspace(-1, 1, 5, device=DEV),) * 3) is None
    b = torch.tensor([[-1.0, 1.8], [-1.0, 1.0], [-1.0, 1.0]])
    u = extract_fields(b[:, 0], b[:, 1], 7, lambda q: atlas(q), device=DEV)
    assert u.shape == (7, 7, 7) and np.isfinite(u).all()
    assert ptrs == [g.feature.data_ptr() for sm in atlas.submaps for g in sm.features]      # no table was re-laid
    # under autograd the loop carries gradients to the tables of both submaps
    atlas(x).abs().sum().backward()
    assert all(sm.features[1].feature.grad is not None and sm.features[1].feature.grad.any() for sm in atlas.submaps)


def _overlapping_atlas(shift=0.6):
    """Two hash submaps of [-1, 1]^3, the second `shift` along x, two keyframes each (global ids 0..3), equal decoders."""
    from miso_amd.grid_opt.models.grid_atlas import GridAtlas
    torch.manual_seed(9)
    atlas = GridAtlas(_cfg(), device=DEV)
    for s in range(2):
        atlas.add_submap(torch.tensor(BOUND), torch.eye(3), torch.tensor([[s * shift], [0.0], [0.0]]), num_poses=2)
        atlas.add_kf(torch.eye(3), torch.zeros(3, 1))
        atlas.add_kf(torch.eye(3), torch.tensor([[0.05], [-0.02], [0.03]]))
    atlas = atlas.to(DEV)
    atlas.get_submap(1).decoder.load_state_dict(atlas.get_submap(0).decoder.state_dict())
    return atlas


class _Samples(torch.utils.data.Dataset):
    """One batch: rows of the four keyframes, most inside both submaps, measured SDF of the sphere (some invalid)."""

    def __len__(self):
        return 1

    def __getitem__(self, i, n=600):
        g = torch.Generator().manual_seed(21)
        x = torch.rand(n, 3, generator=g) * 1.8 - 0.9
        sdf = (x.norm(dim=1, keepdim=True) - 0.5).clamp(-0.2, 0.2)
        return ({"coords_frame": x, "sample_frame_ids": torch.randint(0, 4, (n, 1), generator=g),
                 "weights": torch.ones(n, 1)},
                {"sdf": sdf, "sdf_valid": (torch.rand(n, 1, generator=g) > 0.1).float(), "sdf_signs": torch.zeros(n, 1)})


def test_overlap_gate_of_a_hash_atlas_is_the_lattice_of_its_geometry():
    """check_submap_intersection needs where the finest level IS, not its table: the voxel centres from bound and dims,
    the points a FeatureGrid of that shape lists -- while vertex_positions keeps refusing the latent routes."""
    from miso_amd.grid_opt.models.grid_modules import FeatureGrid
    atlas = _overlapping_atlas()
    fine = atlas.get_submap(0).features[-1]
    dense = FeatureGrid(d=3, fdim=1, bound=torch.tensor(BOUND), cell_size=fine.cell_size)
    assert torch.equal(atlas._finest_vertices(0).cpu(), dense.vertex_positions()) and fine.dims == (16, 16, 16)
    with pytest.raises(ValueError, match="latent alignment"):
        fine.vertex_positions()
    assert bool(atlas.check_submap_intersection(0, 1)) and bool(atlas.check_submap_intersection(1, 0))
    atlas.set_submap_pose(1, torch.eye(3), torch.tensor([[5.0], [0.0], [0.0]]))
    assert not bool(atlas.check_submap_intersection(0, 1))


def test_sdf_space_alignment_runs_on_a_hash_atlas(monkeypatch, caplog):
    """One iteration of every multi-submap SDF-space aligner, overlap gate on (their default): the fused loops decline
    with their log line, the op-by-op loop runs, moves the second submap's pose and leaves finite numbers."""
    import miso_amd.grid_opt.align.base as AB
    import miso_amd.grid_opt.align.mips as MP
    import miso_amd.grid_opt.align.miso as AM
    import miso_amd.grid_opt.align.vfpp as VF
    from miso_amd import ops
    steps, plans = [], []
    step, init = AB._adam_step, ops.AlignPlan.__init__

    def new_step(optimizer, loss_dict, what):
        steps.append({k: float(v.detach()) for k, v in loss_dict.items()})
        return step(optimizer, loss_dict, what)

    def new_init(self, *a, **k):
        plans.append(self)
        init(self, *a, **k)
    monkeypatch.setattr(AB, "_adam_step", new_step)
    monkeypatch.setattr(ops.AlignPlan, "__init__", new_init)
    runs = {
        "sdf": lambda atlas: AM.align_multiple_submaps_hierarchical(atlas, _Samples(), latent_levels=[], finetune_iters=1,
                                                                    device=DEV, verbose=False, finetune_fused=True),
        "vfpp": lambda atlas: VF.align_multiple_submaps_vfpp(atlas, _Samples(), num_iters=1, device=DEV, verbose=False),
        "mips": lambda atlas: MP.align_multiple_submaps_mips(atlas, _Samples(), num_iters=1, device=DEV, verbose=False,
                                                            surf_thresh=0.05),
    }
    for name, run in runs.items():
        atlas = _overlapping_atlas()
        assert AM.fused_sdf_refusal(atlas, DEV) is not None
        steps.clear()
        with caplog.at_level(logging.INFO):
            caplog.clear()
            run(atlas)
        assert not plans, f"{name}: a fused plan was built for a hash atlas"
        assert any("op by op" in r.getMessage() for r in caplog.records), name
        assert len(steps) == 2 and steps[0] and all(np.isfinite(v) for v in steps[0].values()), (name, steps)
        assert any(v > 0 for v in steps[0].values()), (name, steps)          # the gate let the overlapping pairs through
        moved = torch.cat((atlas.rotation_corrections[1].detach().reshape(-1), atlas.translation_corrections[1].detach().reshape(-1)))
        assert torch.isfinite(moved).all() and moved.any(), name
        assert not atlas.rotation_corrections[0].detach().any()               # submap 0 stays fixed
    # the latent stages still say what they need
    with pytest.raises(ValueError, match="latent alignment.*'hash'"):
        AM.align_multiple_submaps_hierarchical(_overlapping_atlas(), _Samples(), level_iters=1, device=DEV, verbose=False)
