"""grid.hash_fused = True: what reaches a hash GridNet through forward() and sdf_and_gradient() takes the one-launch
route (ops.hash_sdf_*), and gives what the op-by-op route gives.  The fixtures are tests/test_hash_routing.py's: the
analytic sphere |x| - 0.5 in [-1, 1]^3, level 0 (8^3 vertices) dense-indexed behind 2^10 rows, level 1 (16^3) hashed four
vertices to a row."""
import numpy as np
import pytest
import torch

import golden_cases as gc
import hash_cases as hc
import sampler_cases as sc
import test_hash_routing as base

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND, LOG2 = base.BOUND, base.LOG2


def _net(seed=0, fused=True, **kw):
    from miso_amd.grid_opt.models.grid_net import GridNet
    cfg = base._cfg(**kw)
    if fused is not None:
        cfg["grid"]["hash_fused"] = fused
    torch.manual_seed(seed)
    net = GridNet(cfg, device=DEV).to(DEV)
    net.set_initial_kf_pose(0, torch.eye(3), torch.zeros(3, 1), kf_key="KF0")
    assert [(g.dims, g.dense_indexed) for g in net.features] == [((8, 8, 8), True), ((16, 16, 16), False)]
    return net


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _count(monkeypatch, *names):
    """call counters on ops.<name>"""
    from miso_amd import ops
    calls = {n: 0 for n in names}
    for n in names:
        def wrapped(*a, _n=n, _f=getattr(ops, n), **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, n, wrapped)
    return calls


def test_pack_and_route(monkeypatch):
    from miso_amd import ops
    net = _net()
    x = base._sphere_batch(257, 1)[0].to(DEV)
    pack = net._fused_hash_decoder()
    assert isinstance(pack, ops.DecoderPack) and net._fused_decoder() is None and net.hash_fused is True
    direct, _ = ops.hash_sdf_fwd_raw(x, *net._hash_args(detach=True), pack, False)
    calls = _count(monkeypatch, "hash_sdf_fwd_raw", "hash_encode_fwd_raw")
    with torch.no_grad():
        sdf = net(x)
    assert calls == {"hash_sdf_fwd_raw": 1, "hash_encode_fwd_raw": 0}
    assert sdf.shape == (257, 1) and torch.equal(_bits(sdf), _bits(direct)) and sdf.std() > 0
    # the op-by-op route of the same net (switch off) is the same field, to the arithmetic of the decoder
    net.hash_fused = False
    assert net._fused_hash_decoder() is None
    with torch.no_grad():
        ref = net(x)
    assert calls == {"hash_sdf_fwd_raw": 1, "hash_encode_fwd_raw": 1}
    assert (sdf - ref).abs().max() <= 2e-6 * max(1.0, float(ref.abs().max()))      # test_split_precision's level
    # a trainable decoder has no frozen pack: the route declines
    net.hash_fused = True
    for p in net.decoder.parameters():
        p.requires_grad_(True)
    assert net._fused_hash_decoder() is None


def test_dense_indexed_twin_gives_the_regular_nets_fused_bits():
    """test_hash_encode's construction: a hash net whose levels all fit their table holds a regular GridNet's values row
    for row -- here against the regular net's FUSED forward, which is one kernel on each side."""
    from miso_amd.grid_opt.models.grid_net import GridNet

    def cfg(grid_type):
        c = gc.model_cfg(sc.BOUNDS[hc.BOUND], 0.4, 2.0, 2, 4, 64, init_stddev=0.1)
        c["grid"]["type"] = grid_type
        if grid_type == "hash":
            c["grid"]["log2_hashmap_size"], c["grid"]["hash_fused"] = 19, True
        return c
    torch.manual_seed(3)
    reg = GridNet(cfg("regular"), device=DEV).to(DEV)
    hsh = GridNet(cfg("hash"), device=DEV).to(DEV)
    hsh.decoder.load_state_dict(reg.decoder.state_dict())
    with torch.no_grad():
        for a, b in zip(hsh.features, reg.features):
            assert a.dense_indexed and a.dims == tuple(reversed(b.feature.shape[2:]))
            a.feature.copy_(b.feature.permute(0, 2, 3, 4, 1).reshape(-1, a.feature.shape[1]))
    assert reg._fused_decoder() is not None and hsh._fused_hash_decoder() is not None
    x = hc.points().x.to(DEV)
    with torch.no_grad():
        a, b = hsh(x), reg(x)
    assert a.shape == (x.shape[0], 1) and torch.equal(_bits(a), _bits(b)) and a.abs().max() > 0
    sa, ga = hsh.sdf_and_gradient(x)
    sb, gb = reg.sdf_and_gradient(x)
    assert torch.equal(_bits(sa), _bits(a)) and torch.equal(_bits(sa), _bits(sb))
    assert ga.shape == gb.shape == (x.shape[0], 3) and torch.isfinite(ga).all()


def test_sdf_and_gradient_builds_no_graph(monkeypatch):
    net = _net()
    net.unlock_feature()
    xd = base._sphere_batch(257, 1)[0].to(DEV)
    with torch.no_grad():
        sdf = net(xd)
    calls = _count(monkeypatch, "hash_encode_bwd_raw", "hash_sdf_fwd_raw", "hash_sdf_bwd_raw")
    graphs = []
    grad = torch.autograd.grad
    monkeypatch.setattr(torch.autograd, "grad", lambda *a, **k: graphs.append(1) or grad(*a, **k))
    s2, gx = net.sdf_and_gradient(xd)
    monkeypatch.setattr(torch.autograd, "grad", grad)
    assert calls == {"hash_encode_bwd_raw": 0, "hash_sdf_fwd_raw": 1, "hash_sdf_bwd_raw": 1} and not graphs
    assert torch.equal(s2, sdf) and gx.shape == (257, 3) and not gx.requires_grad and not s2.requires_grad
    assert all(g.feature.grad is None for g in net.features)
    # against central differences of forward(): test_hash_routing's criterion, word for word
    h = 1e-3
    with torch.no_grad():
        fd = torch.cat([(net(xd + h * e) - net(xd - h * e)) / (2 * h) for e in torch.eye(3, device=DEV)], 1)
    frac = ((xd + 1) * 8 - 0.5) % 1
    inner = ((frac > 0.02) & (frac < 0.98)).all(1) & (xd.abs().max(1).values < 0.9)
    err = (fd - gx)[inner].abs().max(1).values
    assert inner.sum() > 150 and torch.quantile(err, 0.9) <= 0.02 * gx.abs().max() + 1e-5, torch.quantile(err, 0.9)


def test_mapping_trains_through_the_fused_route(tmp_path, monkeypatch):
    """test_hash_routing's training assertions with the switch on: one Trainer step with MisoLossMapping (L1 + free
    space) moves the rows that received a gradient and no other; 30 steps later the loss is below the first step's."""
    net = _net()
    net.unlock_feature()
    net.lock_pose()
    tr = base._trainer(net, tmp_path)
    calls = _count(monkeypatch, "hash_sdf_fwd_raw", "hash_sdf_bwd_raw", "hash_encode_fwd_raw")
    x, mi, gt = base._sphere_batch(2048, 2, half=True)
    before = [g.feature.detach().clone() for g in net.features]
    stab = [g.feature.detach().clone() for g in net.feature_stability]
    losses = [float(tr.train_step(mi, gt).detach())]
    assert calls["hash_sdf_fwd_raw"] >= 1 and calls["hash_sdf_bwd_raw"] >= 1 and calls["hash_encode_fwd_raw"] == 0
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
            assert (~hit).sum() >= 200
    for a, g in zip(stab, net.feature_stability):
        assert torch.equal(a, g.feature.detach())
    for _ in range(29):
        losses.append(float(tr.train_step(mi, gt).detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_extract_fields_and_the_tracker_pick_the_route_up(tmp_path, monkeypatch):
    from miso_amd.grid_opt.slam.tracker import Tracker
    from miso_amd.grid_opt.utils.utils_sdf import extract_fields
    net = _net(num_poses=2, optimize_pose=True)
    calls = _count(monkeypatch, "hash_sdf_fwd_raw", "hash_sdf_bwd_raw", "hash_encode_fwd_raw")
    b = torch.tensor(BOUND)
    u = extract_fields(b[:, 0], b[:, 1], 9, lambda q: net(q), device=DEV)
    assert u.shape == (9, 9, 9) and np.isfinite(u).all() and calls["hash_sdf_fwd_raw"] >= 1
    net.set_initial_kf_pose(1, torch.eye(3), torch.tensor([[0.02], [0.0], [-0.01]]), kf_key="KF1")
    n = 512
    x = base._sphere_batch(n, 3)[0]
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
    seen = dict(calls)
    info = trk.lm_step(1)
    assert calls["hash_sdf_bwd_raw"] > seen["hash_sdf_bwd_raw"]            # sdf_and_gradient on the fused route
    assert all(np.isfinite(v) for v in info.values()) and 0 < info["fov_overlap"] <= 1
    assert torch.isfinite(net.rotation_corrections).all() and net.translation_corrections[1].any()
    trk2 = Tracker(net, DS(), {"device": DEV, "train": train, "tracking": dict(tracking, solver="adam")})
    t_before = net.translation_corrections.detach().clone()
    seen = dict(calls)
    trk2.track_window([1], iterations=2)
    assert calls["hash_sdf_fwd_raw"] > seen["hash_sdf_fwd_raw"] and calls["hash_encode_fwd_raw"] == 0
    assert torch.isfinite(net.translation_corrections).all()
    assert not torch.equal(t_before, net.translation_corrections.detach())


def test_switch_absent_keeps_the_op_by_op_route(monkeypatch):
    net = _net(fused=None)
    assert net.hash_fused is False and net._fused_hash_decoder() is None
    calls = _count(monkeypatch, "hash_sdf_fwd_raw", "hash_sdf_bwd_raw", "hash_encode_fwd_raw")
    x = base._sphere_batch(65, 4)[0].to(DEV)
    with torch.no_grad():
        net(x)
    net.sdf_and_gradient(x)
    assert calls["hash_sdf_fwd_raw"] == 0 and calls["hash_sdf_bwd_raw"] == 0 and calls["hash_encode_fwd_raw"] >= 2
