"""The SDF pair stage on the GPU (csrc/pair_sdf.hip through ops.AlignPlan(residual="sdf" | "sdf_measured")): the
reference's own numbers, the float64 oracle of tests/pair_sdf_cases.py, the fused fine-tune and Vox-Fusion++ loops
against their op-by-op loops, and the fall-back for a decoder outside the kernel table."""
import logging

import pytest
import torch

import golden_cases as gc
import pair_sdf_cases as pc
from test_grid_opt_mirror import G, T, _OneBatch, close, make_atlas_two_kf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dataset():
    mi, gt = gc.atlas_sdf_batch()
    return _OneBatch(mi, gt)


def _corrections(atlas):
    return (torch.stack([p.detach().cpu().reshape(3) for p in atlas.rotation_corrections]),
            torch.stack([p.detach().cpu().reshape(3) for p in atlas.translation_corrections]))


# ---- the reference's numbers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["L2", "L1", "GM"])
def test_single_pair_plan_matches_the_reference(loss):
    """One iteration_a of a single-pair plan on the rows pairwise_loss_sdf draws: the pair loss and the rows of `flat` of
    both submaps against tests/golden/extra.npz's pairsdf_* entries (the reference's own run), at the bars of
    test_pairwise_loss_sdf_matches_reference."""
    from miso_amd import ops
    import miso_amd.grid_opt.align.miso as AM
    g = G("extra")
    atlas = make_atlas_two_kf(DEV)
    batches = AM.draw_batches(_dataset(), 1, DEV)
    assert AM.fused_sdf_refusal(atlas, DEV) is None
    R0 = torch.stack([R.to(DEV) for R in atlas.R_world_submap_list])
    t0 = torch.stack([t.to(DEV) for t in atlas.t_world_submap_list])
    dr, dt = _corrections(atlas)
    for (a, b) in [(0, 1), (1, 2), (2, 0)]:
        pairs = AM.sdf_pair_inputs(atlas, batches, [(a, b)], check_intersection=False)
        plan = ops.AlignPlan(R0, t0, pairs, loss_type=loss, align_weight=3000.0, residual="sdf",
                             decoder=atlas.get_submap(b)._fused_decoder(), gm_scale=0.1)
        plan.params.copy_(torch.cat((dr, dt), dim=1).to(DEV))
        plan.iteration_a()
        key = f"pairsdf_{a}_{b}_{loss}"
        val = float(plan.pair_losses[0])
        print(key, val, float(g[key]))
        assert abs(val - float(g[key])) <= 3e-5 * abs(float(g[key])), (key, val, float(g[key]))
        flat = plan.flat.cpu()
        for which, s in (("src", a), ("dst", b)):
            close(flat[6 * s:6 * s + 3], T(g[key + f"_gR_{which}"]).reshape(3), 2e-3, 2e-3)
            close(flat[6 * s + 3:6 * s + 6], T(g[key + f"_gt_{which}"]).reshape(3), 2e-3, 2e-3)


# ---- the float64 oracle ------------------------------------------------------------------------------------------------
def _plan_for_case(c, loss, residual="sdf", n_rows=None):
    from miso_amd import ops
    ps = c["pose"]
    R0 = torch.stack([ps[:9].view(3, 3), ps[12:21].view(3, 3)]).to(DEV)
    t0 = torch.stack([ps[9:12].view(3, 1), ps[21:24].view(3, 1)]).to(DEV)
    feats = [f.to(DEV).contiguous(memory_format=torch.channels_last_3d) for f in c["feats"]]
    dec = ops.DecoderPack([w.to(DEV) for w in c["ws"]], [b.to(DEV) for b in c["bs"]])
    pair = dict(src=0, dst=1, coords=c["p"].to(DEV), ref=c["ref"].to(DEV), n_rows=n_rows, feats_dst=feats,
                meta_dst=ops.GridMeta.from_bound(pc.BOUND), gate_pts=None)
    # zero corrections: R0 Exp(0) = R0 and t0 + 0 = t0 exactly, so the kernel maps with the oracle's pose
    return ops.AlignPlan(R0, t0, [pair], loss_type=loss, align_weight=1.0, residual=residual, decoder=dec,
                         gm_scale=pc.GM_SCALE), (feats, dec)


@pytest.mark.parametrize("loss", ["L2", "L1", "GM"])
@pytest.mark.parametrize("n", [2049, 130, 0])
@pytest.mark.parametrize("grid", sorted(pc.GRIDS))
def test_pair_sums_against_the_float64_oracle(grid, n, loss):
    """Count exact, every sum within 1e-4 A + 1e-12 of float64 (pair_sdf_cases), exact fp32 chains; the empty list
    leaves all 24 sums zero and the pair loss 0."""
    from miso_amd import ops
    c = pc.case(grid, n)
    sums, A = pc.pair_sdf_sums64(c["p"], c["ref"], c["feats"], pc.BOUND, c["pose"], c["ws"], c["bs"], loss)
    with ops.exact_fp32():
        plan, keep = _plan_for_case(c, loss)
        plan.iteration_a()
        got = plan.pair_out[0].cpu()
        val = float(plan.pair_losses[0])
    ex = pc.excess(got, sums, A)
    print(grid, n, loss, "count", float(got[1]), float(sums[1]), "worst excess / A", float((ex[2:23] / (A[2:23] + 1e-30)).max()))
    if n == 0:
        assert not got.any() and val == 0.0
        return
    assert got[1] == sums[1] and 0 < sums[1] < n
    assert (ex <= 0).all(), (ex, got, sums)
    # the pair loss of the epilogue: sum / count (n_ch = 1), at the bar of the sum it is formed from
    want = sums[0] / sums[1]
    assert abs(val - float(want)) <= pc.REL * float(A[0] / sums[1]) + 1e-6 * abs(float(want))


def test_measured_residual_divides_by_the_full_row_count():
    """residual "sdf_measured": the same sums, and the pair loss = sum / n_rows whatever the in-bound count."""
    from miso_amd import ops
    c = pc.case("c4l2", 130)
    sums, A = pc.pair_sdf_sums64(c["p"], c["ref"], c["feats"], pc.BOUND, c["pose"], c["ws"], c["bs"], "L2")
    with ops.exact_fp32():
        plan, keep = _plan_for_case(c, "L2", residual="sdf_measured", n_rows=1000)
        plan.iteration_a()
        got, val = plan.pair_out[0].cpu(), float(plan.pair_losses[0])
    assert (pc.excess(got, sums, A) <= 0).all()
    want = float(sums[0]) / 1000.0
    assert abs(val - want) <= pc.REL * float(A[0]) / 1000.0 + 1e-6 * abs(want)


# ---- the loops -----------------------------------------------------------------------------------------------------------
def _record_loops(monkeypatch):
    """Plans the fused route builds, and (loss, sum |d loss / d pose|) of every op-by-op iteration."""
    from miso_amd import ops
    import miso_amd.grid_opt.align.base as AB
    plans, steps = [], []
    init, step = ops.AlignPlan.__init__, AB._adam_step

    def new_init(self, *a, **k):
        init(self, *a, **k)
        plans.append(self)

    def new_step(optimizer, loss_dict, what):
        total = step(optimizer, loss_dict, what)
        gsum = sum(float(p.grad.abs().sum()) for grp in optimizer.param_groups for p in grp["params"] if p.grad is not None)
        steps.append((float(total.detach()), gsum))
        return total
    monkeypatch.setattr(ops.AlignPlan, "__init__", new_init)
    monkeypatch.setattr(AB, "_adam_step", new_step)
    return plans, steps


def _compare_loops(run, plans, steps, iters):
    """run(atlas) -> iteration_results.  Fused against op by op on the same rows, at the bars of
    test_hierarchical_alignment_fused_loop_matches_reference: final corrections and per-iteration pose snapshots to 2e-4.
    Losses: iteration 0 starts from equal poses and is held to 3e-5 relative (the pair loss's bar against the
    reference); from then on the two routes' poses are only known to agree to 2e-4 per component, which moves a loss by
    up to 2e-4 sum |d loss / d pose| to first order (the op-by-op route's own gradient of that iteration) -- added."""
    fused = make_atlas_two_kf(DEV)
    before = _corrections(fused)
    res_f = run(fused)
    assert len(plans) == 1 and plans[0].residual != "latent" and not steps       # the fused route ran, and only it
    ring = plans[0].ring()[:iters, 0].cpu()
    loop = make_atlas_two_kf(DEV)
    loop.no_fused_alignment = True
    res_l = run(loop)
    assert len(plans) == 1 and len(steps) == iters
    for a, b in zip(_corrections(fused), _corrections(loop)):
        close(a, b, 0, 2e-4)
    assert (_corrections(fused)[0][1:] != before[0][1:]).any() and (_corrections(fused)[1][1:] != before[1][1:]).any()
    assert sorted(res_f) == sorted(res_l) == list(range(iters))
    for it in range(iters):
        close(res_f[it].cpu(), res_l[it].cpu(), 0, 2e-4)
        want, gsum = steps[it]
        bar = 3e-5 * abs(want) + (2e-4 * gsum if it else 0.0)
        print("iteration", it, "fused", float(ring[it]), "loop", want, "bar", bar)
        assert abs(float(ring[it]) - want) <= bar, (it, float(ring[it]), want, bar)


@pytest.mark.parametrize("gate,loss", [(False, "L2"), (True, "GM")])
def test_fused_finetune_loop_matches_the_op_by_op_loop(monkeypatch, gate, loss):
    """3 submaps, 3 pairs, 6 iterations of the SDF fine-tune, save_iterations=True, without and with the overlap gate."""
    import miso_amd.grid_opt.align.base as AB
    import miso_amd.grid_opt.align.miso as AM
    plans, steps = _record_loops(monkeypatch)
    ds = _dataset()

    def run(atlas):
        fn = AM.sdf_finetune_loss(atlas, AM.draw_batches(ds, 1, DEV), align_loss=loss, device=DEV)
        return AB.generic_align_multiple_submaps(atlas, ds, ("sdf", fn), num_iters=5, lr=1e-2, check_intersection=gate,
                                                 verbose=False, save_iterations=True)["iteration_results"]
    _compare_loops(run, plans, steps, 6)


def test_hierarchical_takes_the_fused_finetune(monkeypatch):
    """align_multiple_submaps_hierarchical(finetune_fused=True): the fine-tune stage through ops.AlignPlan, info keys kept."""
    import miso_amd.grid_opt.align.miso as AM
    plans, steps = _record_loops(monkeypatch)
    atlas = make_atlas_two_kf(DEV)
    info = AM.align_multiple_submaps_hierarchical(atlas, _dataset(), latent_levels=[], finetune_iters=2, device=DEV,
                                                  verbose=False, save_iterations=True, finetune_fused=True)
    assert [p.residual for p in plans] == ["sdf"] and not steps
    assert sorted(info["hier_sdf_L2"]) == ["cpu_time_sec", "gpu_time_sec", "iteration_results"]
    assert sorted(info["hier_sdf_L2"]["iteration_results"]) == [0, 1, 2]


def test_vfpp_loop_matches_the_op_by_op_loop(monkeypatch):
    """align_multiple_submaps_vfpp: the device loop (residual "sdf_measured", overlap gate on) against the op-by-op one."""
    import miso_amd.grid_opt.align.vfpp as VF
    plans, steps = _record_loops(monkeypatch)
    ds = _dataset()

    def run(atlas):
        return VF.align_multiple_submaps_vfpp(atlas, ds, num_iters=5, lr=1e-2, device=DEV, verbose=False,
                                              save_iterations=True)["iteration_results"]
    _compare_loops(run, plans, steps, 6)
    assert plans[0].residual == "sdf_measured"


# ---- fall-back -----------------------------------------------------------------------------------------------------------
def test_decoder_outside_the_table_takes_the_op_by_op_loop(monkeypatch, caplog):
    import miso_amd.grid_opt.align.miso as AM
    from miso_amd.grid_opt.models.grid_atlas import GridAtlas
    c = gc.ATLAS
    cfg = gc.model_cfg(c["bound"], c["base_cell"], c["scale"], c["n_levels"], c["fdim"], 48)      # hidden 48
    atlas = GridAtlas(cfg, device=DEV)
    for s, sub in enumerate(gc.atlas_inputs()):
        atlas.add_submap(torch.tensor(c["bound"], dtype=torch.float32), T(sub["R"]), T(sub["t"]), num_poses=2)
        atlas.add_kf(torch.eye(3), torch.zeros(3, 1))
        R2, t2 = gc.atlas_second_kf_pose(s)
        atlas.add_kf(T(R2), T(t2))
        with torch.no_grad():
            for l, f in enumerate(sub["features"]):
                atlas.get_submap(s).features[l].feature.copy_(T(f))
        atlas.get_submap(s).decoder.load_state_dict(atlas.get_submap(0).decoder.state_dict())
    atlas = atlas.to(DEV)
    plans, steps = _record_loops(monkeypatch)
    with caplog.at_level(logging.INFO, logger=AM.logger.name):
        info = AM.align_multiple_submaps_hierarchical(atlas, _dataset(), latent_levels=[], finetune_iters=1, device=DEV,
                                                      verbose=False, finetune_fused=True)
    assert not plans and len(steps) == 2
    assert any("op by op" in r.getMessage() and "kernels' table" in r.getMessage() for r in caplog.records)
    assert "hier_sdf_L2" in info
