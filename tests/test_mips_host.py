"""MIPS-Fusion's projected-match residual without a GPU: the closed form the kernel sums against the reference's formula
written literally (float64 autograd is the judge), the bar of the GPU tests and what it must see, what
miso_align_plan_build takes and refuses for residual 3, and align/mips.py op by op on the CPU."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import mips_cases as mc
import pair_sdf_cases as pc
import test_pair_sdf_host as ph
from miso_amd import _lib
from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
HERE = os.path.dirname(os.path.abspath(__file__))
SURF = mc.SURF


def _sums(c, constraint, **kw):
    return mc.mips_sums64(c["p"], c["normals"], c["feats"], mc.BOUND, c["pose"], c["ws"], c["bs"], constraint, **kw)


# ---- 1. the closed form against the literal formula ---------------------------------------------------------------------
@pytest.mark.parametrize("constraint", mc.CONSTRAINTS)
@pytest.mark.parametrize("grid", mc.GRIDS)
def test_closed_form_equals_the_literal_formula(grid, constraint):
    """Exactly orthonormal float64 rotations (pair_sdf_cases.pose's draws through rodrigues, not rounded to fp32): the
    closed form's 24 sums, pulled back to d / d (dr, dt) with the epilogue's algebra, equal float64 autograd of the
    reference's formula to 1e-9 of the pulled-back yardstick."""
    c = mc.case(grid, 2049)
    rs = np.random.RandomState(5)                                          # pair_sdf_cases.case: pose(5 + seed)
    Rs, Rd = (torch.tensor(gc.rodrigues(rs.uniform(-0.3, 0.3, 3)), dtype=F64) for _ in range(2))
    assert torch.equal(Rs.float(), c["pose"][:9].view(3, 3)) and torch.equal(Rd.float(), c["pose"][12:21].view(3, 3))
    for Rm in (Rs, Rd):
        assert (Rm @ Rm.T - torch.eye(3, dtype=F64)).abs().max() < 1e-15
    ts, td = c["pose"][9:12].double(), c["pose"][21:24].double()
    pose = torch.cat([Rs.flatten(), ts, Rd.flatten(), td])
    sums, A = mc.mips_sums64(c["p"], c["normals"], c["feats"], mc.BOUND, pose, c["ws"], c["bs"], constraint, map64=True)
    assert 0 < sums[1] < 2049
    loss, grads, bar = mc.pull_back(sums, A, Rs, Rd, Rd, constraint, weight=3000.0)
    want_loss, want, kept = mc.mips_literal64(c["p"], c["normals"], c["feats"], mc.BOUND, (Rs, Rd), (ts, td), c["ws"],
                                              c["bs"], constraint, weight=3000.0)
    assert kept == int(sums[1])
    assert abs(loss - want_loss) <= 1e-9 * 3000.0 * float(A[0]) / (kept * mc.N_CH[constraint])
    for name, got, w, y in zip(("dr_s", "dt_s", "dr_d", "dt_d"), grads, want, bar):
        assert w.abs().max() > 0
        print(grid, constraint, name, "worst |closed - literal| / yardstick", float(((got - w).abs() / y).max()))
        assert ((got - w).abs() <= 1e-9 * y).all(), (name, got, w, y)


# ---- 2., 3. the bar ------------------------------------------------------------------------------------------------------
_SUMS_ONLY = [0] + list(range(2, 23))


@pytest.mark.parametrize("grid", mc.GRIDS)
def test_the_bar_sees_what_it_must(grid):
    c = mc.case(grid, 2049)
    n = c["p"].shape[0]
    # the S2 term left out, point-to-plane
    sums, A = _sums(c, "point_to_plane")
    without, _ = _sums(c, "point_to_plane", s2=False)
    assert torch.equal(without[:5], sums[:5])
    assert (mc.excess(without, sums, A)[5:23] > 0).any()
    # the sign of g flipped on 1 % of the in-bound rows
    _, _, m = R.src_to_dst32(c["p"], c["pose"][:9], c["pose"][9:12], c["pose"][12:21], c["pose"][21:24], mc.BOUND)
    sign = torch.ones(n)
    sign[torch.nonzero(m).flatten()[::100]] = -1.0
    for constraint in mc.CONSTRAINTS:
        sums, A = _sums(c, constraint)
        flip, _ = _sums(c, constraint, g_sign=sign)
        assert flip[1] == sums[1]
        assert (mc.excess(flip, sums, A)[_SUMS_ONLY] > 0).any(), constraint
        # ... and the count off by one
        one = sums.clone()
        one[1] += 1
        assert mc.excess(one, sums, A)[1] > 0


@pytest.mark.parametrize("constraint", mc.CONSTRAINTS)
@pytest.mark.parametrize("grid", mc.GRIDS)
def test_fp32_restatement_is_within_the_bar(grid, constraint):
    """What set REL_MIPS (mips_cases.py): a careful fp32 evaluation at the same coordinates, on every case of the GPU
    tests; the worst ratio is printed."""
    assert mc.REL_MIPS <= 1e-3
    for n in (2049, 130):
        c = mc.case(grid, n)
        sums, A = _sums(c, constraint)
        s32, _ = _sums(c, constraint, dtype=F32)
        ratio = (((s32 - sums).abs() - 1e-12).clamp(min=0) / (A + 1e-300))[_SUMS_ONLY]
        print(grid, constraint, n, "count", int(sums[1]), "worst (|fp32 - fp64| - 1e-12) / A", float(ratio.max()))
        assert 0 < sums[1] < n and s32[1] == sums[1]
        assert (mc.excess(s32, sums, A) <= 0).all()
        assert 4 * float(ratio.max()) <= mc.REL_MIPS
    assert not any(v.any() for v in _sums(mc.case(grid, 0), constraint))


def test_case_rows_and_normals():
    for grid in mc.GRIDS:
        for n in (2049, 130, 0):
            c = mc.case(grid, n)
            assert c["normals"].shape == (n, 3) and c["normals"].dtype == F32
            assert torch.equal(c["p"], pc.case(grid, n)["p"])
            if n:
                assert (c["normals"].norm(dim=1) - 1).abs().max() < 1e-6


# ---- 4. plan build -------------------------------------------------------------------------------------------------------
def _build(residual, constraint=0, loss_type=2, hidden=64, pair=None, **kw):
    """test_pair_sdf_host._build with miso_align_t.constraint set: host addresses, nothing launched"""
    lib = _lib.load()
    cfg = ph.cr.align_cfg()
    cfg.residual, cfg.loss_type, cfg.gm_scale, cfg.constraint = residual, loss_type, 0.1, constraint
    keep = _lib.Mlp()
    keep.in_dim, keep.hidden_dim, keep.out_dim, keep.n_linear = ph.cr.F, hidden, 1, 3
    for i in range(3):
        keep.weight[i] = ph._ADDR
    cfg.mlp, cfg.packed = C.pointer(keep), ph._ADDR
    pairs = (_lib.AlignPair * 1)(pair or ph._pair())
    blob = (C.c_uint8 * int(lib.miso_align_plan_bytes(1)))()
    return lib.miso_align_plan_build(pairs, C.byref(cfg), blob), cfg


def test_align_struct_ends_in_the_constraint():
    names = [f[0] for f in _lib.Align._fields_]
    assert names[-1] == "constraint" and names[-2] == "sdf_shape"


def test_plan_build_takes_and_refuses_the_projected_match():
    # residual 3 needs constraint 1 or 2 and the L2 loss
    for constraint in (1, 2):
        rc, cfg = _build(3, constraint)
        assert rc == 0 and cfg.max_n == ph.cr.N and cfg.sdf_shape != 0
    assert _build(3, 0)[0] == _lib.E_BADARG
    assert _build(3, 3)[0] == _lib.E_BADARG
    assert _build(3, -1)[0] == _lib.E_BADARG
    for lt in (1, 3):
        assert _build(3, 1, loss_type=lt)[0] == _lib.E_BADARG
        assert _build(3, 2, loss_type=lt)[0] == _lib.E_BADARG
    assert _build(4, 1)[0] == _lib.E_BADARG
    # a constraint without residual 3
    for residual in (0, 1, 2):
        for constraint in (1, 2):
            assert _build(residual, constraint)[0] == _lib.E_BADARG
    # point-to-plane reads the normals: NULL, or a pitch below 3, is refused; point-to-point reads neither
    null = ph._pair()
    null.feats_src = None
    assert _build(3, 1, pair=null)[0] == _lib.E_BADARG
    assert _build(3, 2, pair=null)[0] == 0
    thin = ph._pair()
    thin.ld_feats = 2
    assert _build(3, 1, pair=thin)[0] == _lib.E_BADARG
    assert _build(3, 2, pair=thin)[0] == 0
    # the shape and flag refusals of residual 1
    assert _build(3, 1, hidden=48)[0] == _lib.E_UNSUPPORTED
    assert _build(3, 2, hidden=48)[0] == _lib.E_UNSUPPORTED
    for flag in (_lib.F_PAD_BORDER, _lib.F_ALIGN_CORNERS, _lib.F_COORDS_NORMALIZED):
        p = ph._pair()
        p.dst_grid.flags = flag
        assert _build(3, 1, pair=p)[0] == _lib.E_UNSUPPORTED
    # constraint 0: the residuals of before answer as before
    for residual, lt in ((0, 1), (0, 2), (1, 1), (1, 2), (1, 3), (2, 2)):
        assert _build(residual, 0, loss_type=lt)[0] == 0, (residual, lt)
    assert _build(2, 0, loss_type=1)[0] == _lib.E_BADARG
    assert _build(0, 0, loss_type=3)[0] == _lib.E_BADARG
    # the blob size is the one of before
    with open(os.path.join(HERE, "golden", "capi_refusals.json")) as f:
        one = json.load(f)["miso_align_plan_bytes:valid"]
    assert _lib.load().miso_align_plan_bytes(1) == one and _lib.load().miso_align_plan_bytes(28) == 28 * one


# ---- 5. align/mips.py on the CPU -----------------------------------------------------------------------------------------
def _atlas_rows64(src, mi, gt):
    """The rows of ``src``'s keyframes in its frame, float64, their gt sdf, and the source normals grad s_src there."""
    c = gc.ATLAS
    subs = gc.atlas_inputs()
    ids = T(mi["sample_frame_ids"][0, :, 0])
    rows = torch.nonzero(ids // 2 == src).squeeze(1)                       # keyframes 2s, 2s + 1 belong to submap s
    R2, t2 = gc.atlas_second_kf_pose(src)
    R_kf = torch.stack([torch.eye(3, dtype=F64), T(R2).double()])
    t_kf = torch.stack([torch.zeros(3, 1, dtype=F64), T(t2).double()])
    x = R.transform_by_keyframe_loop(T(mi["coords_frame"][0]).double()[rows], ids[rows] - 2 * src, R_kf, t_kf)
    ws, bs = R.decoder_params({k: T(v).double() for k, v in gc.make_decoder(c).items()})
    xg = x.clone().requires_grad_(True)
    s = R.sdf_stock([T(f).double() for f in subs[src]["features"]], torch.tensor(c["bound"], dtype=F64), xg, ws, bs)
    (normals,) = torch.autograd.grad(s.sum(), xg)
    return x, T(gt["sdf"][0]).double()[rows, 0], normals, ws, bs


def _atlas_literal(src, dst, mi, gt, constraint, surf=SURF, weight=3000.0, dtype=F64):
    subs = gc.atlas_inputs()
    x, sdf, normals, ws, bs = _atlas_rows64(src, mi, gt)
    surface = sdf.abs() < surf
    pose = lambda s, k: T(subs[s][k]).double()
    out = mc.mips_literal64(x[surface], normals[surface], [T(f) for f in subs[dst]["features"]], gc.ATLAS["bound"],
                            (pose(src, "R"), pose(dst, "R")), (pose(src, "t").reshape(3), pose(dst, "t").reshape(3)), ws, bs,
                            constraint, weight=weight, dr=(pose(src, "dr").reshape(3), pose(dst, "dr").reshape(3)),
                            dt=(pose(src, "dt").reshape(3), pose(dst, "dt").reshape(3)), stock=True, dtype=dtype)
    return out + (int(surface.sum()),)


def test_atlas_case_counts():
    """At the reference's 1e-3 only a handful of the 900 rows are surface; at SURF every source submap keeps at least 64
    rows and every ordered pair at least 16 of them in the destination's bound at the initial poses."""
    mi, gt = gc.atlas_sdf_batch()
    S = gc.ATLAS["n_submaps"]
    for a in range(S):
        for b in range(S):
            if a != b:
                _, _, kept, surface = _atlas_literal(a, b, mi, gt, "point_to_point")
                print("pair", a, b, "surface rows", surface, "in the destination's bound", kept)
                assert surface >= 64 and kept >= 16, (a, b, surface, kept)
    x, sdf, *_ = _atlas_rows64(0, mi, gt)
    assert int((sdf.abs() < 1e-3).sum()) < 16


@pytest.mark.parametrize("constraint", mc.CONSTRAINTS)
def test_pairwise_loss_mips_matches_the_literal_formula(monkeypatch, constraint):
    """float32, op by op, against mips_literal64 at the atlas' corrections: loss to 3e-5 relative, pose gradients to
    (2e-3, 2e-3), the bars test_pair_sdf.py holds the SDF residuals to against the reference's numbers.

    The route forms p - match_src as a difference of two points of size |p| ~ 1 m that leaves s g, 1e-4 .. 1e-2 m here:
    its own fp32 rounding is not small beside 3e-5 on a pair of few rows.  Measured as the literal formula in fp32
    against itself in float64 (mips_literal64(dtype=F32), same rows), relative to the loss: point_to_plane (0,1) 6.1e-6,
    (1,2) 3.1e-6, (2,0) 5.4e-5 (17 rows, loss 9.9e-6); point_to_point 9.3e-6, 8.8e-7, 1.1e-6.  Where twice that exceeds
    3e-5 -- pair (2,0), point_to_plane -- the loss is held to twice the measurement instead, taken in the test.  The
    point-to-plane gradients are 1e-5 .. 1e-3 in size, far below the absolute 2e-3: they are also held to 2e-3 of their
    largest component plus twice the same measurement of each."""
    from test_grid_opt_mirror import close
    import miso_amd.grid_opt.align.mips as MP
    atlas, ds, mi, gt = ph._two_kf_atlas(monkeypatch)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)
    for (a, b) in [(0, 1), (1, 2), (2, 0)]:
        atlas.zero_grad(set_to_none=True)
        d = MP.pairwise_loss_mips(atlas, loader, a, b, constraint_type=constraint, device="cpu", surf_thresh=SURF)
        assert list(d) == [f"mips_{a}_{b}"]
        (val,) = d.values()
        val.backward()
        want, grads, kept, _ = _atlas_literal(a, b, mi, gt, constraint)
        want32, grads32, kept32, _ = _atlas_literal(a, b, mi, gt, constraint, dtype=F32)
        noise = abs(want32 - want)
        print(constraint, a, b, "rows", kept, "loss", val.item(), want, "fp32 route's noise / loss", noise / want)
        assert kept32 == kept and want > 0
        assert abs(val.item() - want) <= max(3e-5 * abs(want), 2 * noise), (a, b, val.item(), want, noise)
        for s, i in ((a, 0), (b, 2)):
            for got, w, w32 in ((atlas.rotation_corrections[s].grad, grads[i], grads32[i]),
                                (atlas.translation_corrections[s].grad, grads[i + 1], grads32[i + 1])):
                close(got.double(), w.reshape(got.shape), 2e-3, 2e-3)
                close(got.double(), w.reshape(got.shape), 2e-3, 2 * float((w32.double() - w).abs().max()))


def test_pairwise_loss_mips_without_rows_of_the_source(monkeypatch, caplog):
    import miso_amd.grid_opt.align.mips as MP
    atlas, _, mi, gt = ph._two_kf_atlas(monkeypatch)
    from test_grid_opt_mirror import _OneBatch
    mi = dict(mi, sample_frame_ids=np.zeros_like(mi["sample_frame_ids"]))      # every row belongs to submap 0
    loader = torch.utils.data.DataLoader(_OneBatch(mi, gt), batch_size=1, shuffle=False, num_workers=0)
    assert MP.pairwise_loss_mips(atlas, loader, 1, 0, device="cpu", surf_thresh=SURF) == {}
    assert any("No samples found for submap 1" in r.getMessage() for r in caplog.records)
    with pytest.raises(ValueError):
        MP.pairwise_loss_mips(atlas, loader, 0, 1, constraint_type="plane", device="cpu")


def test_mips_loop_on_the_cpu_runs_op_by_op(monkeypatch, caplog):
    """The atlas on the CPU: align_multiple_submaps_mips takes the op-by-op loop, says why, and moves the poses."""
    import logging
    import miso_amd.grid_opt.align.mips as MP
    atlas, ds, _, _ = ph._two_kf_atlas(monkeypatch)
    before = torch.cat([p.detach().reshape(-1).clone() for p in atlas.rotation_corrections])
    with caplog.at_level(logging.INFO, logger=MP.logger.name):
        info = MP.align_multiple_submaps_mips(atlas, ds, num_iters=1, device="cpu", verbose=False, surf_thresh=SURF,
                                              save_iterations=True)
    assert sorted(info["iteration_results"]) == [0, 1]
    assert any("runs op by op" in r.getMessage() and "not on the GPU" in r.getMessage() for r in caplog.records)
    after = torch.cat([p.detach().reshape(-1) for p in atlas.rotation_corrections])
    assert torch.equal(before[:3], after[:3]) and (before[3:] != after[3:]).any()


def test_mips_signatures_follow_the_reference():
    import miso_amd.compat  # noqa: F401
    import grid_opt.align.mips as alias
    import miso_amd.grid_opt.align.mips as MP
    assert alias is MP and MP.pairwise_loss_mips_scannet is MP.pairwise_loss_mips
    sig = inspect.signature(MP.pairwise_loss_mips).parameters
    assert list(sig)[:8] == ["grid_atlas", "data_loader", "src_id", "dst_id", "residual_weight", "use_bound",
                             "constraint_type", "device"]
    assert sig["residual_weight"].default == 3000 and sig["constraint_type"].default == "point_to_plane"
    assert sig["use_bound"].default is True and sig["surf_thresh"].default == 1e-3
    sig = inspect.signature(MP.align_multiple_submaps_mips).parameters
    assert list(sig)[:13] == ["grid_atlas", "dataset", "dataset_name", "num_iters", "lr", "residual_weight", "use_bound",
                              "constraint_type", "pose_reg_weight", "pose_thresh_m", "pose_thresh_rad", "device", "verbose"]
    assert sig["num_iters"].default == 100 and sig["lr"].default == 1e-2 and sig["dataset_name"].default == "SubmapSdf3D"
    sig = inspect.signature(MP.align_submap_pair_mips).parameters
    assert list(sig)[:12] == ["grid_atlas", "dataset", "src_id", "dst_id", "dataset_name", "num_iters", "lr",
                              "residual_weight", "use_bound", "constraint_type", "device", "verbose"]
