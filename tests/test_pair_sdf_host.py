"""The host side of the SDF alignment residuals, without a GPU: the new fields of miso_align_t and what
miso_align_plan_build refuses for them, align/vfpp.py on the CPU against a float64 restatement, the fall-back of the
fused fine-tune, and the float64 oracle of the SDF pair stage (tests/pair_sdf_cases.py) with the bar the GPU tests hold
the kernel to."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest
import torch

import capi_refusal_cases as cr
import golden_cases as gc
import pair_sdf_cases as pc
from miso_amd import _lib
from oracle import ref_torch as R

F32, F64 = torch.float32, torch.float64
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def test_align_struct_has_the_sdf_fields():
    names = [f[0] for f in _lib.Align._fields_]
    for field in ("residual", "mlp", "packed", "gm_scale"):
        assert field in names, field
    # behind everything the latent form reads: with all of them zero the struct is the old one, longer
    assert names.index("residual") > names.index("poses_ready")


# descriptors as tests/capi_refusal_cases.py builds its own (same shapes and values), with every pointer at one live,
# aligned host address of this module: plan_build is host code, launches nothing and reads none of them
_LIVE = C.create_string_buffer(1 << 12)
_ADDR = (C.addressof(_LIVE) + 255) & ~255


def _pair():
    p = _lib.AlignPair()
    g = p.dst_grid
    g.n_levels, g.ignore_mask, g.flags = 2, 0, 0
    for a in range(3):
        g.bound_min[a], g.bound_max[a] = 0.0, 1.0
    for l in range(_lib.MAX_LEVELS):
        s = g.level[l]
        s.data = _ADDR
        s.C, s.X, s.Y, s.Z = 4, 3, 3, 3
        s.sC, s.sX, s.sY, s.sZ = 1, 4, 12, 36
    p.coords_src, p.feats_src, p.ld_feats, p.n = _ADDR, _ADDR, cr.F, cr.N
    p.gate_coords, p.gate_n, p.src, p.dst = _ADDR, 4, 0, 1
    return p


def _build(residual=0, loss_type=2, mlp="valid", packed="valid", gm_scale=0.1, hidden=64, pair=None):
    lib = _lib.load()
    cfg = cr.align_cfg()
    cfg.residual, cfg.loss_type, cfg.gm_scale = residual, loss_type, gm_scale
    keep = None
    if mlp == "valid":
        keep = _lib.Mlp()
        keep.in_dim, keep.hidden_dim, keep.out_dim, keep.n_linear = cr.F, hidden, 1, 3
        for i in range(3):
            keep.weight[i] = _ADDR
        cfg.mlp = C.pointer(keep)
    if packed == "valid":
        cfg.packed = _ADDR
    pairs = (_lib.AlignPair * 1)(pair or _pair())
    blob = (C.c_uint8 * int(lib.miso_align_plan_bytes(1)))()
    return lib.miso_align_plan_build(pairs, C.byref(cfg), blob), cfg, keep


def test_plan_build_refuses_what_the_sdf_residuals_do_not_cover():
    assert _build(residual=3)[0] == _lib.E_BADARG
    assert _build(residual=-1)[0] == _lib.E_BADARG
    assert _build(residual=1, mlp=None)[0] == _lib.E_BADARG
    assert _build(residual=1, packed=None)[0] == _lib.E_BADARG
    assert _build(residual=0, loss_type=3)[0] == _lib.E_BADARG
    assert _build(residual=2, loss_type=1)[0] == _lib.E_BADARG            # the measured-SDF loss is L2
    assert _build(residual=2, loss_type=3)[0] == _lib.E_BADARG
    assert _build(residual=1, loss_type=3, gm_scale=0.0)[0] == _lib.E_BADARG
    assert _build(residual=1, hidden=48)[0] == _lib.E_UNSUPPORTED         # a decoder outside the kernel table
    for flag in (_lib.F_PAD_BORDER, _lib.F_ALIGN_CORNERS, _lib.F_COORDS_NORMALIZED):
        p = _pair()
        p.dst_grid.flags = flag
        assert _build(residual=1, pair=p)[0] == _lib.E_UNSUPPORTED
    big = _pair()
    big.ld_feats = 1 << 24                                                 # residual 2: the source's full row count
    assert _build(residual=2, pair=big)[0] == _lib.E_TOOLARGE
    # ... and takes what they do
    for residual, lt in ((1, 1), (1, 2), (1, 3), (2, 2)):
        rc, cfg, _ = _build(residual=residual, loss_type=lt)
        assert rc == 0, (residual, lt, rc)
        assert cfg.max_n == cr.N and cfg.vec4 == 1
    # the latent form: every new field zero, today's answer
    rc, cfg, _ = _build(residual=0, mlp=None, packed=None, gm_scale=0.0)
    assert rc == 0 and cfg.sdf_shape == 0


def test_plan_blob_size_is_unchanged():
    with open(os.path.join(HERE, "golden", "capi_refusals.json")) as f:
        golden = json.load(f)
    one = golden["miso_align_plan_bytes:valid"]
    assert _lib.load().miso_align_plan_bytes(3) == 3 * one
    assert _lib.load().miso_align_plan_bytes(1) == one


# ---- align/vfpp.py on the CPU -------------------------------------------------------------------------------------------
def _two_kf_atlas(monkeypatch):
    import oracle_backend
    from test_grid_opt_mirror import _OneBatch, make_atlas_two_kf
    oracle_backend.install(monkeypatch)
    mi, gt = gc.atlas_sdf_batch()
    return make_atlas_two_kf("cpu"), _OneBatch(mi, gt), mi, gt


def _vfpp64(src, dst, mi, gt, dr, dt, trunc, weight):
    """pairwise_loss_vfpp in float64 on oracle.ref_torch: dr / dt: per-submap pose corrections (leaves)."""
    c = gc.ATLAS
    subs = gc.atlas_inputs()
    bound = torch.tensor(c["bound"], dtype=F64)
    ids = T(mi["sample_frame_ids"][0, :, 0])
    rows = torch.nonzero(ids // 2 == src).squeeze(1)                       # keyframes 2s, 2s + 1 belong to submap s
    R2, t2 = gc.atlas_second_kf_pose(src)
    R_kf = torch.stack([torch.eye(3, dtype=F64), T(R2).double()])
    t_kf = torch.stack([torch.zeros(3, 1, dtype=F64), T(t2).double()])
    x_src = R.transform_by_keyframe_loop(T(mi["coords_frame"][0]).double()[rows], ids[rows] - 2 * src, R_kf, t_kf)
    pose = lambda s: R.apply_pose_correction(T(subs[s]["R"]).double(), T(subs[s]["t"]).double().view(3, 1), dr[s], dt[s])
    x_dst = R.transfrom_points_from(R.transform_points_to(x_src, *pose(src)), *pose(dst))
    sdf = T(gt["sdf"][0]).double()[rows]
    mask = (sdf.abs() < trunc) & R.coords_in_bound(x_dst, bound)
    ws, bs = R.decoder_params({k: T(v).double() for k, v in gc.make_decoder(c).items()})
    pred = R.sdf_stock([T(f).double() for f in subs[dst]["features"]], bound, x_dst, ws, bs)
    return weight * torch.mean(torch.where(mask, pred - sdf, torch.zeros_like(pred)) ** 2)


def test_pairwise_loss_vfpp_matches_a_float64_restatement(monkeypatch):
    from test_grid_opt_mirror import close
    import miso_amd.grid_opt.align.vfpp as VF
    atlas, ds, mi, gt = _two_kf_atlas(monkeypatch)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)
    subs = gc.atlas_inputs()
    for (a, b) in [(0, 1), (1, 2), (2, 0)]:
        atlas.zero_grad(set_to_none=True)
        d = VF.pairwise_loss_vfpp(atlas, loader, a, b, device="cpu")
        assert list(d) == [f"vfpp_{a}_{b}"]
        (val,) = d.values()
        val.backward()
        dr = [T(s["dr"]).double().reshape(1, 3).requires_grad_(True) for s in subs]
        dt = [T(s["dt"]).double().reshape(3, 1).requires_grad_(True) for s in subs]
        want = _vfpp64(a, b, mi, gt, dr, dt, trunc=0.15, weight=3000)      # the reference's defaults
        want.backward()
        assert want.item() > 0
        assert abs(val.item() - want.item()) <= 3e-5 * abs(want.item()), (a, b, val.item(), want.item())
        for s in (a, b):
            close(atlas.rotation_corrections[s].grad.double(), dr[s].grad.reshape(atlas.rotation_corrections[s].shape), 2e-3, 2e-3)
            close(atlas.translation_corrections[s].grad.double(), dt[s].grad.reshape(atlas.translation_corrections[s].shape), 2e-3, 2e-3)


def test_vfpp_signatures_follow_the_reference():
    import inspect
    import miso_amd.compat  # noqa: F401
    import grid_opt.align.vfpp as alias
    import miso_amd.grid_opt.align.vfpp as VF
    assert alias is VF
    sig = inspect.signature(VF.align_multiple_submaps_vfpp).parameters
    assert sig["sdf_weight"].default == 3000 and sig["num_iters"].default == 10 and sig["lr"].default == 1e-2
    assert sig["dataset_name"].default == "SubmapSdf3D" and sig["use_bound"].default is True
    sig = inspect.signature(VF.pairwise_loss_vfpp).parameters
    assert sig["sdf_weight"].default == 3000 and sig["trunc_dist"].default == 0.15
    assert list(inspect.signature(VF.align_submap_pair_vfpp).parameters)[:5] == \
        ["grid_atlas", "dataset", "src_id", "dst_id", "dataset_name"]


def test_fused_finetune_falls_back_on_the_cpu(monkeypatch, caplog):
    """finetune_fused=True with the atlas on the CPU: the op-by-op loop, the same corrections as finetune_fused=False
    under one seed, and a log line that says why."""
    import miso_amd.grid_opt.align.miso as AM
    out = []
    for fused in (False, True):
        atlas, ds, _, _ = _two_kf_atlas(monkeypatch)
        torch.manual_seed(3)
        np.random.seed(3)
        with caplog.at_level(logging.INFO, logger=AM.logger.name):
            caplog.clear()
            info = AM.align_multiple_submaps_hierarchical(atlas, ds, level_iters=1, finetune_iters=2, latent_levels=[0],
                                                          device="cpu", verbose=False, save_iterations=True,
                                                          finetune_fused=fused)
        assert sorted(info["hier_sdf_L2"]) == ["cpu_time_sec", "gpu_time_sec", "iteration_results"]
        assert sorted(info["hier_sdf_L2"]["iteration_results"]) == [0, 1, 2]
        said = [r.getMessage() for r in caplog.records if "op by op" in r.getMessage()]
        assert bool(said) == fused and all("not on the GPU" in m for m in said)
        out.append(torch.cat([torch.cat([p.detach().reshape(-1) for p in atlas.rotation_corrections]),
                              torch.cat([p.detach().reshape(-1) for p in atlas.translation_corrections])]))
    assert torch.equal(out[0], out[1])
    assert (out[0] != 0).any()


# ---- the oracle of the pair stage and its bar -----------------------------------------------------------------------------
def _sums(c, loss, **kw):
    return pc.pair_sdf_sums64(c["p"], c["ref"], c["feats"], pc.BOUND, c["pose"], c["ws"], c["bs"], loss, **kw)


@pytest.mark.parametrize("grid", sorted(pc.GRIDS))
def test_row_lists_are_what_the_gpu_tests_need(grid):
    for n in (2049, 130, 0):
        c = pc.case(grid, n)
        assert c["p"].shape == (n, 3) and c["p"].dtype == F32 and c["ref"].shape == (n,)
        sums, _ = _sums(c, "L2")
        if n:
            assert 0.2 * n < n - sums[1] < 0.45 * n, (n, sums[1])          # about a third of the rows out of bound
        else:
            assert not sums.any()


@pytest.mark.parametrize("loss", ["L2", "L1", "GM"])
@pytest.mark.parametrize("grid", sorted(pc.GRIDS))
def test_the_sdf_pair_bar_sees_what_it_must(grid, loss):
    c = pc.case(grid, 2049)
    sums, A = _sums(c, loss)
    n = c["p"].shape[0]
    sums_only = lambda ex: ex[[0] + list(range(2, 23))]
    # the oracle's own fp32 evaluation at the same coordinates passes
    s32, _ = _sums(c, loss, dtype=F32)
    ex = pc.excess(s32, sums, A)
    assert (ex <= 0).all(), ex
    # ... on the short list too
    c130 = pc.case(grid, 130)
    ex = pc.excess(_sums(c130, loss, dtype=F32)[0], *_sums(c130, loss))
    assert (ex <= 0).all(), ex
    # one in-bound row dropped (the count patched back: the sums alone must see it)
    _, _, m = R.src_to_dst32(c["p"], c["pose"][:9], c["pose"][9:12], c["pose"][12:21], c["pose"][21:24], pc.BOUND)
    k = int(torch.nonzero(m)[len(torch.nonzero(m)) // 2])
    keep = torch.arange(n) != k
    drop, _ = pc.pair_sdf_sums64(c["p"][keep], c["ref"][keep], c["feats"], pc.BOUND, c["pose"], c["ws"], c["bs"], loss)
    assert drop[1] == sums[1] - 1
    drop[1] = sums[1]
    assert (sums_only(pc.excess(drop, sums, A)) > 0).any()
    # the count off by one
    one = sums.clone()
    one[1] += 1
    assert pc.excess(one, sums, A)[1] > 0
    # the sign of g flipped on 1 % of the rows
    sign = torch.ones(n)
    sign[torch.nonzero(m).flatten()[::100]] = -1.0
    flip, _ = _sums(c, loss, g_sign=sign)
    assert torch.equal(flip[:2], sums[:2])
    assert (sums_only(pc.excess(flip, sums, A)) > 0).any()
    # ref shifted by one row
    shifted, _ = pc.pair_sdf_sums64(c["p"], torch.roll(c["ref"], 1), c["feats"], pc.BOUND, c["pose"], c["ws"], c["bs"], loss)
    assert (sums_only(pc.excess(shifted, sums, A)) > 0).any()
