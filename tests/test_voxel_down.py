"""Voxel down-sampling as a HIP operator (csrc/voxel.hip: miso_voxel_down_sample / miso_voxel_select_rows) against what the
reference's utils_geometry.voxel_down_sample_torch selects on the CPU (tests/golden/voxel_down.npz, written by
tools/make_voxel_goldens.py on the clouds of tests/voxel_cases.py).  Every comparison is equality of index arrays or of
gathered rows: no tolerance anywhere, except where three trainer steps are compared (see test_capture)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import golden_cases as gc
import voxel_cases as vc

DEV = "cuda:0"
BADARG, TOOLARGE = 2001, 2003
CASES = ["room_005", "room_001", "clustered", "lattice", "alias", "one_voxel", "single"]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def clouds():
    return vc.cases()


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(gc.golden_path("voxel_down")))


def mirror_cpu(points: torch.Tensor, v: float) -> torch.Tensor:
    from miso_amd.grid_opt.utils.utils_geometry import voxel_down_sample_torch
    assert not points.is_cuda
    return voxel_down_sample_torch(points, v)


# --------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", CASES)
def test_cpu_mirror_equals_reference(name):
    """The torch mirror on the CPU (already pinned by geometry.npz) reproduces the new fixture: the fixture is the
    reference's, and the mirror may serve as the expected value for shapes the fixture does not hold."""
    pts, v = clouds()[name]
    got = mirror_cpu(T(pts), v)
    assert got.dtype == torch.int64 and torch.equal(got, T(golden()[f"idx_{name}"]))


def test_fixture_pins_the_two_reference_quirks():
    """What the fixture is for: the merge regime (fewer indices than occupied voxels once keys pass 2^24) and the
    ix == side alias are in it."""
    for name in ("room_001", "alias", "lattice"):
        pts, v = clouds()[name]
        cell = np.floor(pts.astype(np.float64) / np.float64(np.float32(v))).astype(np.int64)
        occupied = np.unique(cell, axis=0).shape[0]
        assert golden()[f"idx_{name}"].shape[0] < occupied, name
    pts, v = clouds()["room_001"]
    side = np.floor((pts.max(0) - pts.min(0)) / v).max()
    assert side ** 3 > 2 ** 24


def test_library_exports_the_voxel_entry_points():
    from miso_amd import _lib
    lib = _lib.load()
    for name in ("miso_voxel_down_workspace_bytes", "miso_voxel_down_sample", "miso_voxel_select_rows"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["miso_voxel_down_sample"][1]) == 9
    assert len(_lib.SIGNATURES["miso_voxel_select_rows"][1]) == 11


def test_voxel_entry_points_validate_arguments_without_gpu():
    """Malformed calls are refused before any launch (the pointers below are host arrays that a launch must never see)."""
    from miso_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()                     # 16-byte aligned stand-in for every pointer
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert ctypes.addressof(buf) % 16 == 0
    down = lib.miso_voxel_down_sample
    assert down(None, 3, 8, None, 0.05, p, p, p, None) == BADARG            # points
    assert down(p, 3, 8, None, 0.05, None, p, p, None) == BADARG            # workspace
    assert down(p, 3, 8, None, 0.05, p, None, p, None) == BADARG            # out_idx
    assert down(p, 3, 8, None, 0.05, p, p, None, None) == BADARG            # out_count
    assert down(p, 3, -1, None, 0.05, p, p, p, None) == BADARG
    assert down(p, 2, 8, None, 0.05, p, p, p, None) == BADARG               # ld < 3
    for bad in (0.0, -0.05, float("inf"), float("nan")):
        assert down(p, 3, 8, None, bad, p, p, p, None) == BADARG, bad
    assert down(p, 3, 1 << 22, None, 0.05, p, p, p, None) == TOOLARGE       # the 22-bit index field
    assert lib.miso_voxel_down_workspace_bytes(1 << 22) == 0 and lib.miso_voxel_down_workspace_bytes(-1) == 0
    assert lib.miso_voxel_down_workspace_bytes((1 << 22) - 1) >= 2 * 8 * ((1 << 22) - 1)
    assert lib.miso_voxel_down_workspace_bytes(5000) >= lib.miso_voxel_down_workspace_bytes(4096) > 2 * 8 * 4096
    rows = lib.miso_voxel_select_rows
    assert rows(None, None, None, None, None, 8, None, None, None, None, None) == BADARG
    assert rows(p, p, p, p, p, -1, p, p, p, p, None) == BADARG
    assert rows(p, p, p, p, p, 1 << 22, p, p, p, p, None) == TOOLARGE
    assert rows(p, p, p, p, p, 8, p, p, p, p, None) == BADARG               # source and destination overlap
    q = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    assert rows(p, p, q, p, p, 8, p, p, p, p, None) == BADARG               # aux not 16-byte aligned


def test_ops_refuse_cpu_clouds():
    from miso_amd import ops
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.voxel_down_sample(torch.rand(10, 3), 0.1)


# --------------------------------------------------------------------------- GPU
def selection(points_dev, v, **kw):
    from miso_amd import ops
    idx, count = ops.voxel_down_sample(points_dev, v, **kw)
    m = int(count.item())
    assert idx.dtype == torch.int64 and idx.shape[0] >= points_dev.shape[0] and bool((idx[m:points_dev.shape[0]] == -1).all())
    return idx[:m].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_operator_equals_reference(name):
    from miso_amd.grid_opt.utils.utils_geometry import voxel_down_sample_torch
    pts, v = clouds()[name]
    want = T(golden()[f"idx_{name}"])
    x = T(pts).to(DEV)
    got = selection(x, v)
    print(name, "selected", got.shape[0], "of", pts.shape[0], "reference", want.shape[0])
    assert torch.equal(got, want)
    via = voxel_down_sample_torch(x, v)
    assert via.is_cuda and torch.equal(via.cpu(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n,v", [(n, 0.05) for n in (1, 63, 64, 65, 1023, 1024, 1025, 4097, 65537)]
                         + [(1025, 0.01), (65537, 0.01)])
def test_boundary_sizes(n, v):
    """Prefixes of the room cloud at the sizes where a wavefront (64), a workgroup (1024), a radix tile (4096) and the
    tile count (> 16 tiles) change; expected: the CPU mirror, run here."""
    pts = T(clouds()["room_005"][0][:n].copy())
    assert torch.equal(selection(pts.to(DEV), v), mirror_cpu(pts, v))


@pytest.mark.gpu
def test_row_stride_and_empty_cloud():
    """A (N, 4)-strided view is read in place through ld; an empty cloud gives count 0."""
    from miso_amd import ops
    pts = T(clouds()["clustered"][0][:3001].copy())
    wide = torch.full((3001, 4), float("nan"), device=DEV)
    wide[:, :3] = pts.to(DEV)
    assert torch.equal(selection(wide[:, :3], 0.1), mirror_cpu(pts, 0.1))
    idx, count = ops.voxel_down_sample(torch.zeros(0, 3, device=DEV), 0.1)
    assert idx.numel() == 0 and int(count.item()) == 0


@pytest.mark.gpu
def test_device_live_count():
    """Capacity 4096 with 3000 live rows counted on the device: the rows behind them (NaN, 1e30) are never read."""
    from miso_amd import ops
    pts = T(clouds()["room_005"][0][:4096].copy())
    x = pts.to(DEV).clone()
    x[3000:3500] = float("nan")
    x[3500:] = 1e30
    live = torch.tensor([3000], dtype=torch.int32, device=DEV)
    idx, count = ops.voxel_down_sample(x, 0.05, n_live=live)
    m = int(count.item())
    want = mirror_cpu(pts[:3000], 0.05)
    assert torch.equal(idx[:m].cpu(), want) and bool((idx[m:] == -1).all())
    assert torch.equal(want, selection(pts[:3000].to(DEV), 0.05))
    live.zero_()
    idx, count = ops.voxel_down_sample(x, 0.05, n_live=live)
    assert int(count.item()) == 0 and bool((idx == -1).all())


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    from miso_amd import ops
    for name in ("room_001", "clustered"):
        pts, v = clouds()[name]
        x = T(pts).to(DEV)
        a = [t.clone() for t in ops.voxel_down_sample(x, v)]
        b = ops.voxel_down_sample(x, v)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _rgbd(voxel_size=None, padded=False):
    from miso_amd.grid_opt.datasets.sdf_rgbd import PosedSdfRgbd
    from miso_amd.grid_opt.utils.utils_data import CameraParameters
    c, inp = gc.RGBD, gc.rgbd_inputs()
    cam = CameraParameters(fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], H=c["H"], W=c["W"])
    return PosedSdfRgbd.from_frames(T(inp["depth"]), T(inp["R"]), T(inp["t"]), cam, n_rays=c["n_rays"],
                                    min_depth=c["min_depth"], dist_behind_surf=c["dist_behind_surf"],
                                    n_strat_samples=c["n_strat"], n_surf_samples=c["n_surf"], trunc_dist=c["trunc_dist"],
                                    device=DEV, normals=T(inp["normals"]), voxel_size=voxel_size, padded=padded)


def _rgbd_draws():
    c, g = gc.RGBD, np.load(gc.golden_path("samples"))
    total, n1 = c["n_frames"] * c["n_rays"], g["rgbd_all_u"].shape[0]
    u = torch.zeros(total, c["n_strat"])
    u[:n1] = T(g["rgbd_all_u"])
    gg = torch.zeros(total, c["n_surf"] - 1)
    gg[:n1] = T(g["rgbd_all_g"])
    return T(g["rgbd_all_pix_h"]).to(DEV), T(g["rgbd_all_pix_w"]).to(DEV), u.to(DEV), gg.to(DEV)


@pytest.mark.gpu
def test_rgbd_rows_contract():
    """PosedSdfRgbd(voxel_size=0.05) on the golden RGB-D case with fixed draws: the exact-size dictionaries are the
    sampler's indexed by the CPU mirror's selection of its coords_frame; the padded batch holds the same rows in front,
    neutral rows behind them and the count on the device."""
    draws, v = _rgbd_draws(), 0.05
    base_in, base_gt = _rgbd().getitem_sdf(0, draws=draws)
    sel = mirror_cpu(base_in["coords_frame"].cpu(), v)
    m, n = sel.shape[0], base_in["coords_frame"].shape[0]
    print("rows", n, "selected", m)
    assert 0 < m < n
    want = {k: t.cpu()[sel] for k, t in {**base_in, **base_gt}.items()}
    got_in, got_gt = _rgbd(voxel_size=v).getitem_sdf(0, draws=draws)
    got = {**got_in, **got_gt}
    assert set(got) == set(want) == {"coords_frame", "sample_frame_ids", "weights", "sdf", "sdf_valid", "sdf_signs"}
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k].cpu(), want[k]), k
    pad_in, pad_gt = _rgbd(voxel_size=v, padded=True).getitem_sdf(0, draws=draws)
    cap = gc.RGBD["n_frames"] * gc.RGBD["n_rays"] * (gc.RGBD["n_strat"] + gc.RGBD["n_surf"])
    assert pad_in["live_rows"].dtype == torch.int32 and pad_in["live_rows"].is_cuda and int(pad_in["live_rows"]) == m
    pad = {**{k: t for k, t in pad_in.items() if k != "live_rows"}, **pad_gt}
    for k in want:
        assert pad[k].shape[0] == cap and torch.equal(pad[k][:m].cpu(), want[k]), k
        assert not bool(pad[k][m:].cpu().to(torch.float32).any()), k          # coordinates 0, id 0, valid = sign = weight = 0


@pytest.mark.gpu
def test_capture(tmp_path):
    """A padded, voxel-down-sampled dataset feeds the captured trainer step: three steps with captured_step on give the
    losses of three steps with it off under the same seed.  The two paths are different kernels (one fused launch against
    op-by-op autograd); tests/test_datasets.py::test_padded_batches_feed_one_captured_step bounds their loss difference
    on one batch by 1e-5 relative, and the same bound is used here for each of the three steps."""
    from miso_amd.grid_opt.datasets.sdf_rgbd import PosedSdfRgbd
    from miso_amd.grid_opt.loss import MisoLossMapping
    from miso_amd.grid_opt.models.grid_net import GridNet
    from miso_amd.grid_opt.trainer import GridTrainer
    from miso_amd.grid_opt.utils.utils_data import CameraParameters
    H, W, rays = 48, 64, 700
    cp = CameraParameters(fx=50.0, fy=50.0, cx=31.5, cy=23.5, H=H, W=W)
    g = torch.Generator().manual_seed(4)
    depth = 1.5 + torch.rand(3, H, W, generator=g)
    depth[torch.rand(3, H, W, generator=g) < 0.3] = 0.0
    R = torch.eye(3).repeat(3, 1, 1)
    t = torch.tensor([[[0.0], [0.0], [0.0]], [[0.3], [0.1], [0.0]], [[-0.2], [0.0], [0.1]]])
    ds = PosedSdfRgbd.from_frames(depth, R, t, cp, n_rays=rays, n_strat_samples=5, n_surf_samples=4, trunc_dist=0.15,
                                  device=DEV, padded=True, voxel_size=0.05)
    cfg_model = gc.model_cfg([[-3.0, 3.0], [-2.5, 2.5], [-0.5, 3.5]], 0.5, 4, 2, 4, 32, num_poses=3, init_stddev=1e-2)
    lf = MisoLossMapping(loss_type="L1", weight_sdf=1.0, weight_eik=0.0, weight_fs=0.5, trunc_dist=0.15)
    losses, counts = {}, {}
    for captured in (True, False):
        torch.manual_seed(0)
        net = GridNet(cfg_model, device=DEV).to(DEV)
        for k in range(3):
            net.set_initial_kf_pose(k, R[k], t[k], kf_key=f"KF{k}")
        net.unlock_feature()
        net.lock_pose()
        cfg_train = {"verbose": False, "optimizer": "adam", "learning_rate": 1e-3, "epochs": 3, "ckpt_every": -1,
                     "eval_every": -1, "eval_metric": None, "pretrained_model": None, "log_dir": str(tmp_path),
                     "relchange_tol": 0, "max_epochs_in_level": 100, "grid_training_mode": "joint",
                     "captured_step": captured}
        loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)
        tr = GridTrainer(cfg_train, net, lf, loader, None, DEV, torch.float32)
        seen, live = [], []
        step = tr.train_step

        def spy(model_input, gt, _raw=False, _step=step, _seen=seen, _live=live):
            _live.append(model_input["live_rows"].reshape(-1)[0].clone())
            total = _step(model_input, gt, _raw=_raw)
            _seen.append(total.detach().reshape(()).clone())
            return total

        tr.train_step = spy
        torch.manual_seed(9)                                     # the dataset's draws
        tr.train()
        assert bool(tr.__dict__.get("_mapping_steps")) == captured
        losses[captured] = [float(v) for v in seen]
        counts[captured] = [int(v) for v in live]
    print("captured", losses[True], "eager", losses[False], "live rows", counts[True])
    assert len(losses[True]) == 3 and counts[True] == counts[False]
    assert all(0 < c < 3 * rays * 9 for c in counts[True]) and len(set(counts[True])) > 1
    for a, b in zip(losses[True], losses[False]):
        assert a > 0 and abs(a - b) <= 1e-5 * abs(b), (losses[True], losses[False])


def _lidar(device, **kw):
    from miso_amd.grid_opt.datasets.sdf_3d_lidar import PosedSdf3DLidar
    c = vc.LIDAR
    frames = vc.lidar_frames()
    poses = np.tile(np.eye(4), (len(frames), 1, 1))
    poses[1, :3, 3] = [1.0, -2.0, 0.5]
    ds = PosedSdf3DLidar.from_frames(frames, poses, frame_samples=64, frame_batchsize=64, min_z=c["min_z"],
                                     max_z=c["max_z"], min_range=c["min_range"], max_range=c["max_range"], device=device,
                                     generator=torch.Generator(device=device).manual_seed(1), **kw)
    return ds, frames


@pytest.mark.gpu
def test_lidar_frames_are_down_sampled_like_the_reference():
    from miso_amd.grid_opt.datasets.sdf_3d_lidar import crop_points
    ds, frames = _lidar(DEV, voxel_size=vc.LIDAR["voxel_size"], adaptive_range=True)
    for f, pts in enumerate(frames):
        kept = golden()[f"lidar_kept_{f}"]
        assert 0 < kept.shape[0] < pts.shape[0]
        assert torch.equal(ds.frames_lidar[f]["points_local"], T(pts[kept])), f
    plain, _ = _lidar(DEV)                                       # the defaults: frames as before, cropped only
    c = vc.LIDAR
    for f, pts in enumerate(frames):
        want, _ = crop_points(T(pts), None, c["min_z"], c["max_z"], c["min_range"], c["max_range"])
        assert torch.equal(plain.frames_lidar[f]["points_local"], want)
    assert plain.voxel_size is None and not plain.adaptive_range


def test_lidar_cpu_dataset_takes_the_mirror():
    """On the CPU device the same sequence runs through the torch mirror (the reference's own host path)."""
    ds, frames = _lidar("cpu", voxel_size=vc.LIDAR["voxel_size"], adaptive_range=True)
    for f, pts in enumerate(frames):
        assert torch.equal(ds.frames_lidar[f]["points_local"], T(pts[golden()[f"lidar_kept_{f}"]])), f
