"""Ray casting against a mesh, the host side (no GPU): the fixtures and oracle of tests/mesh_cases.py, the host plan, the
grid route restated in numpy fp32 (with and without its rounding slack), utils_geometry.cast_rays_torch,
utils_sample.pinhole_rays_lookat, utils_sdf.render_mesh_depth on the CPU, PosedSdf3D on the CPU, and the refusals of the
new entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mesh_cases as mc

BADARG, TOOLARGE = 2001, 2003
CAP = 1 << 24


# --------------------------------------------------------------------------- 1. oracle and fp32 restatement
@pytest.mark.parametrize("name", list(mc.FIXTURES))
def test_fixture_keeps_its_rays_and_fp32_restatement_agrees(name):
    """By the oracle alone: at most 1 % of a fixture's rays are ill-conditioned.  On the others the numpy fp32 restatement
    of the formula picks the float64 triangle and its t is within FP32_E_MAX (the figure T_TOL is four times of);
    `lattice` is exact, ties to the lowest index included."""
    fx = mc.fixture(name)
    kept = fx["kept"]
    assert 1.0 - kept.mean() <= mc.KEPT_CAP, (name, 1.0 - kept.mean())
    got = mc.cast_fp32(fx["origins"], fx["dirs"], fx["vertices"], fx["triangles"])
    ref = fx["ref"]
    assert (got["tri"][kept] == ref["tri"][kept]).all()
    e = mc.t_error(fx, got["t"])[kept & (ref["tri"] >= 0)]
    assert np.nanmax(e, initial=0.0) <= mc.FP32_E_MAX, (name, np.nanmax(e))
    if name == "lattice":
        assert (got["t"].astype(np.float64) == ref["t"]).all() and (got["tri"] == ref["tri"]).all()
        tied = 0
        for sl, t, u, v, det, inside, _ in mc._all_triangles(fx["origins"], fx["dirs"], fx["vertices"], fx["triangles"], np.float64):
            hits = inside & (t >= 0) & (t == ref["t"][sl, None])
            tied += int((hits.sum(axis=1) > 1).sum())
            first = np.where(hits.any(axis=1), hits.argmax(axis=1), -1)
            assert (first == ref["tri"][sl]).all()
        assert tied > 100            # rays through shared edges and vertices are in the fixture
    if name == "open":
        assert 0.35 < (ref["tri"] < 0).mean() < 0.65
    if name == "sliver":
        ok = mc.hittable(fx["vertices"], fx["triangles"])
        assert (~ok).sum() == 4 and not np.isin(ref["tri"], np.nonzero(~ok)[0]).any()
        dup = np.arange(501, 521)                              # the copies of triangles 1 .. 20 never win
        assert not np.isin(ref["tri"], dup).any() and np.isin(ref["tri"], dup - 500).any()


# --------------------------------------------------------------------------- 2. the plan
def _plan(lo, hi, cell, n_tri):
    from miso_amd import _lib
    p = _lib.MeshPlan()
    rc = _lib.load().miso_mesh_plan((ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi), cell, n_tri, ctypes.byref(p))
    return rc, p


def test_plan_dims_doubling_and_last_cell():
    f = np.float32
    rc, p = _plan((0, 0, 0), (8, 6, 3), 0.25, 12)
    assert rc == 0 and list(p.dims) == [33, 25, 13] and p.cells == 33 * 25 * 13 and p.n_tri == 12
    assert p.coord_mag >= 8 + 8.25 and p.widen == pytest.approx(p.coord_mag * 2.0 ** -17)
    # the cell cap: 1 mm over 8 x 6 x 3 m would be 1.4e11 cells; doubled until the table fits
    rc, p = _plan((0, 0, 0), (8, 6, 3), 1e-3, 12)
    assert rc == 0 and p.cells <= CAP and p.cells * 8 > CAP
    assert math.log2(p.cell / f(1e-3)) == round(math.log2(p.cell / f(1e-3))) and p.cell >= 0.016
    # the largest vertex lands in the last cell, in the kernels' arithmetic, at awkward bounds
    rng = np.random.default_rng(0)
    for _ in range(200):
        lo = rng.uniform(-100, 100, 3).astype(f)
        hi = (lo + rng.uniform(0, 50, 3).astype(f)).astype(f)
        cell = float(f(rng.uniform(0.01, 3.0)))
        rc, p = _plan(lo, hi, cell, 5)
        assert rc == 0
        for a in range(3):
            c = np.floor(f(f(hi[a] - f(p.bound_min[a])) / f(p.cell)))
            assert int(c) == p.dims[a] - 1
    assert _plan((0, 0, 0), (1, 1, 1), 0.0, 5)[0] == BADARG
    assert _plan((0, 0, 0), (1, 1, 1), float("nan"), 5)[0] == BADARG
    assert _plan((0, 0, 0), (1, -1, 1), 0.1, 5)[0] == BADARG
    assert _plan((0, 0, 0), (float("inf"), 1, 1), 0.1, 5)[0] == BADARG
    assert _plan((0, 0, 0), (1, 1, 1), 0.1, -1)[0] == BADARG
    assert _plan((0, 0, 0), (1, 1, 1), 0.1, 1 << 31)[0] == TOOLARGE
    rc, p = _plan((0, 0, 0), (0, 0, 0), 0.1, 0)                # the empty mesh
    assert rc == 0 and p.cells == 1 and p.n_tri == 0


def test_plan_doubles_the_cell_at_the_entry_cap():
    """ops.mesh_plan_fit: while the counted list entries exceed the cap, the cell doubles and the count runs again."""
    from miso_amd import ops
    seen = []

    def count(plan):
        seen.append(float(plan.cell))
        return int(1000 / plan.cell ** 2), "ws%d" % len(seen)          # entries fall with the square of the cell

    plan, entries, ws = ops.mesh_plan_fit((0, 0, 0), (8, 6, 3), 0.1, 12, count, max_entries=10000)
    assert seen == pytest.approx([0.1, 0.2, 0.4]) and plan.cell == pytest.approx(0.4) and entries == 6249 and ws == "ws3"
    plan, entries, ws = ops.mesh_plan_fit((0, 0, 0), (0, 0, 0), 0.1, 0, count)
    assert entries == 0 and ws is None and len(seen) == 3
    assert ops.MESH_MAX_ENTRIES == 1 << 27


# --------------------------------------------------------------------------- 3. the stop rule and its slack
def test_walk_restated_in_fp32_needs_its_slack():
    """The grid route restated on the CPU (mc.walk_fp32: lists, clip, start cell, per-step boundaries, stop rule, every
    operation in numpy fp32 as csrc/mesh.hip orders them).  With the slack w of the plan every ray of `lattice` and
    `straddle` gets the all-triangles answer, bit for bit, at both cell sizes.  The bare rule (w = 0: lists from the
    unwidened boxes, clip to the unwidened grid) loses winners on `lattice`: rays through cell edges and corners, such as
    (1.75, 1.25, 0.75) + t (-1, 1, 1), which meets the inner wall y = 2 on its border x = 1 at t = 0.75.  Only cell (1, 2, .)
    lists that quad there; the walk leaves (1, 1, .) through the edge, steps x first and then y, and passes around it."""
    lost_bare = 0
    for name, rays in (("lattice", slice(None)), ("straddle", slice(0, 768))):
        fx = mc.fixture(name)
        for cell in fx["cells"]:
            plan = mc.mesh_plan(fx["vertices"], fx["triangles"], cell)
            for slack in (True, False):
                t, tri, ta, ia = mc.walk_fp32(fx["vertices"], fx["triangles"], fx["origins"][rays], fx["dirs"][rays], plan, slack)
                bad = int(((t.view(np.int32) != ta.view(np.int32)) | (tri != ia)).sum())
                if slack:
                    assert bad == 0, (name, cell)
                    assert (tri == fx["ref"]["tri"][rays])[fx["kept"][rays]].all()
                elif name == "lattice":
                    lost_bare += bad
    assert lost_bare > 0


def test_bare_rule_loses_a_hit_inside_the_t_window():
    """A made case for the other half of the stop rule (t_out > t_max).  Bounds from -75.14, cell 0.37: a face k whose
    computed position F = fl(lo + fl(k cell)) lies BELOW points that fl(fl(p - lo) / cell) still puts into cell k - 1.  A
    triangle in the plane x = F + 2 ulp is then listed in cell k - 1 only; a ray coming down x from inside cell k, with
    t_max one ulp past the hit, leaves cell k at t_out > t_max and stops: the bare rule misses a hit inside [t_min,
    t_max].  With the slack the triangle is listed in cell k too."""
    f = np.float32
    lo, cell = f(-75.14), f(0.37)
    for k in range(300, 20, -1):
        F = f(lo + f(f(k) * cell))
        x = np.nextafter(np.nextafter(F, f(np.inf)), f(np.inf))
        if int(np.floor(f(f(x - lo) / cell))) == k - 1:
            break
    else:
        pytest.fail("no inconsistent face found")
    verts = np.array([[x, 1.0, 0.5], [x, 1.6, 0.5], [x, 1.3, 1.1],
                      [-75.14, -75.14, 0.0], [-75.0, -75.14, 0.0], [-75.14, -75.0, 0.2],
                      [75.0, 75.0, 3.0], [74.9, 75.0, 3.0], [75.0, 74.9, 2.8]], dtype=f)
    tris = np.arange(9).reshape(3, 3)
    o = np.array([[f(x + f(0.25)), 1.3, 0.7]], dtype=f)
    d = np.array([[-1.0, 0.0, 0.0]], dtype=f)
    t_hit = mc.cast_fp32(o, d, verts, tris)["t"][0]
    assert np.isfinite(t_hit)
    t_max = np.nextafter(f(t_hit), f(np.inf))
    plan = mc.mesh_plan(verts, tris, float(cell))
    assert plan.cell == cell and f(plan.bound_min[0]) == lo
    t, tri, ta, ia = mc.walk_fp32(verts, tris, o, d, plan, slack=False, t_max=t_max)
    assert ia[0] == 0 and ta[0] == t_hit and tri[0] == -1 and t[0] == np.inf
    t, tri, ta, ia = mc.walk_fp32(verts, tris, o, d, plan, slack=True, t_max=t_max)
    assert tri[0] == 0 and t[0] == t_hit


# --------------------------------------------------------------------------- 4. cast_rays_torch
@pytest.mark.parametrize("name", ["room", "sliver", "lattice"])
def test_cast_rays_torch_against_the_oracle(name):
    from miso_amd.grid_opt.utils.utils_geometry import cast_rays_torch
    fx = mc.fixture(name)
    T = torch.from_numpy
    ref, kept = fx["ref"], fx["kept"]
    t, tri = cast_rays_torch(T(fx["origins"]), T(fx["dirs"]), T(fx["vertices"]), T(fx["triangles"]), chunk=512)
    assert t.dtype == torch.float32 and tri.dtype == torch.int64
    t, tri = t.numpy(), tri.numpy()
    assert (tri[kept] == ref["tri"][kept]).all() and (np.isinf(t) == (tri < 0)).all()
    e = mc.t_error(fx, t)[kept & (tri >= 0)]
    assert np.nanmax(e, initial=0.0) <= mc.T_TOL
    t64, tri64 = cast_rays_torch(T(fx["origins"]).double(), T(fx["dirs"]).double(), T(fx["vertices"]).double(), T(fx["triangles"]),
                                 chunk=300)
    assert (tri64.numpy() == ref["tri"]).all()
    hit = ref["tri"] >= 0
    assert np.allclose(t64.numpy()[hit], ref["t"][hit], rtol=1e-12, atol=0) and np.isinf(t64.numpy()[~hit]).all()
    # the window hides the nearest hit; an empty mesh; zero rays
    if name == "room":
        lo = float(np.median(ref["t"]))
        tw, iw = cast_rays_torch(T(fx["origins"][:256]), T(fx["dirs"][:256]), T(fx["vertices"]), T(fx["triangles"]), t_min=lo, t_max=2 * lo)
        want = mc.oracle(fx["origins"][:256], fx["dirs"][:256], fx["vertices"], fx["triangles"], t_min=np.float32(lo), t_max=np.float32(2 * lo))
        k = kept[:256]
        assert (iw.numpy()[k] == want["tri"][k]).all() and (iw.numpy() != ref["tri"][:256]).any()
        t0, i0 = cast_rays_torch(T(fx["origins"][:5]), T(fx["dirs"][:5]), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64))
        assert torch.isinf(t0).all() and (i0 == -1).all()
        t0, i0 = cast_rays_torch(torch.zeros(0, 3), torch.zeros(0, 3), T(fx["vertices"]), T(fx["triangles"]))
        assert t0.shape == (0,) and i0.shape == (0,)


# --------------------------------------------------------------------------- 5. pinhole_rays_lookat
def test_pinhole_rays_lookat_geometry():
    from miso_amd.grid_opt.utils.utils_sample import pinhole_rays_lookat
    W, H, fov = 64, 48, 90.0
    eye, center, up = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1.0, 2.0, 2.0]), torch.tensor([0.0, 1.0, 0.0])
    rays = pinhole_rays_lookat(fov, center, eye, up, W, H)
    assert rays.shape == (H * W, 6) and rays.dtype == torch.float32
    assert (rays[:, :3] == eye).all()
    d = rays[:, 3:].reshape(H, W, 3)
    f = 0.5 * W / math.tan(math.radians(fov) / 2)
    assert f == pytest.approx(32.0)
    z = torch.tensor([0.0, 0.0, -1.0])
    x = torch.linalg.cross(up, z)
    y = torch.linalg.cross(z, x)
    assert torch.allclose(d @ z, torch.ones(H, W), atol=1e-6)                      # z-depth = ray parameter
    cols = (torch.arange(W) + 0.5 - W / 2) / f
    rows = (torch.arange(H) + 0.5 - H / 2) / f
    assert torch.allclose(d @ x, cols[None, :].expand(H, W), atol=1e-6)            # through pixel centres, row-major
    assert torch.allclose(d @ y, rows[:, None].expand(H, W), atol=1e-6)
    # the horizontal field of view is the angle between the image's left and right borders
    left, right = -0.5 * W / f, 0.5 * W / f
    assert math.degrees(math.atan(right) - math.atan(left)) == pytest.approx(fov)
    assert d.norm(dim=-1).max() > 1.2                                               # not normalised


# --------------------------------------------------------------------------- 6. render_mesh_depth on the CPU
ROOM = np.array([[0.0, 8.0], [0.0, 6.0], [0.0, 3.0]])


def _camera(H=48, W=64):
    from miso_amd.grid_opt.utils.utils_data import CameraParameters
    return CameraParameters(fx=40.0, fy=40.0, cx=31.5, cy=23.5, H=H, W=W)


def _pose(yaw_deg, pitch_deg, t):
    yaw, pitch = math.radians(yaw_deg), math.radians(pitch_deg)
    fwd = np.array([math.cos(yaw) * math.cos(pitch), math.sin(yaw) * math.cos(pitch), -math.sin(pitch)])
    right = np.cross(np.array([0.0, 0.0, -1.0]), fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.stack((right, down, fwd), axis=1), np.asarray(t, dtype=np.float64)


def _box_room_depth(R, t, cam):
    """the analytic box room of tools/demo_synthetic.py (render_depth there), restated: slab exit of every pixel's ray"""
    v, u = np.meshgrid(np.arange(cam.H), np.arange(cam.W), indexing="ij")
    d_c = np.stack(((u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy, np.ones_like(u, dtype=np.float64)), -1)
    d_w = d_c @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        hit = np.where(d_w > 0, (ROOM[:, 1] - t) / d_w, (ROOM[:, 0] - t) / d_w)
    return hit.min(axis=-1)


def test_render_mesh_depth_on_cpu_is_the_analytic_box_room():
    from miso_amd.grid_opt.utils import utils_sdf
    cam = _camera()
    mesh = utils_sdf.box_mesh(ROOM)
    for yaw, pitch, t in ((20.0, 5.0, (2.0, 2.5, 1.4)), (200.0, -10.0, (6.0, 3.0, 1.0))):
        R, tt = _pose(yaw, pitch, t)
        want = _box_room_depth(R, tt, cam)
        depth, mask, nrm = utils_sdf.render_mesh_depth(mesh, torch.tensor(R, dtype=torch.float32), torch.tensor(tt, dtype=torch.float32),
                                                       cam, normals=True)
        assert depth.shape == (cam.H, cam.W) and mask.dtype == torch.bool and nrm.shape == (cam.H, cam.W, 3)
        got = depth.numpy().astype(np.float64)
        # a pixel whose ray passes within 1e-4 of a room edge may fall between two wall triangles: at most a handful
        assert mask.float().mean() > 0.995
        m = mask.numpy()
        assert np.abs(got - want)[m].max() <= mc.T_TOL * (8.0 + want.max() * 1.5)
        n = nrm.numpy()[m]
        assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5) and (np.abs(n).max(axis=1) > 0.999).all()   # axis-aligned walls
    short, mask = utils_sdf.render_mesh_depth(mesh, torch.tensor(R, dtype=torch.float32), torch.tensor(tt, dtype=torch.float32), cam,
                                              max_dist=3.0)
    far = want * np.linalg.norm(np.stack(((np.arange(cam.W)[None, :] - cam.cx) / cam.fx + 0 * want,
                                          (np.arange(cam.H)[:, None] - cam.cy) / cam.fy + 0 * want, np.ones_like(want)), -1), axis=-1) > 3.0 + 1e-3
    assert (short.numpy()[far] == 0).all() and not mask.numpy()[far].any() and mask.any()


# --------------------------------------------------------------------------- 7, 8. PosedSdf3D on the CPU
def _box_distance(p):
    """distance of points inside the room to its walls"""
    return np.minimum(p - ROOM[:, 0], ROOM[:, 1] - p).min(axis=1)


def check_posed_sdf_3d(ds, n_frames, frame_samples, near_n, free_n, trunc, tol):
    """what tests 7 (CPU) and the device test share: the layout of ds.frames and of a batch"""
    per = frame_samples * (1 + near_n + free_n)
    assert len(ds.frames) == n_frames and len(ds) == per // ds.frame_batchsize
    for f, frame in enumerate(ds.frames):
        R, t = frame["R_world_frame_gt"].cpu().numpy().astype(np.float64), frame["t_world_frame_gt"].cpu().numpy().astype(np.float64)
        pts = frame["points_frame"].cpu().numpy().astype(np.float64) @ R.T + t.T
        sdf, valid, sign = (frame[k].cpu().numpy()[:, 0] for k in ("sdfs", "sdfs_valid", "signs"))
        assert pts.shape == (per, 3) and sdf.shape == (per,)
        eye = t[:, 0]
        hit, near, free = pts[:frame_samples], pts[frame_samples:frame_samples * (1 + near_n)], pts[frame_samples * (1 + near_n):]
        assert np.abs(_box_distance(hit)).max() <= tol                         # hit rows lie on the mesh
        assert (sdf[:frame_samples] == 0).all() and (valid[:frame_samples] == 1).all() and (sign[:frame_samples] == 0).all()
        d_hit = np.linalg.norm(hit - eye, axis=1)
        d_near = np.linalg.norm(near - eye, axis=1)
        lab = sdf[frame_samples:frame_samples * (1 + near_n)]
        assert np.abs((d_near - np.repeat(d_hit, near_n)) + lab).max() <= 1e-4  # label = minus the displacement along the ray
        cosang = np.einsum("ij,ij->i", near - eye, np.repeat(hit - eye, near_n, axis=0)) / (d_near * np.repeat(d_hit, near_n))
        assert cosang.min() > 1 - 1e-5
        assert (valid[frame_samples:frame_samples * (1 + near_n)] == 1).all() and (sign[frame_samples:frame_samples * (1 + near_n)] == 0).all()
        d_free = np.linalg.norm(free - eye, axis=1)
        gap = np.repeat(d_hit, free_n) - d_free
        assert gap.min() >= trunc - 1e-4 and np.abs(gap - sdf[frame_samples * (1 + near_n):]).max() <= 1e-4
        assert (sign[frame_samples * (1 + near_n):] == 1).all() and (valid[frame_samples * (1 + near_n):] == 0).all()
    inp, gt = ds[0]
    B = min(ds.frame_batchsize, per)
    assert set(inp) == {"R_world_frame", "t_world_frame", "coords_frame", "coords_world_noisy", "coords_world_gt", "frame_indices"}
    assert set(gt) == {"sdf", "sdf_valid", "sdf_signs", "R_world_frame_gt", "t_world_frame_gt"}
    assert inp["coords_frame"].shape == (n_frames * B, 3) and gt["sdf"].shape == (n_frames * B, 1)
    assert gt["sdf_valid"].shape == (n_frames * B, 1) and gt["sdf_signs"].shape == (n_frames * B, 1)
    assert inp["R_world_frame"].shape == (n_frames, 3, 3) and inp["t_world_frame"].shape == (n_frames, 3, 1)
    fi = inp["frame_indices"].cpu()
    assert fi.dtype == torch.int64 and fi.tolist() == [[f * B, (f + 1) * B] for f in range(n_frames)]
    for f in range(n_frames):
        rows = slice(f * B, (f + 1) * B)
        R, t = ds.true_kf_pose_in_world(f)
        assert torch.allclose(inp["coords_world_gt"][rows], inp["coords_frame"][rows] @ R.T + t.T, atol=1e-5)
    assert torch.equal(inp["coords_world_noisy"], inp["coords_world_gt"])       # no pose noise asked for


def posed_sdf_3d_poses():
    Rs, ts = zip(*(_pose(y, p, t) for y, p, t in ((20.0, 5.0, (2.0, 2.5, 1.4)), (200.0, -10.0, (6.0, 3.0, 1.0)), (100.0, 0.0, (4.0, 1.0, 2.0)))))
    return torch.tensor(np.stack(Rs), dtype=torch.float32), torch.tensor(np.stack(ts), dtype=torch.float32).reshape(-1, 3, 1)


def test_posed_sdf_3d_on_cpu():
    from miso_amd.grid_opt.datasets.sdf_3d import BatchPosedSdf3D, PosedSdf3D
    from miso_amd.grid_opt.utils import utils_sdf
    mesh = utils_sdf.box_mesh(ROOM)
    np.random.seed(4)
    ds = PosedSdf3D(mesh, frame_batchsize=128, frame_samples=256, near_surface_n=2, free_space_n=1, trunc_dist=0.15,
                    device="cpu", frame_poses=posed_sdf_3d_poses(), width_px=64, height_px=48)
    assert ds.num_frames == 3 and np.allclose(ds.bound, ROOM) and np.allclose(ds.get_inflated_bound(), ROOM + [-0.5, 0.5])
    check_posed_sdf_3d(ds, 3, 256, 2, 1, 0.15, tol=mc.T_TOL * 20.0)
    # sdf_fn: the camera loop of the reference runs, and hit points carry its labels
    calls = []

    def sdf_fn(p):
        calls.append(len(p))
        return _box_distance(np.asarray(p, dtype=np.float64))

    np.random.seed(5)
    ds2 = PosedSdf3D(mesh, frame_batchsize=64, frame_samples=64, num_frames=2, device="cpu", sdf_fn=sdf_fn, width_px=32, height_px=24)
    assert ds2.num_frames == 2 and calls.count(1) >= 2 and calls.count(64) == 2
    assert (_box_distance(ds2.t_world_frame_gt[:, :, 0].numpy().astype(np.float64)) > 0.3).all()
    assert ds2.frames[0]["sdfs"][:64].abs().max() < 1e-3
    both = BatchPosedSdf3D([mesh, mesh], frame_batchsize=64, frame_samples=64, device="cpu",
                           frame_poses=[posed_sdf_3d_poses()] * 2, width_px=32, height_px=24)
    inp, gt = both[0]
    assert len(both) == 2 * len(both.datasets[0]) and int(inp["dataset_index"]) in (0, 1)
    assert torch.allclose(inp["dataset_bound"], torch.tensor(ROOM + [-0.5, 0.5], dtype=torch.float32))


def test_posed_sdf_3d_names_the_missing_signed_distance():
    from miso_amd.grid_opt.datasets.sdf_3d import PosedSdf3D
    from miso_amd.grid_opt.utils import utils_sdf
    with pytest.raises(ValueError, match="signed distance"):
        PosedSdf3D(utils_sdf.box_mesh(ROOM), device="cpu")


# --------------------------------------------------------------------------- 9. refusals without a GPU
def test_mesh_entry_points_refuse_bad_arguments_without_gpu():
    from miso_amd import _lib, ops
    lib = _lib.load()
    rc, p = _plan((0, 0, 0), (8, 6, 3), 0.5, 12)
    assert rc == 0 and lib.miso_mesh_workspace_bytes(ctypes.byref(p)) >= (p.cells + 1) * 4 + 12 * 48
    assert lib.miso_mesh_workspace_bytes(ctypes.byref(p)) % 16 == 0
    bad = _lib.MeshPlan()
    assert lib.miso_mesh_workspace_bytes(ctypes.byref(bad)) == 0 and lib.miso_mesh_workspace_bytes(None) == 0
    torn = _plan((0, 0, 0), (8, 6, 3), 0.5, 12)[1]
    torn.dims[0] += 1                                            # dims no longer multiply to cells
    assert lib.miso_mesh_workspace_bytes(ctypes.byref(torn)) == 0
    P, X = ctypes.byref(p), ctypes.c_void_p(0x1000)                # X: never dereferenced, the calls are refused first
    inf = float("inf")
    assert lib.miso_mesh_plan(None, None, 0.5, 12, None) == BADARG
    assert lib.miso_mesh_count(P, None, 3, 8, None, 3, None, None, None) == BADARG
    assert lib.miso_mesh_count(P, X, 3, 8, X, 3, X, None, None) == BADARG              # no entries slot
    assert lib.miso_mesh_count(P, X, 2, 8, X, 3, X, X, None) == BADARG                 # stride
    assert lib.miso_mesh_count(P, X, 3, 8, X, 3, ctypes.c_void_p(0x1004), X, None) == BADARG   # workspace alignment
    assert lib.miso_mesh_count(ctypes.byref(torn), X, 3, 8, X, 3, X, X, None) == BADARG
    assert lib.miso_mesh_build(P, None, X, 10, None) == BADARG
    assert lib.miso_mesh_build(P, X, None, 10, None) == BADARG
    assert lib.miso_mesh_build(P, X, X, -1, None) == BADARG
    assert lib.miso_mesh_build(P, X, X, (1 << 27) + 1, None) == TOOLARGE
    assert lib.miso_mesh_cast_rays(P, X, X, 10, None, 3, X, 3, 5, 0.0, inf, X, X, None, None) == BADARG
    assert lib.miso_mesh_cast_rays(P, X, X, 10, X, 3, X, 2, 5, 0.0, inf, X, X, None, None) == BADARG
    assert lib.miso_mesh_cast_rays(P, None, X, 10, X, 3, X, 3, 5, 0.0, inf, X, X, None, None) == BADARG
    assert lib.miso_mesh_cast_rays(P, X, X, 10, X, 3, X, 3, 1 << 31, 0.0, inf, X, X, None, None) == TOOLARGE
    assert lib.miso_mesh_cast_rays(ctypes.byref(bad), X, X, 10, X, 3, X, 3, 5, 0.0, inf, X, X, None, None) == BADARG
    assert lib.miso_mesh_cast_rays_all(None, 3, 8, X, 3, 12, X, 3, X, 3, 5, 0.0, inf, X, X, None) == BADARG
    assert lib.miso_mesh_cast_rays_all(X, 3, 8, X, 3, 12, X, 3, X, 3, 5, 0.0, inf, None, X, None) == BADARG
    assert lib.miso_mesh_cast_rays_all(X, 3, 8, X, 3, -1, X, 3, X, 3, 5, 0.0, inf, X, X, None) == BADARG
    assert lib.miso_mesh_cast_rays_all(X, 3, 8, X, 3, 1 << 31, X, 3, X, 3, 5, 0.0, inf, X, X, None) == TOOLARGE
    # the operators refuse CPU tensors, as everywhere in ops
    v, t, o = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(2, 3)
    for call in (lambda: ops.MeshIndex(v, t), lambda: ops.cast_rays_all(o, o, v, t), lambda: ops.cast_rays(o, o, v, t)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    with pytest.raises(_lib.MisoError) as e:
        _lib.check(lib.miso_mesh_build(P, X, X, -1, None), "miso_mesh_build")
    assert e.value.code == BADARG and not isinstance(e.value, _lib.NotCovered)


# --------------------------------------------------------------------------- the command-line tool
def test_render_mesh_views_tool_writes_the_frames_of_its_poses(tmp_path, monkeypatch):
    """tools/render_mesh_views.py on the CPU: a PLY and two KITTI poses in, depth .npy per pose out, equal to
    render_mesh_depth with the camera the tool states."""
    import importlib.util
    import os
    import sys
    from miso_amd.grid_opt.utils import utils_geometry, utils_sdf
    from miso_amd.grid_opt.utils.utils_data import CameraParameters
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mesh = utils_sdf.box_mesh(ROOM)
    mesh.export_ply(str(tmp_path / "room.ply"))
    poses = []
    for yaw, pitch, t in ((20.0, 5.0, (2.0, 2.5, 1.4)), (200.0, -10.0, (6.0, 3.0, 1.0))):
        R, tt = _pose(yaw, pitch, t)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, tt
        poses.append(T)
    utils_geometry.write_kitti_format_poses(str(tmp_path / "poses.txt"), np.stack(poses), direct_use_filename=True)
    spec = importlib.util.spec_from_file_location("render_mesh_views", os.path.join(root, "tools", "render_mesh_views.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "views"
    monkeypatch.setattr(sys, "argv", ["render_mesh_views.py", "--mesh", str(tmp_path / "room.ply"), "--poses", str(tmp_path / "poses.txt"),
                                      "--out", str(out), "--width", "32", "--height", "24", "--device", "cpu"])
    tool.main()
    fx, fy, cx, cy, H, W = (float(v) for v in open(out / "camera.txt").read().split())
    assert (H, W) == (24, 32) and fx == pytest.approx(16.0) and (cx, cy) == (15.5, 11.5)
    cam = CameraParameters(fx=fx, fy=fy, cx=cx, cy=cy, H=int(H), W=int(W))
    again = utils_geometry.read_kitti_format_poses(str(out / "poses_kitti.txt"))
    for k, T in enumerate(poses):
        depth = np.load(out / f"depth_{k:06d}.npy")
        assert depth.shape == (24, 32) and depth.dtype == np.float32 and np.allclose(again[k], T)
        want = _box_room_depth(T[:3, :3], T[:3, 3], cam)
        hit = depth > 0
        assert hit.mean() > 0.99 and np.abs(depth - want)[hit].max() <= mc.T_TOL * (8.0 + want.max() * 1.5)
