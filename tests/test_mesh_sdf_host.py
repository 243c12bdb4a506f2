"""The mesh distance without a GPU: the float64 oracles against the numpy fp32 restatements of tests/msdf_cases.py (the
formula, the two-level shell walk and its stop test, half-open crossing counts), the torch routes of utils_geometry on the
CPU, utils_sdf.MeshSdf / mesh_signed_distance, the datasets of grid_opt/datasets/sdf_3d.py on the CPU, and the refusals
of the HIP ops."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_cases as mc
import msdf_cases as md

ROOM = np.array([[0.0, 8.0], [0.0, 6.0], [0.0, 3.0]])
FAR_SETTINGS = ((4.0, 3), (8.0, 1))            # (factor, rings): the library's, and one that sends most queries coarse


def box_signed_distance(p, bound=ROOM):
    """signed distance to the box, positive inside"""
    inside = np.minimum(p - bound[:, 0], bound[:, 1] - p).min(axis=1)
    outside = np.linalg.norm(np.maximum(np.maximum(bound[:, 0] - p, p - bound[:, 1]), 0.0), axis=1)
    return np.where(inside >= 0, inside, -outside)


def box_points(n=2000, seed=0):
    """points in and around ROOM, none within 1e-3 of its surface"""
    p = np.random.default_rng(seed).uniform(ROOM[:, 0] - 1.5, ROOM[:, 1] + 1.5, size=(n, 3)).astype(np.float32)
    return p[np.abs(box_signed_distance(p.astype(np.float64))) > 1e-3]


# --------------------------------------------------------------------------- 1. the formula
@pytest.mark.parametrize("name", list(md.FIXTURES))
def test_fp32_restatement_against_the_oracle(name):
    fx = md.fixture(name)
    got = md.closest_fp32(fx["points"], fx["vertices"], fx["triangles"])
    e, e_tri = md.d_error(fx, got["d2"], got["tri"])
    assert (fx["ref"]["tri"] >= 0).all() and (got["tri"] >= 0).all()
    assert np.nanmax(e) <= md.FP32_E_MAX and np.nanmax(e_tri) <= md.FP32_E_MAX
    assert (got["v"] >= 0).all() and (got["w"] >= 0).all() and (got["v"] + got["w"] <= 1 + 2.0 ** -23).all()
    if name == "cube":
        assert (got["d2"].astype(np.float64) == fx["ref"]["d2"]).all() and (got["tri"] == fx["ref"]["tri"]).all()
        centre = np.nonzero((fx["points"] == 2.0).all(axis=1))[0]
        assert len(centre) == 1 and got["tri"][centre[0]] == 0 and got["d2"][centre[0]] == 4.0    # six faces tie: the lowest index


def test_fp32_e_max_is_the_measured_figure():
    worst, per = md.measure_fp32_error()
    print(f"max e {worst:.3e}: {per}")
    assert 0.9 * md.FP32_E_MAX <= worst <= md.FP32_E_MAX and per["cube"] == 0.0


def test_dead_triangles_and_non_finite_queries_never_win():
    fs = md.fixture("sliver")
    dead = np.nonzero(~mc.hittable(fs["vertices"], fs["triangles"]))[0]
    got = md.closest_fp32(fs["points"], fs["vertices"], fs["triangles"])
    assert len(dead) == 4 and not np.isin(got["tri"], dead).any() and not np.isin(got["tri"], np.arange(501, 521)).any()
    q = np.array([[np.nan, 1.0, 1.0], [np.inf, 1.0, 1.0], [1.0, -np.inf, 1.0]], np.float32)
    bad = md.closest_fp32(q, fs["vertices"], fs["triangles"])
    assert np.isposinf(bad["d2"]).all() and (bad["tri"] == -1).all()


# --------------------------------------------------------------------------- 2. the shell walk
@pytest.mark.parametrize("name", list(md.FIXTURES))
def test_restated_shell_walk_returns_the_all_triangles_bits(name):
    """The lists, the shells, the stop test with its slack and the restart on the coarse index, in numpy fp32: the
    all-triangles answer bit for bit on every walking query, at two cell sizes and two (factor, rings) settings, and
    without a far set.  The bare stop test (no slack) runs beside it: it may lose, and on these fixtures it does not (the
    lists' own w covers what the test's slack covers: test_a_made_case_loses_only_without_both_slacks); it goes coarse on
    no more queries, which shows the slack acts."""
    fx = md.fixture(name)
    P = fx["points"][fx["walks"]]
    top = md.candidates(name)
    went = []
    for cell in fx["cells"]:
        plan = mc.mesh_plan(fx["vertices"], fx["triangles"], cell)
        settings = [(None, 0)] + [(mc.mesh_plan(fx["vertices"], fx["triangles"], float(plan.cell) * f), r) for f, r in FAR_SETTINGS]
        for plan_far, rings in settings:
            d2, tri, d2_all, tri_all, coarse = md.shells_fp32(fx["vertices"], fx["triangles"], P, plan, plan_far, rings, top=top)
            assert (d2.view(np.int32) == d2_all.view(np.int32)).all() and (tri == tri_all).all(), (name, cell, rings)
            went.append(int(coarse.sum()))
        bare = md.shells_fp32(fx["vertices"], fx["triangles"], P, plan, settings[2][0], settings[2][1], slack=False, top=top)
        lost = int(((bare[0].view(np.int32) != bare[2].view(np.int32)) | (bare[1] != bare[3])).sum())
        print(f"{name} cell {cell}: went coarse {went[-3:]}, the bare rule loses {lost}, goes coarse on {int(bare[4].sum())}")
        assert int(bare[4].sum()) <= went[-1]
    assert went[0] == 0 and went[2] > 0                                  # no far set; one fine shell at the small cell


def test_a_made_case_loses_only_without_both_slacks():
    """msdf_cases.made_face_case: a triangle in a plane that membership puts in cell k although the computed face of cell k
    lies ulps above it.  Lists without w and the bare stop test return the farther triangle; either slack alone -- the w
    of the lists (every index the library builds has it) or the 2^-18 (A + g) of the stop test -- returns the winner."""
    fx = md.made_face_case()
    plan = mc.mesh_plan(fx["vertices"], fx["triangles"], fx["cells"][0])
    assert fx["ulps"] >= 2 and plan.widen > 0
    got = {(w, s): md.shells_fp32(fx["vertices"], fx["triangles"], fx["points"], plan, None, 0, slack=s, widen=w)
           for w in (True, False) for s in (True, False)}
    want = md.closest_oracle(fx["points"], fx["vertices"], fx["triangles"])
    assert want["tri"][0] == 0
    for key, (d2, tri, d2_all, tri_all, _) in got.items():
        assert tri_all[0] == 0
        assert (tri[0], d2[0] == d2_all[0]) == ((1, False) if key == (False, False) else (0, True)), key


def test_far_fixture_takes_every_route():
    fx = md.fixture("far")
    assert (~fx["walks"]).sum() == fx["n_beyond"] == 5
    for cell in fx["cells"]:
        plan = mc.mesh_plan(fx["vertices"], fx["triangles"], cell)
        assert (np.abs(fx["points"][~fx["walks"]]).max(axis=1) > 4.0 * plan.coord_mag).all()      # answered from all rows
        assert (np.abs(fx["points"][fx["walks"]]).max(axis=1) <= 4.0 * plan.coord_mag).all()
    plan = mc.mesh_plan(fx["vertices"], fx["triangles"], fx["cells"][0])
    far = mc.mesh_plan(fx["vertices"], fx["triangles"], float(plan.cell) * 4.0)
    coarse = md.shells_fp32(fx["vertices"], fx["triangles"], fx["points"][fx["walks"]], plan, far, 3, top=md.candidates("far"))[4]
    assert 0 < coarse.sum() < len(coarse)                               # some stay on the fine shells, some go coarse


# --------------------------------------------------------------------------- 3. crossing counts
def test_half_open_counting_is_exact_on_lattice():
    """every ray of `lattice` (cell faces, edges, corners, from outside): the walk's count is the all-triangles count, which
    is the float64 count; counting a hit in every listed cell the walk visits (no stretch rule) is wrong on thousands"""
    fx = md.lattice()
    for cell in fx["cells"]:
        plan = mc.mesh_plan(fx["vertices"], fx["triangles"], cell)
        walk, all_ = md.count_walk_fp32(fx["vertices"], fx["triangles"], fx["origins"], fx["dirs"], plan)
        assert (walk == all_).all() and (all_ == fx["count"]).all()
        naive, _ = md.count_walk_fp32(fx["vertices"], fx["triangles"], fx["origins"], fx["dirs"], plan, half_open=False)
        assert (naive != all_).sum() > 1000
    assert fx["count"].max() >= 8                                       # a ray through a vertex counts its whole fan


@pytest.mark.parametrize("name", list(md.FIXTURES))
def test_half_open_counting_and_parity_on_the_fixtures(name):
    fx = md.fixture(name)
    inside, counts, kept = md.parity(name)
    print(f"{name}: {(~kept).mean():.4f} of the points left out, {inside.mean():.3f} inside")
    if name != "cube":                          # (cube's lattice puts its points ON faces, edges and vertices by design)
        assert (~kept).mean() <= md.KEPT_CAP
    ok = fx["walks"]
    o, d = md.parity_rays(fx["points"][ok])
    k3 = np.tile(kept[ok], 3)
    for cell in fx["cells"]:
        plan = mc.mesh_plan(fx["vertices"], fx["triangles"], cell)
        walk, all_ = md.count_walk_fp32(fx["vertices"], fx["triangles"], o, d, plan)
        assert (walk == all_).all()                                     # every ray, never filtered
        assert (all_[k3] == counts[:, ok].reshape(-1)[k3]).all()
    if name == "nested":
        assert (inside == md.nested_inside(fx["points"]))[kept].all()
    if name == "cube":                          # (a point ON a face crosses it at t = 0: its side is anybody's)
        sd = box_signed_distance(fx["points"].astype(np.float64), np.array([[0.0, 4.0]] * 3))
        assert (inside == (sd > 0))[kept & (sd != 0)].all()


def test_parity_directions_are_the_ops_constants_and_generic():
    from miso_amd import ops
    d = np.array(ops.MESH_PARITY_DIRS)
    assert (d == md.PARITY_DIRS).all() and np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 1e-15
    a = np.sort(np.abs(d), axis=1)
    assert a.min() > 0.09 and (np.diff(a, axis=1) > 0.09).all()         # off every axis plane and every face-diagonal plane
    assert np.abs(d @ d.T - np.eye(3)).max() < 0.5


# --------------------------------------------------------------------------- 4. the torch routes on the CPU
@pytest.mark.parametrize("name", ["cube", "sliver", "nested"])
def test_torch_routes_on_the_cpu(name):
    from miso_amd.grid_opt.utils import utils_geometry
    fx = md.fixture(name)
    V, T, P = (torch.from_numpy(fx[k]) for k in ("vertices", "triangles", "points"))
    d2, tri, vw = utils_geometry.closest_on_mesh_torch(P, V, T, chunk=300)
    e, e_tri = md.d_error(fx, d2.numpy(), tri.numpy())
    assert d2.dtype == torch.float32 and tri.dtype == torch.int64 and vw.shape == (len(P), 2)
    assert np.nanmax(e) <= md.D_TOL and np.nanmax(e_tri) <= md.D_TOL
    d64, t64, _ = utils_geometry.closest_on_mesh_torch(P.double(), V.double(), T)
    assert (d64.numpy() == fx["ref"]["d2"]).all() and (t64.numpy() == fx["ref"]["tri"]).all()
    o, d = md.parity_rays(fx["points"])
    inside, counts, kept = md.parity(name)
    c = utils_geometry.count_crossings_torch(torch.from_numpy(o), torch.from_numpy(d), V, T, chunk=1000).numpy()
    assert c.dtype == np.int32 and (c.reshape(3, -1) == counts)[:, kept].all()
    empty = utils_geometry.closest_on_mesh_torch(P[:5], V, T[:0])
    assert torch.isposinf(empty[0]).all() and (empty[1] == -1).all() and (empty[2] == 0).all()
    assert (utils_geometry.count_crossings_torch(P[:5], P[:5], V, T[:0]) == 0).all()


def test_torch_count_is_exact_on_lattice():
    from miso_amd.grid_opt.utils import utils_geometry
    fx = md.lattice()
    c = utils_geometry.count_crossings_torch(*(torch.from_numpy(fx[k]) for k in ("origins", "dirs", "vertices", "triangles")))
    assert (c.numpy() == fx["count"]).all()


# --------------------------------------------------------------------------- 5. MeshSdf, mesh_signed_distance
def test_mesh_sdf_on_the_cpu_is_the_analytic_box_distance_positive_inside(tmp_path):
    from miso_amd.grid_opt.utils import utils_sdf
    mesh = utils_sdf.box_mesh(ROOM)
    p = box_points()
    want = box_signed_distance(p.astype(np.float64))
    tol = md.D_TOL * (ROOM.max() + 1.5 + np.abs(want))
    f = utils_sdf.MeshSdf(mesh.vertices, mesh.triangles, device="cpu")
    got = f(p)
    assert got.dtype == np.float32 and got.shape == (len(p),)
    assert ((got > 0) == (want > 0)).all() and (want > 0).any() and (want < 0).any()        # interior positive, exterior negative
    assert (np.abs(np.abs(got) - np.abs(want)) <= tol).all()
    assert (f.contains(p) == (want > 0)).all() and f.contains(p).dtype == bool
    assert (f(p.astype(np.float64).tolist()) == got).all()                                  # anything array-like, as pysdf
    P = torch.from_numpy(p)
    assert (utils_sdf.mesh_signed_distance(mesh, P).numpy() == got).all()
    assert (utils_sdf.mesh_signed_distance(mesh, P, inside_positive=False).numpy() == -got).all()
    path = tmp_path / "box.ply"
    mesh.export_ply(str(path))
    assert (utils_sdf.mesh_signed_distance(str(path), P).numpy() == got).all()
    none = utils_sdf.TriangleMesh(np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    assert torch.isposinf(utils_sdf.mesh_signed_distance(none, P[:4])).all()


# --------------------------------------------------------------------------- 6. the datasets on the CPU
def check_posed_mesh(ds):
    """PosedSdf3D(box, sdf_fn='mesh', num_frames=2, frame_samples=64, 32 x 24 pixels): cameras inside, hit labels zero"""
    assert ds.num_frames == 2 and len(ds.frames) == 2
    assert (box_signed_distance(ds.t_world_frame_gt[:, :, 0].cpu().numpy().astype(np.float64)) > 0.3).all()
    for frame in ds.frames:
        assert frame["sdfs"][:64].abs().max() < 1e-3 and (frame["sdfs_valid"][:64] == 1).all()
    inp, gt = ds[0]
    assert gt["sdf"].shape == (2 * 64, 1) and inp["coords_frame"].shape == (2 * 64, 3)


def test_posed_sdf_3d_with_its_own_mesh_on_the_cpu():
    from miso_amd.grid_opt.datasets.sdf_3d import BatchPosedSdf3D, PosedSdf3D
    from miso_amd.grid_opt.utils import utils_sdf
    mesh = utils_sdf.box_mesh(ROOM)
    kw = dict(sdf_fn="mesh", num_frames=2, width_px=32, height_px=24, frame_samples=64, frame_batchsize=64)
    np.random.seed(5)
    ds = PosedSdf3D(mesh, device="cpu", **kw)
    check_posed_mesh(ds)
    assert isinstance(ds.sdf_fn, utils_sdf.MeshSdf)
    np.random.seed(6)
    both = BatchPosedSdf3D([mesh, mesh], device="cpu", **kw)
    assert len(both.datasets) == 2 and all(isinstance(d.sdf_fn, utils_sdf.MeshSdf) for d in both.datasets)
    check_posed_mesh(both.datasets[1])
    with pytest.raises(ValueError, match="'mesh'"):
        PosedSdf3D(mesh, device="cpu", sdf_fn="pysdf")
    with pytest.raises(ValueError, match="signed distance to a mesh"):             # nothing asked for: today's refusal
        PosedSdf3D(mesh, device="cpu")


def check_sdf_3d(ds, total, batch, trunc):
    """the layout, validity and signs of an Sdf3D of the box ROOM"""
    half = total // 2
    coords, sdf, valid, sign = (x.cpu().numpy() for x in (ds.coords, ds.sdfs, ds.sdf_valid, ds.sdf_signs))
    assert coords.shape == (total, 3) and sdf.shape == valid.shape == sign.shape == (total, 1) and len(ds) == total // batch + 1
    assert coords.dtype == np.float32 and np.allclose(ds.bound, ROOM + [-0.5, 0.5]) and np.allclose(ds.get_inflated_bound(), ds.bound)
    want = box_signed_distance(coords.astype(np.float64))
    assert (sdf[:half] == 0).all() and np.abs(want[:half]).max() < 1e-5          # the first half: on the surface, labelled 0
    tol = md.D_TOL * (ROOM.max() + 0.5 + np.abs(want))
    assert (np.abs(sdf[half:, 0] - want[half:]) <= tol[half:]).all()              # positive inside, not negated
    assert (want[half:] > 0.05).any() and (want[half:] < -0.05).any()
    assert (coords[total * 7 // 8:] >= ds.bound[:, 0] - 1e-6).all() and (coords[total * 7 // 8:] <= ds.bound[:, 1] + 1e-6).all()
    if trunc is None:
        assert (valid == 1).all() and (sign == 0).all()
    else:
        clear = np.abs(np.abs(want) - trunc) > 1e-4
        assert (valid[:, 0] == (np.abs(want) < trunc))[clear].all() and 0.5 < valid.mean() < 1.0
        assert (sign[:, 0] == np.where(want > trunc, 1.0, np.where(want < -trunc, -1.0, 0.0)))[clear].all()
        assert (sign == 1).any() and (sign == -1).any()
    inp, gt = ds[0]
    assert inp["coords"].shape == (batch, 3) and all(gt[k].shape == (batch, 1) for k in ("sdf", "sdf_valid", "sdf_sign"))


def test_sdf_3d_on_the_cpu():
    from miso_amd.grid_opt.datasets.sdf_3d import BatchedSdf3D, Sdf3D
    from miso_amd.grid_opt.utils import utils_sdf
    mesh = utils_sdf.box_mesh(ROOM)
    for trunc in (None, 0.2):
        np.random.seed(9)
        ds = Sdf3D(mesh, total_samples=2 ** 10, batch_size=128, trunc_dist=trunc, device="cpu")
        check_sdf_3d(ds, 2 ** 10, 128, trunc)
    first = ds.coords.clone()
    ds.resample()
    assert not torch.equal(first, ds.coords)
    norm = Sdf3D(mesh, total_samples=2 ** 8, batch_size=32, normalize=True, device="cpu")
    assert np.allclose(norm.bound, [[-1.0, 1.0]] * 3) and norm.coords.abs().max() <= 1.0 and norm.surface_stddev == 0.01
    with pytest.raises(AssertionError):
        Sdf3D(mesh, total_samples=100, device="cpu")
    small = utils_sdf.box_mesh(np.array([[1.0, 2.0], [1.0, 3.0], [0.0, 1.0]]))
    both = BatchedSdf3D([mesh, small], total_samples=2 ** 9, batch_size=64, device="cpu")
    assert len(both) == 2 * (2 ** 9 // 64 + 1) and len(both.datasets) == 2
    seen = set()
    for _ in range(16):
        inp, gt = both[0]
        seen.add(int(inp["dataset_index"]))
        assert inp["coords"].shape == (64, 3) and gt["sdf"].shape == (64, 1)
        lo, hi = both.datasets[int(inp["dataset_index"])].bound.T
        assert (inp["coords"].numpy() >= lo - 0.5).all() and (inp["coords"].numpy() <= hi + 0.5).all()
    assert seen == {0, 1}


# --------------------------------------------------------------------------- 7. refusals
def test_hip_ops_refuse_cpu_tensors_wrong_dtypes_and_shapes():
    from miso_amd import ops
    p, v, t = torch.zeros(4, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    for call in (lambda: ops.closest_all(p, v, t), lambda: ops.closest(p, v, t), lambda: ops.count_crossings_all(p, p, v, t),
                 lambda: ops.MeshIndex(v, t)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
    # (dtype and shape are checked after the device: tests/test_mesh_sdf.py)


def test_c_abi_refuses_bad_arguments_and_accepts_a_null_far_set():
    """argument checks come before any launch, so they run without a GPU; with n == 0 a valid call launches nothing"""
    from miso_amd import _lib
    lib = _lib.load()
    plan = _lib.MeshPlan()
    lo, hi = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    assert lib.miso_mesh_plan(lo, hi, 0.25, 0, ctypes.byref(plan)) == 0                    # an empty mesh: no workspace
    far = _lib.MeshPlan()
    assert lib.miso_mesh_plan(lo, hi, 2.0, 0, ctypes.byref(far)) == 0
    null, one = None, ctypes.c_void_p(16)
    bad = _lib.E_BADARG
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, None, null, null, 0, null, 3, 0, null, null, null, null, null) == 0
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, ctypes.byref(far), null, null, 0, null, 3, 0, null, null, null, null, null) == 0
    # a far set given in part; one of another mesh; a stride below 3; a negative n; outputs missing; misaligned vw / stats
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, None, null, null, 7, null, 3, 0, null, null, null, null, null) == bad
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, None, one, null, 0, null, 3, 0, null, null, null, null, null) == bad
    other = _lib.MeshPlan()
    assert lib.miso_mesh_plan(lo, hi, 2.0, 5, ctypes.byref(other)) == 0
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, ctypes.byref(other), one, one, 4, null, 3, 0, null, null, null, null, null) == bad
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, None, null, null, 0, null, 2, 0, null, null, null, null, null) == bad
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, None, null, null, 0, null, 3, -1, null, null, null, null, null) == bad
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, None, null, null, 0, one, 3, 4, null, null, null, null, null) == bad
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, None, null, null, 0, null, 3, 0, null, null, ctypes.c_void_p(4), null, null) == bad
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, None, null, null, 0, null, 3, 0, null, null, null, ctypes.c_void_p(4), null) == bad
    assert lib.miso_mesh_closest(None, null, null, 0, None, null, null, 0, null, 3, 0, null, null, null, null, null) == bad
    assert lib.miso_mesh_closest(ctypes.byref(other), null, null, 0, None, null, null, 0, null, 3, 0, null, null, null, null, null) == bad   # triangles, no workspace
    assert lib.miso_mesh_closest(ctypes.byref(plan), null, null, 0, None, null, null, 0, null, 3, 1 << 31, null, null, null, null, null) == _lib.E_TOOLARGE
    assert lib.miso_mesh_closest_all(null, 3, 0, null, 3, 0, null, 3, 0, null, null, null, null) == 0
    assert lib.miso_mesh_closest_all(null, 3, 0, null, 3, 2, null, 3, 0, null, null, null, null) == bad          # triangles without an array
    assert lib.miso_mesh_closest_all(null, 3, 0, null, 3, 0, null, 1, 0, null, null, null, null) == bad
    assert lib.miso_mesh_closest_all(null, 3, 0, null, 3, 0, one, 3, 4, null, null, null, null) == bad
    assert lib.miso_mesh_count_hits(ctypes.byref(plan), null, null, 0, null, 3, null, 3, 0, 0.0, 1.0, null, null) == 0
    assert lib.miso_mesh_count_hits(ctypes.byref(plan), null, null, 0, null, 3, null, 2, 0, 0.0, 1.0, null, null) == bad
    assert lib.miso_mesh_count_hits(ctypes.byref(plan), null, null, 0, one, 3, one, 3, 4, 0.0, 1.0, null, null) == bad
    assert lib.miso_mesh_count_hits(ctypes.byref(other), null, null, 0, null, 3, null, 3, 0, 0.0, 1.0, null, null) == bad
    assert lib.miso_mesh_count_hits_all(null, 3, 0, null, 3, 0, null, 3, null, 3, 0, 0.0, 1.0, null, null) == 0
    assert lib.miso_mesh_count_hits_all(null, 3, 0, null, 3, 0, null, 3, null, 3, -1, 0.0, 1.0, null, null) == bad
    assert lib.miso_mesh_count_hits_all(null, 3, 0, null, 3, 0, one, 3, one, 3, 4, 0.0, 1.0, null, null) == bad
