"""ICP without a GPU: the host solve of grid_opt/utils/utils_registration.py against hand-computed values, the float64
restatements of tests/icp_cases.py on the fixtures, registration_icp driven by those restatements in place of the device
operators, the refusals that are decided on the host, and the conditions the GPU tests (tests/test_icp.py) rely on the
fixtures to meet."""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

import icp_cases as ic
import nn_cases as nc


@contextlib.contextmanager
def float64_operators():
    """ops.IcpWorkspace = icp_cases.Workspace64 inside the block (as test_mesh_eval.float64_search replaces ops.nearest)"""
    from miso_amd import ops
    real = ops.IcpWorkspace
    ops.IcpWorkspace = ic.Workspace64
    try:
        yield
    finally:
        ops.IcpWorkspace = real


# --------------------------------------------------------------------------- the solve, by hand
def test_euler_update_is_rz_ry_rx():
    from miso_amd.grid_opt.utils.utils_registration import transform_vector6d_to_matrix4d as to_matrix
    h = math.pi / 2
    T = to_matrix(np.array([h, 0.0, 0.0, 1.0, 2.0, 3.0]))
    assert np.allclose(T[:3, :3], [[1, 0, 0], [0, 0, -1], [0, 1, 0]], atol=1e-15) and T[:3, 3].tolist() == [1.0, 2.0, 3.0]
    assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert np.allclose(to_matrix(np.array([0.0, 0.0, h, 0, 0, 0]))[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    # Ry(90) Rx(90) = [[0 1 0] [0 0 -1] [-1 0 0]]; the other order, Rx Ry, would be [[0 0 1] [1 0 0] [0 1 0]]
    assert np.allclose(to_matrix(np.array([h, h, 0.0, 0, 0, 0]))[:3, :3], [[0, 1, 0], [0, 0, -1], [-1, 0, 0]], atol=1e-15)
    assert np.allclose(ic._euler(np.array([0.3, -0.2, 0.5, 1, 2, 3])), to_matrix(np.array([0.3, -0.2, 0.5, 1, 2, 3])), atol=1e-15)


def _pair_sums(p, q, origin):
    p, q, o = np.asarray(p, float), np.asarray(q, float), np.asarray(origin, float)
    return len(p), (p - o).sum(0), (q - o).sum(0), ((q - o).T @ (p - o)).ravel()


def test_umeyama_from_sums_rotation_and_reflection():
    from miso_amd.grid_opt.utils.utils_registration import umeyama_from_sums
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 3], [0, 0, -3]], dtype=np.float64)
    P = ic.pose(25.0, 0.7)
    origin = (2.0, 1.5, 1.25)
    T = umeyama_from_sums(*_pair_sums(p + 5.0, ic.apply64(P, p + 5.0), origin), origin)
    assert np.allclose(T, P, atol=1e-13)
    # q = p mirrored in z: H = diag(2, 8, -18) / 6; the proper rotation that maximises tr(R H) is diag(-1, 1, -1) (the
    # axis of the smallest singular value is flipped), not the mirror itself
    T = umeyama_from_sums(*_pair_sums(p, p * [1, 1, -1], (0, 0, 0)))
    assert np.allclose(T[:3, :3], np.diag([-1.0, 1.0, -1.0]), atol=1e-14) and np.allclose(T[:3, 3], 0, atol=1e-14)
    assert np.linalg.det(T[:3, :3]) == pytest.approx(1.0)
    assert umeyama_from_sums(0.0, np.zeros(3), np.zeros(3), np.zeros(9)) is None


def test_tukey_weight_at_and_beyond_k():
    from miso_amd.grid_opt.utils.utils_registration import tukey_weight
    k = 0.01
    r = np.array([0.0, 0.005, -0.005, k, -k, np.nextafter(k, 1.0), 0.02, -1.0])
    assert tukey_weight(r, k).tolist() == [1.0, 0.5625, 0.5625, 0.0, 0.0, 0.0, 0.0, 0.0]
    # the same rule inside the restated sums: residual 0.005 along the normal, J = [p x n, n] = [0 0 0 0 0 1] at p = (0, 0, z)
    tgt, nrm = np.zeros((1, 3), np.float32), np.array([[0, 0, 1]], np.float32)
    for z, w in ((0.005, 0.5625), (0.01, 0.0), (0.02, 0.0)):
        moved = np.array([[0, 0, z]], np.float32)
        s, _, _ = ic.sums64(moved, np.array([z * z], np.float32), np.array([0]), tgt, nrm, 0.5, "point_to_plane", 0.01)
        zz = float(np.float32(z))
        assert s[0] == 1 and s[22] == pytest.approx(w, abs=1e-6) and s[29] == pytest.approx(w * zz * zz, rel=1e-5, abs=1e-18)


def test_solve_point_to_plane_refuses_a_singular_system():
    from miso_amd.grid_opt.utils import utils_registration as reg
    s = np.zeros(32)
    s[0] = 10
    assert reg.solve_point_to_plane(s) is None                      # A = 0
    A = np.diag([2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    s[2:23] = A[np.triu_indices(6)]
    s[23:29] = [-0.02, 0, 0, -5.0, 0, 0]
    T = reg.solve_point_to_plane(s)
    assert np.allclose(T, reg.transform_vector6d_to_matrix4d(np.array([0.01, 0, 0, 1.0, 0, 0])), atol=1e-15)
    s[23] = np.nan
    assert reg.solve_point_to_plane(s) is None


class _Scripted:
    """an IcpWorkspace whose evaluations are scripted: (fitness, rmse) per call, a regular point-to-plane system"""

    def __init__(self, script):
        self.script, self.calls, self.n, self.origin = list(script), [], 100, (0.0, 0.0, 0.0)

    def __call__(self, src, index, normals=None):
        return self

    def step(self, T, max_dist, kind="point_to_plane", tukey_k=None):
        fit, rmse = self.script[len(self.calls)]
        self.calls.append(np.array(T))
        s = np.zeros(32)
        s[0], s[1] = fit * self.n, rmse * rmse * fit * self.n
        s[2:23] = np.eye(6)[np.triu_indices(6)]
        s[23:29] = [0, 0, 0, -0.125, 0, 0]                              # update: x += 0.125
        return s


def test_convergence_rule_and_loop_ends():
    from miso_amd import ops
    from miso_amd.grid_opt.utils import utils_registration as reg
    assert reg.converged((0.5, 0.1), (0.5 + 5e-7, 0.1 - 5e-7), 1e-6, 1e-6)
    assert not reg.converged((0.5, 0.1), (0.5 + 2e-6, 0.1), 1e-6, 1e-6)          # fitness alone still moving
    assert not reg.converged((0.5, 0.1), (0.5, 0.1 + 2e-6), 1e-6, 1e-6)          # rmse alone still moving
    assert not reg.converged((0.5, 0.25), (0.5, 0.25 + 2.0 ** -20), 2.0 ** -20, 2.0 ** -20)      # strictly below
    index = ic.Index64(np.zeros((1, 3)))
    real = ops.IcpWorkspace
    try:
        # evaluated at init, then after every update; stops after the first pair of evaluations that agree
        ops.IcpWorkspace = w = _Scripted([(0.5, 0.1), (0.6, 0.05), (0.7, 0.04), (0.7, 0.04), (0.9, 0.0)])
        r = reg.registration_icp(np.zeros((100, 3)), index, None, None, 0.1, max_iteration=30)
        assert r.iterations == 3 and len(w.calls) == 4 and (r.fitness, r.inlier_rmse) == (0.7, pytest.approx(0.04))
        assert np.allclose(r.transformation[:3, 3], [0.375, 0, 0]) and np.allclose(w.calls[2][:3, 3], [0.25, 0, 0])
        ops.IcpWorkspace = w = _Scripted([(0.5, 0.1), (0.6, 0.05), (0.7, 0.04), (0.8, 0.03)])
        r = reg.registration_icp(np.zeros((100, 3)), index, None, None, 0.1, max_iteration=2)
        assert r.iterations == 2 and len(w.calls) == 3 and r.fitness == 0.7
        ops.IcpWorkspace = w = _Scripted([(0.5, 0.1)])
        r = reg.registration_icp(np.zeros((100, 3)), index, None, None, 0.1, max_iteration=0)
        assert r.iterations == 0 and r.fitness == 0.5
        # no inlier: the loop ends with the pose it was given
        ops.IcpWorkspace = w = _Scripted([(0.0, 0.0)])
        init = ic.pose(10.0, 0.3)
        r = reg.registration_icp(np.zeros((100, 3)), index, None, None, 0.1, init=init)
        assert r.iterations == 0 and np.array_equal(r.transformation, init) and r.fitness == 0.0 and r.inlier_rmse == 0.0
    finally:
        ops.IcpWorkspace = real
    with pytest.raises(ValueError, match="Unknown constraint type"):
        reg.registration_icp(np.zeros((1, 3)), index, kind="plane_to_plane")


# --------------------------------------------------------------------------- the restated loop on the fixtures
@pytest.mark.parametrize("kind", ["point_to_plane", "point_to_point"])
def test_icp_loop64_on_independent_samplings(kind):
    """icp_loop64 recovers the 3 deg / 5 cm offset of the fixture, coarse then fine, to what icp_cases.INDEPENDENT_REACHED
    records (the figures tests/test_icp.py holds the GPU run to, times two)."""
    T, fitness, rmse, _, trace = ic.loop64("independent", kind)
    f = ic.fixture()
    start = ic.pose_error(np.eye(4), f["pose"])
    assert start[0] == pytest.approx(0.05) and start[1] == pytest.approx(math.radians(3.0))
    dt, dr = ic.pose_error(T, f["pose"])
    print(f"{kind}: translation error {dt:.3e} m, rotation error {dr:.3e} rad, fitness {fitness:.4f}")
    want = ic.INDEPENDENT_REACHED[kind]
    assert dt <= want[0] * 1.01 and dr <= want[1] * 1.01
    assert 0.1 < fitness <= 1.0 and 0.0 < rmse < ic.FINE


def test_icp_loop64_exact_case():
    T, fitness, rmse, _, _ = ic.loop64("exact", "point_to_plane")
    dt, dr = ic.pose_error(T, ic.fixture()["pose"])
    assert dt <= 1e-7 and dr <= 1e-7 and fitness == 1.0 and rmse < 2e-7


@pytest.mark.parametrize("kind,iters", [("point_to_plane", 30), ("point_to_point", 3)])
def test_registration_icp_follows_the_restated_loop(kind, iters):
    """registration_icp with ops.IcpWorkspace replaced by the float64 restatement (same search, sums64 instead of the
    kernels) against icp_loop64, which forms J^T W J and the Umeyama covariance directly: the same iterates."""
    from miso_amd.grid_opt.utils import utils_registration as reg
    f = ic.fixture()
    coarse64 = ic.loop64_pass("independent", kind, "coarse")
    got = []
    with float64_operators():
        r = reg.registration_icp(f["src"], ic.Index64(f["tgt"]), f["tgt"], f["normals"], ic.COARSE, kind=kind,
                                 max_iteration=iters, callback=lambda i, T, fit, rmse: got.append(T))
        want = coarse64[4][:iters + 1]
        assert len(got) == len(want) == r.iterations + 1
        for a, b in zip(got, want):
            assert np.abs(a - b).max() <= 1e-10
        if kind == "point_to_plane":
            assert r.iterations == coarse64[3] and r.fitness == coarse64[1] and r.inlier_rmse == pytest.approx(coarse64[2], rel=1e-9)
            fine64 = ic.loop64_pass("independent", kind, "fine")
            r2 = reg.registration_icp(f["src"], ic.Index64(f["tgt"]), f["tgt"], f["normals"], ic.FINE, init=coarse64[0],
                                      kind=kind, loss=reg.TukeyLoss(ic.TUKEY_K), max_iteration=30)
            assert r2.iterations == fine64[3] and np.abs(r2.transformation - fine64[0]).max() <= 1e-10


# --------------------------------------------------------------------------- what is decided on the host
def test_align_multiple_submaps_raises():
    from miso_amd.grid_opt.align import icp
    with pytest.raises(NotImplementedError, match="pose-graph"):
        icp.align_multiple_submaps(None, None)


def test_refusals_without_gpu():
    from miso_amd import _lib, ops
    lib = _lib.load()
    x, d2, idx = torch.zeros(5, 3), torch.zeros(5), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.icp_transform(x, np.eye(4))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.icp_sums(x, d2, idx, x, x, max_dist=0.1)
    with pytest.raises(ops.MisoError, match="needs the targets' normals") as e:
        ops.icp_sums(x, d2, idx, x, None, max_dist=0.1, kind="point_to_plane")
    assert e.value.code == _lib.E_BADARG and e.value.what == "miso_icp_sums" and not isinstance(e.value, ops.NotCovered)
    with pytest.raises(ops.MisoError, match="unknown kind") as e:
        ops.icp_sums(x, d2, idx, x, x, max_dist=0.1, kind="plane")
    assert e.value.code == _lib.E_BADARG
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.icp_sums(x, d2, idx, x, None, max_dist=0.1, kind="point_to_point")
    # the entry points refuse bad arguments before any launch
    E = _lib.E_BADARG
    pose = (ctypes.c_float * 12)()
    assert lib.miso_icp_transform(None, 3, 4, pose, None, None) == E
    assert lib.miso_icp_transform(None, 3, 0, None, None, None) == E and lib.miso_icp_transform(None, 2, 0, pose, None, None) == E
    assert lib.miso_icp_workspace_bytes(-1) == 0 and lib.miso_icp_workspace_bytes(0) == 256
    assert lib.miso_icp_workspace_bytes(257) == 512 and lib.miso_icp_workspace_bytes(10 ** 8) == _lib.ICP_MAX_BLOCKS * 256
    assert _lib.ICP_SUMS == 32 == ic.SUMS
    assert lib.miso_icp_sums(None, None, None, 0, None, 3, 0, None, 0, 0.1, 1, 0, 0.0, None, None, None, None) == E
    plan = _lib.NnPlan()
    assert lib.miso_nn_normals(ctypes.byref(plan), None, None, 3, 0, 0.1, None, None, None) == E      # not a written plan
    lo = (ctypes.c_float * 3)(0, 0, 0)
    assert lib.miso_nn_plan(lo, lo, 0.1, 0, 4, ctypes.byref(plan)) == 0
    assert lib.miso_nn_normals(ctypes.byref(plan), None, None, 3, 0, 0.0, None, None, None) == E      # radius
    assert lib.miso_nn_normals(ctypes.byref(plan), None, None, 3, 5, 0.1, None, None, None) == E      # no arrays
    assert lib.miso_nn_normals(ctypes.byref(plan), None, None, 3, 0, 0.1, None, None, None) == 0      # nothing to do


# --------------------------------------------------------------------------- the fixtures' own conditions
def test_fixture_shapes_and_pose():
    f = ic.fixture()
    assert f["tgt"].shape == (6000, 3) and f["src"].shape == (5000, 3) and f["tgt"].dtype == np.float32
    assert np.allclose(np.linalg.norm(f["normals"], axis=1), 1.0)
    e = ic.exact_fixture()
    back = ic.apply64(f["pose"], e["src"])
    assert np.abs(back - e["tgt"][e["rows"]]).max() < 1e-6 and len(np.unique(e["rows"])) == 5000


def test_no_pair_sits_at_a_threshold():
    """Within relative 1e-5 of a threshold a float64 restatement and an fp32 search could disagree about a pair for
    reasons that are nobody's error.  No correspondence of the sums fixture lies that close to SUMS_MAX_DIST (in float64,
    at the pose the test uses: the identity), nor of the recovery fixtures to COARSE / FINE at their start, and no two
    targets lie that close to NORMALS_RADIUS.  The three pairs of placed_pairs() are there on purpose."""
    f = ic.fixture()
    for src, thresholds in ((f["src"], (ic.SUMS_MAX_DIST, ic.COARSE, ic.FINE)), (ic.exact_fixture()["src"], (ic.COARSE, ic.FINE))):
        d = np.sqrt(ic.nearest64(src, f["tgt"])[0])
        for th in thresholds:
            assert np.abs(d - th).min() > 1e-5 * th, th
    share = (np.sqrt(ic.nearest64(f["src"], f["tgt"])[0]) <= ic.SUMS_MAX_DIST).mean()
    assert 0.3 < share < 0.8                                           # inliers and outliers both
    t = f["tgt"].astype(np.float64)
    closest = np.inf
    for a in range(0, len(t), 500):
        d = np.sqrt(((t[a:a + 500, None, :] - t[None, :, :]) ** 2).sum(axis=2))
        closest = min(closest, np.abs(d - ic.NORMALS_RADIUS).min())
    assert closest > 1e-5 * ic.NORMALS_RADIUS
    src, tgt, max_dist = ic.placed_pairs()
    d2 = nc.true_d2(src, tgt, np.arange(3))
    assert d2[0] == max_dist ** 2 and d2[1] > max_dist ** 2 > d2[2] and d2[1] - d2[2] < 1e-6


def test_normals_fixture_has_an_eigen_gap():
    f = ic.fixture()
    normals, counts, gaps = ic.normals_reference()
    assert counts.min() >= 3 and (gaps >= 0.05).mean() >= 0.90
    # away from the edges (a third of the points at this radius) the neighbourhood lies in its face: the face's normal
    on_face = np.abs(np.abs((normals * f["normals"]).sum(axis=1)) - 1.0) < 1e-9
    assert on_face.mean() > 0.3 and gaps[on_face].min() > 0.05


def test_shape_mesh_is_the_fixture_shape():
    v, tri = ic.shape_mesh()
    a, b, c = (v[tri[:, k]] for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
    assert area == pytest.approx(2 * (12 + 10 + 7.5) + 2 * (0.6 + 0.8 + 0.48))
    assert v.min(axis=0).tolist() == [0, 0, 0] and v.max(axis=0).tolist() == [4.0, 3.0, 2.5]
