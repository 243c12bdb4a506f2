"""Marching cubes (the step after the path): the oracle against the third-party goldens
(scikit-image, tests/golden/mcubes.npz), the compiled case table against the oracle's derivation, and the HIP
sweeps against the oracle -- vertices and triangle indices bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import golden_cases as gc
import mcubes_cases as MC
from oracle import mcubes_ref as M

NAMES = ("sphere", "torus", "gyroid", "noise")
DEV = "cuda:0"


def G():
    return np.load(gc.golden_path("mcubes"))


def lexsorted(v):
    return v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))]


def test_case_table_properties():
    tab, cnt = M.case_table()
    assert tab.shape == (256, 15) and cnt.max() == 5 and cnt[0] == 0 and cnt[255] == 0
    for c in range(256):
        e = tab[c][tab[c] >= 0]
        assert len(e) == 3 * cnt[c]
        # every crossing edge of the case is used, and only crossing edges
        crossing = {k for k in range(12) if ((c >> M.EDGE_ENDS[k, 0]) & 1) != ((c >> M.EDGE_ENDS[k, 1]) & 1)}
        assert set(e.tolist()) == crossing
        # the complementary case covers the same edges
        assert set(tab[255 - c][tab[255 - c] >= 0].tolist()) == crossing


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_third_party_golden(name):
    g = G()
    u, iso = g[f"{name}_u"], float(g[f"{name}_iso"])
    v, f = M.marching_cubes(u, iso)
    assert v.dtype == np.float32 and f.dtype == np.int64 and f.max() == len(v) - 1
    gv = g[f"{name}_verts"]
    assert v.shape == gv.shape
    assert np.abs(lexsorted(v) - gv).max() <= 4e-6        # same edges crossed, same linear interpolation
    cu, cd = M.edge_manifold_counts(f)
    assert cu.max() == 2 and cd.max() == 1                # manifold, consistently oriented (open only at the volume border)
    area, vol = M.mesh_area_volume(v, f)
    if name != "noise":                                   # ambiguous cells: the two tables join them differently
        assert len(f) == int(g[f"{name}_faces"])
        assert abs(area - float(g[f"{name}_area"])) <= 1e-3 * float(g[f"{name}_area"])
    if name in ("sphere", "torus"):                       # closed surfaces
        assert cu.min() == 2 and len(v) - len(cu) + len(f) == (2 if name == "sphere" else 0)
        assert vol < 0                                    # raw normals point to the u < iso side
        assert abs(-vol - float(g[f"{name}_volume"])) <= 2e-3 * float(g[f"{name}_volume"])


def test_oracle_analytic_sphere_and_empty():
    n = 40
    grid = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).astype(np.float32)
    u = np.linalg.norm(grid - 19.3, axis=-1) - 12.7
    v, f = M.marching_cubes(u, 0.0)
    assert np.abs(np.linalg.norm(v - 19.3, axis=1) - 12.7).max() < 0.03          # chord error of linear interpolation
    area, vol = M.mesh_area_volume(v, f)
    assert abs(area / (4 * np.pi * 12.7 ** 2) - 1) < 5e-3 and abs(-vol / (4 / 3 * np.pi * 12.7 ** 3) - 1) < 5e-3
    v, f = M.marching_cubes(u, 1e3)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f = M.marching_cubes(u[:1], 0.0)                                          # no cells along x
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_compiled_case_table_equals_derivation():
    from miso_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_int8 * 4096)()
    assert lib.miso_mc_case_table(buf) == 0
    got = np.frombuffer(buf, dtype=np.int8).reshape(256, 16)
    tab, cnt = M.case_table()
    assert np.array_equal(got[:, :15], tab) and np.array_equal(got[:, 15], cnt.astype(np.int8))
    assert lib.miso_mc_case_table(None) == _lib.E_BADARG
    assert lib.miso_mc_words(0, 4, 4) == -1 and lib.miso_mc_words(2048, 2048, 2048) == -1
    assert lib.miso_mc_words(1, 4, 4) == 4 and lib.miso_mc_words(3, 3, 65) == 18 and lib.miso_mc_words(256, 256, 256) == 1 << 18
    # per row and chunk of 64 samples: one sign word, three vertex words, two work-list slots
    assert lib.miso_mc_workspace_bytes(3, 3, 65) == 18 * 40
    assert lib.miso_mc_classify(None, 4, 4, 4, 0.0, None, None, None) == _lib.E_BADARG
    assert lib.miso_mc_emit(4, 4, 4, None, None, 0, 0, None, None) == _lib.E_BADARG


def test_ply_roundtrip_and_normals(tmp_path):
    from miso_amd.grid_opt.utils import utils_sdf as US
    g = G()
    v, f = M.marching_cubes(g["sphere_u"], 0.0)
    mesh = US.TriangleMesh(v, f[:, [2, 1, 0]])
    mesh.apply_transform(np.array([[0, -1, 0, 1.0], [1, 0, 0, 2.0], [0, 0, 1, 3.0], [0, 0, 0, 1]]))
    mesh.compute_vertex_normals()
    c = mesh.vertices.mean(0)
    out = ((mesh.vertices - c) * mesh.vertex_normals).sum(1)
    assert (out > 0).all()                                 # flipped faces: normals point out of the sphere
    p = tmp_path / "m.ply"
    mesh.export_ply(str(p))
    back = US.read_ply(str(p))
    assert np.array_equal(back.triangles, mesh.triangles) and np.allclose(back.vertices, mesh.vertices, atol=1e-5)
    assert open(p, "rb").read(3) == b"ply"


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_marching_cubes_equals_oracle(name):
    from miso_amd import ops
    g = G()
    u, iso = g[f"{name}_u"], float(g[f"{name}_iso"])
    v, f = ops.marching_cubes(torch.from_numpy(u).to(DEV), iso)
    rv, rf = M.marching_cubes(u, iso)
    assert np.array_equal(f.cpu().numpy(), rf)
    assert np.array_equal(v.cpu().numpy(), rv)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 2, 5), (17, 16, 18), (33, 9, 70), (1, 8, 8), (5, 1, 7)])
def test_hip_marching_cubes_ragged_shapes(shape):
    from miso_amd import ops
    rs = np.random.RandomState(sum(shape))
    u = rs.standard_normal(shape).astype(np.float32)
    v, f = ops.marching_cubes(torch.from_numpy(u).to(DEV), 0.05)
    rv, rf = M.marching_cubes(u, 0.05)
    assert np.array_equal(f.cpu().numpy(), rf) and np.array_equal(v.cpu().numpy(), rv)
    v, f = ops.marching_cubes(torch.from_numpy(u).to(DEV), 100.0)               # nothing crosses
    assert v.shape == (0, 3) and f.shape == (0, 3)


@pytest.mark.gpu
def test_hip_marching_cubes_full_size_properties():
    """256^3 sphere + ripple: closed, consistently oriented, Euler characteristic 2, volume of the sphere."""
    from miso_amd import ops
    n = 256
    ax = torch.arange(n, device=DEV, dtype=torch.float32)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    r = torch.sqrt((x - 127.3) ** 2 + (y - 126.1) ** 2 + (z - 128.9) ** 2)
    u = r - 90.0 + 0.8 * torch.sin(0.21 * x) * torch.cos(0.17 * y)
    v, f = ops.marching_cubes(u, 0.0)
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    cu, cd = M.edge_manifold_counts(fn)
    assert cu.min() == 2 and cu.max() == 2 and cd.max() == 1
    assert len(vn) - len(cu) + len(fn) == 2
    _, vol = M.mesh_area_volume(vn, fn)
    assert abs(-vol / (4 / 3 * np.pi * 90.0 ** 3) - 1) < 2e-3
    # every vertex lies on a lattice edge, at the zero of the linear interpolant
    frac = vn - np.floor(vn)
    assert ((frac > 0).sum(1) <= 1).all()


@pytest.mark.gpu
def test_save_mesh_of_a_gridnet(tmp_path):
    """save_mesh end to end: fused forward over the lattice -> HIP marching cubes -> PLY; equals the oracle run on
    the same volume, mapped to metres like the reference (utils_sdf.py:96-100)."""
    import test_grid_opt_mirror as tm
    from miso_amd.grid_opt.utils import utils_sdf as US
    case = gc.CASES["small"]
    net = tm.make_gridnet(case, DEV)
    bound = torch.tensor(case["bound"], dtype=torch.float32)
    res = 48
    with torch.no_grad():
        u = US.extract_fields(bound[:, 0], bound[:, 1], res, lambda p: net(p.to(DEV)), device=DEV)
    iso = float(np.median(u))                              # a random decoder's field need not cross zero
    verts, tris = US.extract_geometry(bound[:, 0], bound[:, 1], res, iso, lambda p: net(p.to(DEV)), device=DEV)
    rv, rf = M.marching_cubes(u, iso)
    lo, hi = bound[:, 0].numpy(), bound[:, 1].numpy()
    assert np.array_equal(tris, rf)
    assert np.allclose(verts, rv.astype(np.float64) / (res - 1.0) * (hi - lo) + lo, atol=1e-12)

    class Shifted(torch.nn.Module):
        def forward(self, p):
            return net(p) - iso

    T = torch.eye(4)
    T[:3, 3] = torch.tensor([1.0, -2.0, 0.5])
    mesh = US.save_mesh(Shifted(), bound, save_path=str(tmp_path / "sub" / "m.ply"), resolution=res, device=DEV,
                        transform=T)
    back = US.read_ply(str(tmp_path / "sub" / "m.ply"))
    assert len(back.triangles) == len(rf) and np.array_equal(back.triangles, mesh.triangles)
    assert mesh.vertex_normals.shape == mesh.vertices.shape


# ---------------------------------------------------------------------------------------------------------------
# Word logic of the sweeps: long rows, word boundaries, ties, non-finite samples, capacity, used buffers.
# The volumes are tests/mcubes_cases.py; the CPU tests pin that each case still reaches the code it exists for.
CASE_NAMES = tuple(MC.CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(u, iso, oracle vertices, oracle faces) of a named case: built once, shared, read-only."""
    u, iso = MC.build(name)
    with np.errstate(over="ignore"):                       # extremes-huge: ub - ua overflows, as it is meant to
        v, f = M.marching_cubes(u, iso)
    for a in (u, v, f):
        a.setflags(write=False)
    return u, iso, v, f


def cell_triangles(u, iso):
    """Triangle count of every cell, (nx-1, ny-1, nz-1), from the signs and the case table alone."""
    nx, ny, nz = u.shape
    below = u < iso
    c = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for k in range(8):
        dx, dy, dz = M.CORNERS[k]
        c |= below[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << k
    return M.case_table()[1][c]


def crossed_edges(u, iso):
    """The crossed lattice edges in vertex order: low sample (x, y, z) and axis, sorted by the vertex key."""
    nx, ny, nz = u.shape
    below = u < iso
    rows = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        a = np.argwhere(below[tuple(lo)] != below[tuple(hi)])
        rows.append(np.concatenate([a, np.full((len(a), 1), axis)], 1))
    e = np.concatenate(rows, 0)
    key = ((e[:, 0] * ny + e[:, 1]) * 3 + e[:, 3]) * nz + e[:, 2]
    return e[np.argsort(key)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_oracle_mesh_is_manifold(name):
    u, iso, v, f = case(name)
    assert v.dtype == np.float32 and f.dtype == np.int64 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    if len(f):
        assert f.min() >= 0 and f.max() == len(v) - 1
        cu, cd = M.edge_manifold_counts(f)
        assert cu.max() <= 2 and cd.max() <= 1
    else:
        assert len(v) == 0


@pytest.mark.parametrize("shape", MC.WORD_EDGE_SHAPES)
def test_case_word_edges_reaches_the_word_boundaries(shape):
    u, iso, v, f = case("word_edges-" + MC._tag(shape))
    nz = shape[2]
    assert (nz + 63) // 64 == {64: 1, 65: 2, 128: 2, 129: 3, 257: 5, 321: 6, 700: 11}[nz]
    below = u < iso
    if nz > 64:                                            # a z-edge from lane 63 into the next word's bit 0
        z = np.arange(63, nz - 1, 64)
        assert (below[:, :, z] != below[:, :, z + 1]).any()
    if nz > 65:                                            # a cell in lane 63 with triangles
        z = np.arange(63, nz - 1, 64)
        assert (cell_triangles(u, iso)[:, :, z] > 0).any()


def test_case_flat_and_blocks_shapes():
    for shape in MC.FLAT_SHAPES:
        u, iso, v, f = case("flat-" + MC._tag(shape))
        assert u.shape == shape and (len(f) > 0) == (shape[2] > 1)
    u, iso, v, f = case("blocks")
    nx, ny, nz = u.shape
    assert (nx * ny) % 4 == 1 and nx * ny * ((nz + 63) // 64) == 2 * 256 + 1 and len(f) > 0


def test_case_ties_vertices_sit_on_lattice_points():
    for name in ("ties-iso0", "ties-iso1"):
        u, iso, v, f = case(name)
        assert (u == iso).mean() > 0.15
        assert (v == np.floor(v)).all(1).sum() > 1000
    u, iso, v, f = case("ties-iso0")
    e = crossed_edges(u, iso)
    assert len(e) == len(v)
    # both ends occur: t == 0 (the low sample equals iso) and t == 1 (the high one does)
    on_axis = v[np.arange(len(v)), e[:, 3]] - e[np.arange(len(v)), e[:, 3]]
    assert (on_axis == 0).sum() > 100 and (on_axis == 1).sum() > 100


def test_case_neg_zero_equals_ties():
    u, iso, v, f = case("neg_zero")
    tu, tiso, tv, tf = case("ties-iso0")
    assert np.array_equal(u, tu) and np.signbit(u).sum() > np.signbit(tu).sum()
    assert np.array_equal(f, tf) and np.array_equal(v, tv)


def test_case_checker_crosses_every_edge():
    u, iso, v, f = case("checker")
    assert len(f) == 4 * 4 * 3 * 129
    assert len(v) == 4 * 4 * 130 + 5 * 3 * 130 + 5 * 4 * 129
    assert (cell_triangles(u, iso) == 4).all()


def test_case_non_finite_counts():
    u, iso, v, f = case("non_finite")
    assert np.isnan(u).sum() > 50 and np.isposinf(u).sum() > 50 and np.isneginf(u).sum() > 50
    assert np.isnan(v).any(1).sum() >= 100
    assert f.min() >= 0 and f.max() < len(v)


def test_case_extremes_reach_the_ends_of_fp32():
    u, iso, v, f = case("extremes-subnormal")
    tiny = np.finfo(np.float32).tiny
    assert (u != 0).mean() > 0.99 and (np.abs(u) < tiny).all() and len(f) > 0
    u, iso, v, f = case("extremes-huge")
    e = crossed_edges(u, iso)
    a, b = e[:, :3].copy(), e[:, :3].copy()
    b[np.arange(len(e)), e[:, 3]] += 1
    with np.errstate(over="ignore", invalid="ignore"):
        d = u[tuple(b.T)] - u[tuple(a.T)]
    assert np.isinf(d).sum() > 10                          # ub - ua overflows


def test_case_corner_straddle_constant_sizes():
    u, iso, v, f = case("corner")
    assert (len(v), len(f)) == (3, 1)
    u, iso, v, f = case("straddle")
    assert (len(v), len(f)) == (16, 24)
    assert (cell_triangles(u, iso)[:, :, [63, 191]] > 0).any((0, 1)).all()       # cells in lane 63
    for kind in ("above", "equal", "below"):
        u, iso, v, f = case("constant-" + kind)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_case_ellipsoid_is_a_closed_sphere():
    u, iso, v, f = case("ellipsoid")
    cu, cd = M.edge_manifold_counts(f)
    assert cu.min() == 2 and cu.max() == 2 and cd.max() == 1
    assert len(v) - len(cu) + len(f) == 2
    assert set((v[:, 2].astype(np.int64) >> 6).tolist()) == set(range(8))        # vertices in all 8 chunks


def check_shifted(meshes):
    """The surface does not depend on where the block sits: same faces, same x and y, and z - z0 within 2**-15.
    A vertex is float(z) + t in fp32: the two sums differ by at most half an ulp at 512 (2**-16) plus half an ulp
    at 32 (2**-20)."""
    v1, f1 = meshes[1]
    for z0 in MC.SHIFTS:
        v, f = meshes[z0]
        assert np.array_equal(f, f1) and len(f) > 0
        assert np.array_equal(v[:, :2], v1[:, :2])
        dz = (v[:, 2].astype(np.float64) - z0) - (v1[:, 2].astype(np.float64) - 1)
        assert np.abs(dz).max() <= 2.0 ** -15


def test_case_shifted_is_translation_invariant():
    check_shifted({z0: case(f"shifted-{z0}")[2:] for z0 in MC.SHIFTS})


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n.startswith("word_edges")] + ["ellipsoid"])
def test_oracle_offsets_against_float64_linear_zero(name):
    """Every oracle vertex is fl(a + t) of its edge's low sample a, with t the fp32 crossing; t lies within 2**-22
    of the float64 crossing (three fp32 roundings -- iso - ua, ub - ua, the quotient -- of 2**-24 relative each, and
    t <= 1)."""
    u, iso, v, f = case(name)
    e = crossed_edges(u, iso)
    assert len(e) == len(v)
    n = np.arange(len(e))
    a, b = e[:, :3].copy(), e[:, :3].copy()
    b[n, e[:, 3]] += 1
    ua, ub = u[tuple(a.T)], u[tuple(b.T)]
    t32 = (iso - ua) / (ub - ua)
    assert t32.dtype == np.float32
    want = a.astype(np.float32)
    want[n, e[:, 3]] += t32
    assert np.array_equal(v, want)
    ua, ub = ua.astype(np.float64), ub.astype(np.float64)
    t64 = (np.float64(iso) - ua) / (ub - ua)
    assert (t64 > 0).all() and (t64 <= 1).all()
    assert np.abs(t32.astype(np.float64) - t64).max() <= 2.0 ** -22


# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_mesh(name):
    from miso_amd import ops
    u, iso, _, _ = case(name)
    v, f = ops.marching_cubes(torch.from_numpy(u).to(DEV), float(iso))
    assert v.dtype == torch.float32 and f.dtype == torch.int64
    return v.cpu().numpy(), f.cpu().numpy()


def assert_mesh_equal(v, f, rv, rf):
    assert v.shape == rv.shape and f.shape == rf.shape and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    assert np.array_equal(f, rf)
    assert np.array_equal(np.isnan(v), np.isnan(rv))
    assert np.array_equal(v, rv, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_hip_marching_cubes_case_equals_oracle(name):
    _, _, rv, rf = case(name)
    v, f = device_mesh(name)
    assert_mesh_equal(v, f, rv, rf)


@pytest.mark.gpu
def test_hip_marching_cubes_shifted_block():
    check_shifted({z0: device_mesh(f"shifted-{z0}") for z0 in MC.SHIFTS})


@pytest.mark.gpu
def test_hip_marching_cubes_ellipsoid_properties():
    v, f = device_mesh("ellipsoid")
    cu, cd = M.edge_manifold_counts(f)
    assert cu.min() == 2 and cu.max() == 2 and cd.max() == 1
    assert len(v) - len(cu) + len(f) == 2


GUARD, FACE_FILL, VERT_FILL = 64, -7, 12345.0


def mc_through_abi(u, iso, ws, counts, cap_tris=None, cap_verts=None):
    """ops.marching_cubes replayed on the C ABI with the caller's workspace and counts (used or not) and the
    caller's capacities; outputs carry GUARD extra rows and are prefilled.  -> verts, faces, n_vert, n_tri."""
    from miso_amd import _lib, ops
    lib = _lib.load()
    nx, ny, nz = u.shape
    W = lib.miso_mc_words(nx, ny, nz)
    assert ws.numel() * 8 >= lib.miso_mc_workspace_bytes(nx, ny, nz) and counts.numel() >= 4 * W + 2
    d = torch.from_numpy(u).to(DEV)
    st = ops._stream(d)
    assert lib.miso_mc_classify(ops._ptr(d), nx, ny, nz, float(iso), ops._ptr(ws), ops._ptr(counts), st) == 0
    c = counts[:4 * W + 2]
    offs = torch.cat([torch.cumsum(c[:3 * W], 0, dtype=torch.int64), torch.cumsum(c[3 * W:4 * W], 0, dtype=torch.int64),
                      c[4 * W:].long()])
    n_vert, n_tri, tri_chunks, vert_chunks = (int(x) for x in offs[[3 * W - 1, 4 * W - 1, 4 * W, 4 * W + 1]].tolist())
    offs[:4 * W] -= c[:4 * W]
    faces = torch.full((n_tri + GUARD, 3), FACE_FILL, dtype=torch.int64, device=DEV)
    verts = torch.full((n_vert + GUARD, 3), VERT_FILL, dtype=torch.float32, device=DEV)
    cap_tris = n_tri if cap_tris is None else cap_tris(n_tri)
    cap_verts = n_vert if cap_verts is None else cap_verts(n_vert)
    assert lib.miso_mc_emit(nx, ny, nz, ops._ptr(ws), ops._ptr(offs), tri_chunks, cap_tris, ops._ptr(faces), st) == 0
    assert lib.miso_mc_vertices(ops._ptr(d), nx, ny, nz, float(iso), ops._ptr(ws), ops._ptr(offs), vert_chunks,
                                cap_verts, ops._ptr(verts), st) == 0
    return verts.cpu().numpy(), faces.cpu().numpy(), n_vert, n_tri


def mc_buffers(names, fill=0xFF):
    from miso_amd import _lib
    lib = _lib.load()
    shapes = [case(n)[0].shape for n in names]
    ws = torch.full((max(lib.miso_mc_workspace_bytes(*s) for s in shapes),), fill, dtype=torch.uint8, device=DEV)
    counts = torch.full((4 * (4 * max(lib.miso_mc_words(*s) for s in shapes) + 2),), fill, dtype=torch.uint8, device=DEV)
    return ws.view(torch.int64), counts.view(torch.int32)


@pytest.mark.gpu
def test_hip_marching_cubes_abi_with_used_buffers():
    """One workspace and one counts buffer, prefilled with 0xFF and never cleared, through three volumes of
    different sizes: the sweeps neither read stale words nor depend on zeroed memory."""
    names = ("word_edges-3x3x321", "corner", "checker")
    ws, counts = mc_buffers(names)
    assert (counts == -1).all()
    for name in names:
        u, iso, rv, rf = case(name)
        v, f, n_vert, n_tri = mc_through_abi(u, iso, ws, counts)
        assert (n_vert, n_tri) == (len(rv), len(rf))
        assert_mesh_equal(v[:n_vert], f[:n_tri], rv, rf)
        assert (f[n_tri:] == FACE_FILL).all() and (v[n_vert:] == VERT_FILL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["checker", "word_edges-5x4x257"])
@pytest.mark.parametrize("which", ["tris", "verts"])
def test_hip_marching_cubes_capacity_clamps(name, which):
    """Rows below the capacity are the oracle's; every row from the capacity on, the guard rows included, keeps
    its prefill; the calls succeed."""
    u, iso, rv, rf = case(name)
    ws, counts = mc_buffers((name,))
    n = len(rf) if which == "tris" else len(rv)
    assert n > 64
    for cap in (0, 1, n // 2, n - 1, n):
        kw = {"cap_tris" if which == "tris" else "cap_verts": lambda total, cap=cap: cap}
        v, f, n_vert, n_tri = mc_through_abi(u, iso, ws, counts, **kw)
        assert (n_vert, n_tri) == (len(rv), len(rf))
        ct, cv = (cap, n_vert) if which == "tris" else (n_tri, cap)
        assert np.array_equal(f[:ct], rf[:ct]) and (f[ct:] == FACE_FILL).all() and len(f) == n_tri + GUARD
        assert np.array_equal(v[:cv], rv[:cv]) and (v[cv:] == VERT_FILL).all() and len(v) == n_vert + GUARD
